// conv_kernels.h -- launch wrappers of kernels_conv.hip.  No device code: the host side (conv.cpp) is plain C++.
#pragma once
#include "../csrc/kernels.h"  // v2f
#include "conv_geom.h"

namespace fwc {

using fwa::v2f;

// Raises the dynamic-LDS limit of the kernels a plan of this length launches (filter as it is, and conjugated).
hipError_t setup_conv_kernels(uint32_t n);
// One launch of geometry(n) over `batch` rows: dst[b] = ifft(fft(src[b]) * h(filter[b mod filters])) * scale, unscaled
// ifft, h = conj when conj_filter.  src == dst is the in-place form; src and filter are never written.
hipError_t launch_conv(uint32_t n, bool conj_filter, const v2f *src, const v2f *filter, v2f *dst, uint64_t batch,
                       uint64_t filters, float scale, hipStream_t st);

}  // namespace fwc
