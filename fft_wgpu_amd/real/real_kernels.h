// real_kernels.h -- launch wrappers of kernels_real.hip.  No device code: the host side (real.cpp) is plain C++.
#pragma once
#include "../csrc/kernels.h"  // FWD / INV
#include "real_geom.h"

namespace fwr {

// Raises the dynamic-LDS limit of the kernel a plan of this length launches (both directions).
hipError_t setup_real_kernels(uint32_t n);
// One launch of geometry(n) over `batch` rows.  dir = fwa::FWD: `real` (batch rows of n f32) -> `spec` (batch rows of
// n / 2 + 1 samples {re, im}); dir = fwa::INV: `spec` -> `real`, times `scale` (1 or an exact power of two).  The side
// that is read is never written.
hipError_t launch_real(int dir, uint32_t n, float *real, float *spec, uint64_t batch, float scale, hipStream_t st);

}  // namespace fwr
