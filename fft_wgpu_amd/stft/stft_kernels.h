// stft_kernels.h -- launch wrappers of kernels_stft.hip.  No device code: the host side (stft.cpp) is plain C++.
#pragma once
#include "../csrc/kernels.h"
#include "stft_geom.h"

namespace fwt {

// Raises the dynamic-LDS limit of the kernels a plan of this length may launch (all four forms: pair or single loads,
// windowed or rectangular).
hipError_t setup_stft_kernels(uint32_t n);
// One launch of geometry(n) over signals * frames_per_signal(n, hop, sig_len) frames: `src` (signals signals of sig_len f32)
// -> `dst` (one row per frame: n / 2 + 1 samples {re, im}, or n / 2 + 1 f32 when `power`).  `window`: n f32, or nullptr for
// the rectangular form.  src and window are never written.
hipError_t launch_stft(uint32_t n, uint32_t hop, uint64_t sig_len, uint64_t signals, bool power, const float *src, const float *window,
                       float *dst, hipStream_t st);

}  // namespace fwt
