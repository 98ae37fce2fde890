// fft2d_kernels.h -- launch wrappers of kernels_fft2d.hip.  No device code: the host side (fft2d.cpp) is plain C++.
#pragma once
#include "../csrc/kernels.h"  // v2f, FWD / INV
#include "fft2d_geom.h"

namespace fw2 {

using fwa::v2f;

// Raises the dynamic-LDS limit of the row kernel a plan of this shape launches (both directions).
hipError_t setup_fft2d_kernels(uint32_t rows, uint32_t cols);
// The row launch of geometry(rows, cols) over `batch` images (rows x cols, row-major, back to back at buf), in place:
// every row its own DFT, times row_scale; on the fused path (rows, cols <= 32) every column too, times col_scale, and
// nothing is left for a second launch.  dir: fwa::FWD / fwa::INV; the scales are 1 or exact powers of two.
hipError_t launch_fft2d_rows(int dir, uint32_t rows, uint32_t cols, v2f *buf, uint64_t batch, float row_scale,
                             float col_scale, hipStream_t st);

}  // namespace fw2
