// strided_kernels.h -- launch wrappers of kernels_strided.hip.  No device code: the host side (strided.cpp) is plain C++.
#pragma once
#include "../csrc/kernels.h"  // v2f, FWD / INV
#include "strided_geom.h"

namespace fws {

using fwa::v2f;

// Raises the dynamic-LDS limit of every kernel a plan of length n can launch (both directions, both addressing forms).
hipError_t setup_strided_kernels(uint32_t n);
// The columns of `batch` matrices (n rows x howmany columns, row-major, back to back at buf), in place; one launch.
// dir: fwa::FWD / fwa::INV; every output is multiplied by `scale` (1 or 2^-log2 n) in the last stage.
hipError_t launch_strided(int dir, uint32_t n, v2f *buf, uint64_t howmany, uint64_t batch, float scale, hipStream_t st);

}  // namespace fws
