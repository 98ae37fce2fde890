// strided_geom.h -- launch geometry of the strided-batch (column) plans: pure integer logic, no HIP, no device code.
// One definition for the kernels (kernels_strided.hip instantiates exactly these networks), the launcher and the host side
// (strided.cpp: fws_describe answers from here without a device).
//
// A plan transforms the columns of `batch` row-major matrices of n rows x howmany columns in place.  A tile is `tile_cols`
// adjacent columns by all n rows of one matrix; every load / store instruction moves tile_cols * 8-byte row segments.
//   n <= 32        a thread holds a whole column (fft_reg<n>): no exchange, no LDS.  256 threads take 256 adjacent columns
//                  (16 tiles) per step and 32 / n steps, so that every workgroup moves 64 KiB whatever n is:
//                  tiles_per_wg = 512 / n.
//   64 .. 1024     two register stages r0 x r1 and one plane-wise exchange through LDS (real parts, then imaginary parts:
//                  n * 16 * 4 bytes); `points` per thread, n / points threads per column, 16 columns.  At n = 1024 this is
//                  k_p1_gen's shape: 512 threads x 32 points, a 64-KiB plane, two workgroups per CU.
//   2048, 4096     three stages 32 x 32 x (2 | 4) with 32 points per thread and two exchanges.  Both take ONE workgroup of
//                  1024 threads per CU with a 128-KiB plane: 2048 keeps 16 columns (128-byte row segments, the shape
//                  k_cols32<11> ships); 4096 x 16 would need 2048 threads and 256 KiB, so it drops to 8 columns (64-byte
//                  segments) rather than to fewer points in flight per CU.
// blocks = batch * ceil(ceil(howmany / tile_cols) / tiles_per_wg); tiles_per_wg = 1 above n = 32.
#pragma once
#include <cstdint>

namespace fws {

constexpr uint32_t MIN_LEN = 2, MAX_LEN = 4096;
constexpr uint32_t SMALL_MAX = 32, SMALL_THREADS = 256;

// the register network of one length: radices of the stages (r2 = 1: two stages), points per thread, tile width
struct Net {
    int r0, r1, r2, points, tile_cols;
};
constexpr Net net_of(int lg_n)
{
    return lg_n == 6 ? Net{8, 8, 1, 8, 16} : lg_n == 7 ? Net{16, 8, 1, 16, 16} : lg_n == 8 ? Net{16, 16, 1, 16, 16}
         : lg_n == 9 ? Net{32, 16, 1, 32, 16} : lg_n == 10 ? Net{32, 32, 1, 32, 16} : lg_n == 11 ? Net{32, 32, 2, 32, 16}
         : lg_n == 12 ? Net{32, 32, 4, 32, 8} : Net{0, 0, 0, 0, 0};
}

struct Geometry {
    int32_t tile_cols = 0, threads = 0, lds_bytes = 0, tiles_per_wg = 0;
};

constexpr int ilog2u(uint32_t n) { return n <= 1 ? 0 : 1 + ilog2u(n >> 1); }

// n: a power of two in [MIN_LEN, MAX_LEN]
constexpr Geometry geometry(uint32_t n)
{
    Geometry g;
    if (n <= SMALL_MAX) {
        g.tile_cols = 16; g.threads = (int32_t)SMALL_THREADS; g.lds_bytes = 0; g.tiles_per_wg = (int32_t)(512 / n);
    } else {
        const Net k = net_of(ilog2u(n));
        g.tile_cols = k.tile_cols; g.threads = (int32_t)(n / (uint32_t)k.points) * k.tile_cols;
        g.lds_bytes = (int32_t)(n * (uint32_t)k.tile_cols * 4u); g.tiles_per_wg = 1;
    }
    return g;
}

constexpr uint64_t wgs_per_matrix(const Geometry &g, uint64_t howmany)
{
    const uint64_t tiles = (howmany + (uint64_t)g.tile_cols - 1) / (uint64_t)g.tile_cols;
    return (tiles + (uint64_t)g.tiles_per_wg - 1) / (uint64_t)g.tiles_per_wg;
}

}  // namespace fws
