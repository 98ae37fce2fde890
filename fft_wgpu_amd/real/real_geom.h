// real_geom.h -- launch geometry of the real-input plans (rfft / irfft): pure integer logic, no HIP, no device code.  One
// definition for the kernels (kernels_real.hip), the launcher and the host side (real.cpp: fwr_describe answers from here
// without a device).
//
// A plan takes `batch` rows of n f32 to `batch` rows of M + 1 = n / 2 + 1 samples {f32 re, f32 im} (forward) or back
// (inverse), out of place, in one launch: a row is read as M complex samples, transformed by an M-point network, and
// split (forward: after the network; inverse: before it).
//   n = 2 .. 64      k_real_small<log2 n>: one row per thread, 256 rows per 256-thread workgroup
//   n = 128 .. 4096  k_real<log2 M>: RT adjacent rows per workgroup on the network of fws::net_of(log2 M)
//
// k_real_small.  The 256 rows of a workgroup are one contiguous span on both sides: 256 n words (4 bytes each) of real
// data, 256 (n + 2) words of spectrum.  A span moves between global memory and LDS in units of 8 bytes, thread t taking
// units t + 256 i (i < M on the real side, i < M + 1 on the spectrum side), each as two 4-byte LDS accesses; in between
// thread t reads its own row from one parking and leaves the result row in the other, all 4-byte accesses.  Both parkings
// use the same LDS, one after the other (a barrier in between): word w of a span at
//     small_real_word(n, w) = w + w / n           row stride n + 1 words
//     small_spec_word(n, w) = w + w / (n + 2)     row stride n + 3 words
// so LDS = 256 (n + 3) words = small_lds_bytes(n).  Degree of every access = the largest number of distinct words on one
// bank (bank = word mod 32) within one 32-lane half of a wave, the rule of the 4-byte LDS accesses, computed over every
// half-wave of a full workgroup and every i (a partial workgroup touches a subset):
//   n                                            2   4   8  16  32  64
//   real span    (words 2 u, 2 u + 1 of unit u)  1   2   2   2   1   2
//   real row     (word t (n + 1) + j)            1   1   1   1   1   1
//   spectrum row (word t (n + 3) + j)            1   1   1   1   1   1
//   spectrum span                                2   2   2   3   2   2
// The row accesses -- n + (n + 2) per thread against 2 M + 2 (M + 1) span accesses -- are conflict-free because both row
// strides are odd.  A 2-way conflict of a 4-byte LDS store costs no time (the store's address and data transfer takes as
// long); on the loads of the unpark it is one extra cycle per half-wave.
//
// k_real.  RT = fws::net_of(log2 M).tile_cols adjacent rows per workgroup, T = M / points threads per row, lane = t + T r;
// threads and LDS are fws::geometry(M)'s: one plane of M * RT words, row r line-major, element d of a row at
// fw2::row_word(fw2::row_swizzle(log2 M), M, r, d) -- the map of k_rows2d, whose exchanges these are.  Degree, same rule,
// over every half-wave of the workgroup and every register index m:
//   n                                               128  256  512  1024  2048  4096
//   exchange writes (fws::exchange, both exchanges)   1    1    1     1     1     1
//   natural order   (element t + T m: the reads of    1    1    1     1     1     1
//                    the exchanges, the mirror's writes)
//   mirrored read   (element (M - t - T m) mod M,     2    2    2     2     2     2
//                    forward only)
// The mirrored read of an instruction is a descending run of T elements whose first one (t = 0) belongs to the aligned
// block of T above the other T - 1 (to element 0 at m = 0): that one lane meets a bank of the run, degree 2, one extra
// cycle per half-wave on 2 * points of the 4-byte reads of a thread.  The inverse mirrors in global memory, not in LDS.
#pragma once
#include <cstdint>

#include "../fft2d/fft2d_geom.h"
#include "../strided/strided_geom.h"

namespace fwr {

constexpr uint32_t MIN_LEN = 2, MAX_LEN = 4096;
constexpr uint32_t SMALL_MAX = 64;                 // n <= SMALL_MAX: k_real_small
constexpr uint32_t SMALL_ROWS = 256;               // rows per workgroup = threads of k_real_small

constexpr uint32_t small_real_word(uint32_t n, uint32_t w) { return w + w / n; }
constexpr uint32_t small_spec_word(uint32_t n, uint32_t w) { return w + w / (n + 2); }
constexpr int32_t small_lds_bytes(uint32_t n) { return (int32_t)(SMALL_ROWS * (n + 3) * 4); }

struct Geometry {
    int32_t threads = 0, lds_bytes = 0, rows_per_block = 0;
    bool small = false;
};

// n: a power of two in [MIN_LEN, MAX_LEN]
constexpr Geometry geometry(uint32_t n)
{
    Geometry g;
    if (n <= SMALL_MAX) {
        g.small = true; g.threads = (int32_t)SMALL_ROWS; g.lds_bytes = small_lds_bytes(n); g.rows_per_block = (int32_t)SMALL_ROWS;
    } else {
        const fws::Geometry s = fws::geometry(n / 2);
        g.threads = s.threads; g.lds_bytes = s.lds_bytes; g.rows_per_block = s.tile_cols;
    }
    return g;
}

constexpr uint64_t blocks(const Geometry &g, uint64_t batch)
{
    return (batch + (uint64_t)g.rows_per_block - 1) / (uint64_t)g.rows_per_block;
}

}  // namespace fwr
