// stft_geom.h -- launch geometry and frame arithmetic of the framed real-input plans (windowed STFT frames): pure integer
// logic, no HIP, no device code.  One definition for the kernels (kernels_stft.hip), the launcher and the host side
// (stft.cpp: fwt_describe answers from here without a device).
//
// `src` holds `signals` signals of L f32 back to back; frame f of signal s is the n floats from s L + f hop on, f < F =
// 1 + (L - n) / hop.  Frame g = s F + f is row g of `dst`: M + 1 = n / 2 + 1 samples {f32 re, f32 im} (spectrum) or M + 1
// f32 (power), no padding.  A frame is what a row is to the real-input plans (../real/real_geom.h), whose geometry this is:
//   n = 2 .. 64      k_stft_small<log2 n>: one frame per thread, 256 frames per 256-thread workgroup
//   n = 128 .. 4096  k_stft<log2 M>: RT = 16 adjacent frames per workgroup, threads, LDS and word map of k_real
// threads, LDS and frames per workgroup are fwr::geometry(n)'s, for both outputs.
//
// k_stft.  The LDS plane, its word map (fw2::row_word) and every access to it are k_real's, forward: the degrees are the
// second table of real_geom.h.  The signal side does not pass through LDS.
//
// k_stft_small.  A thread reads its own frame from global memory into registers: frames lie hop floats apart, so there is
// no contiguous real span to park, and no real parking.  The spectrum side is k_real_small's: thread t leaves its row at
// word t (n + 3) + j, and the 256 (n + 2)-word span leaves in 8-byte units, unit u from words small_spec_word(n, 2 u), + 1
// -- the rows "spectrum row" and "spectrum span" of the first table of real_geom.h.  The power side parks rows of M + 1
// words at the odd row stride small_power_stride(n) = (M + 1) | 1 -- M + 1 itself from n = 4 on, 3 at n = 2 -- and the
// 256 (M + 1)-word span leaves in 4-byte units, thread t taking words t + 256 i, i < M + 1: word w of the span at
//     small_power_word(n, w) = w + (w / (M + 1)) (stride - (M + 1))       (the identity from n = 4 on)
// Degree of every access = the largest number of distinct words on one bank (bank = word mod 32) within one 32-lane half of
// a wave, the rule of the 4-byte LDS accesses, over every half-wave of a full workgroup and every i or j:
//   n                                            2   4   8  16  32  64
//   power row    (word t stride + j)             1   1   1   1   1   1
//   power span   (word t + 256 i of the span)    2   1   1   1   1   1
// Both parkings fit the LDS of k_real_small, 256 (n + 3) words, which stays the figure fwt_describe reports.
#pragma once
#include <cstdint>

#include "../real/real_geom.h"

namespace fwt {

constexpr uint32_t MIN_LEN = fwr::MIN_LEN, MAX_LEN = fwr::MAX_LEN;
constexpr uint32_t SMALL_ROWS = fwr::SMALL_ROWS;  // frames per workgroup = threads of k_stft_small

constexpr uint32_t small_power_stride(uint32_t n) { return (n / 2 + 1) | 1u; }
constexpr uint32_t small_power_word(uint32_t n, uint32_t w) { return w + (w / (n / 2 + 1)) * (small_power_stride(n) - (n / 2 + 1)); }

using Geometry = fwr::Geometry;  // rows_per_block: frames per workgroup
constexpr Geometry geometry(uint32_t n) { return fwr::geometry(n); }
using fwr::blocks;  // ceil(frames / rows_per_block)

// frames per signal; L >= n, hop >= 1
constexpr uint64_t frames_per_signal(uint32_t n, uint32_t hop, uint64_t L) { return 1 + (L - n) / hop; }
// first float of frame g
constexpr uint64_t frame_start(uint64_t g, uint64_t F, uint64_t L, uint32_t hop) { return (g / F) * L + (g % F) * (uint64_t)hop; }
// every frame starts on an 8-byte boundary of a 16-byte aligned buffer: the 8-byte pair loads of k_real may be used
constexpr bool pair_loads(uint32_t hop, uint64_t L) { return hop % 2 == 0 && L % 2 == 0; }

}  // namespace fwt
