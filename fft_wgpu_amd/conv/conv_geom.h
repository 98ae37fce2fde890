// conv_geom.h -- launch geometry of the fused FFT-convolution plans: pure integer logic, no HIP, no device code.  One
// definition for the kernels (kernels_conv.hip), the launcher and the host side (conv.cpp: fwc_describe answers from here
// without a device).
//
// A plan takes `batch` rows of n samples {f32 re, f32 im} to ifft(fft(row) * filter[row mod F]) in one launch: the row
// stays in registers between the forward and the inverse transform.
//   n = 2 .. 32      k_conv_small<log2 n>: the streaming shape of k_chunk2d<log2 n, 0> -- one 256-thread workgroup per
//                    chunk of fw2::CHUNK = 8192 samples, thread t owning samples 32 t .. 32 t + 31 = 32 / n whole rows:
//                    rows_per_block = 8192 / n, blocks = ceil(batch * n / 8192)
//   n = 64 .. 4096   k_conv<log2 n>: the shape of k_rows2d -- RT = fws::net_of(log2 n).tile_cols adjacent rows per
//                    workgroup (16; 8 at 4096), T = n / points threads per row, lane = t + T r: blocks = ceil(batch / RT)
//
// LDS.  Both shapes use the word maps of fft2d_geom.h unchanged, with the accesses those kernels make, so the degrees
// stated there hold here: k_conv_small parks its chunk plane-wise at fw2::chunk_word (two planes of fw2::CHUNK_PLANE
// words, every access of degree 1); k_conv runs fws::exchange on fw2::row_word -- the two (2048, 4096: four) exchanges of
// the forward and of the inverse network write and read the same elements from the same lanes, degree 1 at every n.  The
// filter never passes through LDS.
#pragma once
#include <cstdint>

#include "../fft2d/fft2d_geom.h"
#include "../strided/strided_geom.h"

namespace fwc {

constexpr uint32_t MIN_LEN = 2, MAX_LEN = 4096;
constexpr uint32_t SMALL_MAX = fw2::CHUNK_MAX;     // n <= SMALL_MAX: k_conv_small

struct Geometry {
    int32_t threads = 0, lds_bytes = 0, rows_per_block = 0;
    bool small = false;
};

// n: a power of two in [MIN_LEN, MAX_LEN]
constexpr Geometry geometry(uint32_t n)
{
    Geometry g;
    if (n <= SMALL_MAX) {
        g.small = true; g.threads = (int32_t)fw2::CHUNK_THREADS; g.lds_bytes = fw2::CHUNK_LDS_BYTES;
        g.rows_per_block = (int32_t)(fw2::CHUNK / n);
    } else {
        const fws::Geometry s = fws::geometry(n);
        g.threads = s.threads; g.lds_bytes = s.lds_bytes; g.rows_per_block = s.tile_cols;
    }
    return g;
}

// rows_per_block divides 8192 / n rows exactly for n <= 32, so this is ceil(batch * n / 8192) there
constexpr uint64_t blocks(const Geometry &g, uint64_t batch)
{
    return batch / (uint64_t)g.rows_per_block + (batch % (uint64_t)g.rows_per_block ? 1 : 0);
}

}  // namespace fwc
