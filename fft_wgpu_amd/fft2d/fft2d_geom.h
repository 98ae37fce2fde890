// fft2d_geom.h -- launch geometry of the in-place 2-D plans: pure integer logic, no HIP, no device code.  One definition
// for the kernels (kernels_fft2d.hip), the launcher and the host side (fft2d.cpp: fw2_describe answers from here without
// a device).
//
// A plan transforms `batch` row-major images of rows x cols in place: a row pass over the batch * rows contiguous lines of
// cols samples, then the column pass of the strided-batch plans (fws_plan: fft_len = rows, howmany = cols).
//   rows <= 32 and cols <= 32   1 launch   k_chunk2d<LGW, LGH>: rows, then columns, inside one 64-KiB chunk
//   cols <= 32, rows >= 64      2 launches k_chunk2d<LGW, 0> (rows only), then the fws plan
//   cols >= 64                  2 launches k_rows2d<LGW>, then the fws plan
//
// k_chunk2d.  One 256-thread workgroup per chunk of CHUNK = 8192 samples (the last one of a buffer may be partial: whole
// rows, or whole images in the fused form, since rows * cols divides 8192).  The chunk is parked plane-wise -- real parts,
// then imaginary parts -- at word chunk_word(p) = p + p / 32 of its plane: CHUNK_PLANE = 8192 + 256 words, two planes =
// 67584 bytes, two workgroups per CU.  With the bank rule of the 4-byte LDS accesses (bank = word mod 32, the two 32-lane
// halves of a wave apart) every access is conflict-free (degree 1) at every width and height:
//   park / unpark   lane l moves samples 2 l and 2 l + 1 of a run of 128: words 2 l + k (l < 16), 2 l + 1 + k (l >= 16)
//   row phase       thread t owns samples 32 t .. 32 t + 31 (32 / cols whole rows): word 33 t + j, lanes 33 apart
//   column phase    thread t = g * cols + c owns column c of the images g * 32 / rows + k, k < 32 / rows, all inside
//                   samples [g * 32 cols, (g + 1) * 32 cols): element j at sample g * 32 cols + k * rows * cols + j * cols + c,
//                   word = that + g * cols + const(j, k): the 32 / cols values of g in a half are cols banks apart
//
// k_rows2d.  A workgroup owns RT adjacent rows of the whole buffer (a tile may span two images); RT, the threads and the
// register network are those of fws::geometry(cols) / fws::net_of: T = cols / points threads per row, lane = t + T * r.
// LDS: one plane of cols * RT words, row r line-major at r * cols, element d of a row at
//     d ^ ((((d >> a) & m) ^ (r * k)) & 31)            (a, m, k) = row_swizzle(log2 cols)
// -- a bijection of the row (only bits 0 .. 4 change, by bits above a >= 3 and by the row).  Degree of every access of the
// exchanges (writes elements r0 apart from adjacent threads, second exchange: runs of r0 adjacent elements r0 * r1 apart;
// reads adjacent elements), same bank rule, computed for every half-wave of the workgroup:
//   cols    64  128  256  512  1024  2048  4096
//   degree   1    1    1    1     1     1     1
// No skew words: row_lds_bytes = cols * RT * 4.
#pragma once
#include <cstdint>

#include "../strided/strided_geom.h"

namespace fw2 {

constexpr uint32_t MIN_LEN = fws::MIN_LEN, MAX_LEN = fws::MAX_LEN;
constexpr uint32_t CHUNK_MAX = 32;                 // cols <= CHUNK_MAX: k_chunk2d; rows <= CHUNK_MAX too: fused
constexpr uint32_t CHUNK = 8192, CHUNK_THREADS = 256;
constexpr uint32_t CHUNK_PLANE = CHUNK + CHUNK / 32;
constexpr int32_t CHUNK_LDS_BYTES = (int32_t)(2 * CHUNK_PLANE * 4);

constexpr uint32_t chunk_word(uint32_t p) { return p + (p >> 5); }

struct RowSwizzle {
    int a, m, k;
};
constexpr RowSwizzle row_swizzle(int lg_cols)
{
    return lg_cols == 6 ? RowSwizzle{3, 7, 8} : lg_cols == 7 ? RowSwizzle{4, 7, 8} : lg_cols == 8 ? RowSwizzle{3, 31, 17}
         : lg_cols == 9 ? RowSwizzle{4, 31, 17} : RowSwizzle{5, 31, 0};
}
constexpr uint32_t row_word(RowSwizzle s, uint32_t cols, uint32_t r, uint32_t d)
{
    return r * cols + (d ^ ((((d >> s.a) & (uint32_t)s.m) ^ (r * (uint32_t)s.k)) & 31u));
}

struct Geometry {
    int32_t launches = 0, row_threads = 0, row_lds_bytes = 0, row_tile = 0;  // row_tile: rows per workgroup (k_rows2d)
    bool chunked = false, fused = false;
};

// rows, cols: powers of two in [MIN_LEN, MAX_LEN]
constexpr Geometry geometry(uint32_t rows, uint32_t cols)
{
    Geometry g;
    if (cols <= CHUNK_MAX) {
        g.chunked = true; g.fused = rows <= CHUNK_MAX; g.launches = g.fused ? 1 : 2;
        g.row_threads = (int32_t)CHUNK_THREADS; g.row_lds_bytes = CHUNK_LDS_BYTES;
    } else {
        const fws::Geometry s = fws::geometry(cols);
        g.launches = 2; g.row_tile = s.tile_cols; g.row_threads = s.threads; g.row_lds_bytes = s.lds_bytes;
    }
    return g;
}

// workgroups of the row launch over `lines` = batch * rows lines of cols samples
constexpr uint64_t row_blocks(const Geometry &g, uint64_t lines, uint32_t cols)
{
    return g.chunked ? (lines * cols + CHUNK - 1) / CHUNK : (lines + (uint64_t)g.row_tile - 1) / (uint64_t)g.row_tile;
}

}  // namespace fw2
