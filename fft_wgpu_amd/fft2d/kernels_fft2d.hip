// kernels_fft2d.hip -- the in-place row pass of the 2-D plans, for every width, and the fused one-launch kernel of images
// up to 32 x 32.  gfx950 only.  Geometry, the LDS word maps and their bank-conflict degrees: fft2d_geom.h.
//
// k_chunk2d<LGW, LGH> (cols <= 32): the streaming shape of k_chunk -- one 256-thread workgroup per 64-KiB chunk of the
// buffer, every wave walks its own 16 KiB front to back, here with 16 loads of 1 KiB (16 bytes = two samples per lane), all in
// flight before the first use.  The chunk is parked in LDS plane-wise; every thread transforms 32 / cols whole rows in
// registers (fft_reg<cols>) and writes them back in natural order; in the fused form (LGH >= 1; LGH = 0: rows only) every
// thread then transforms 32 / rows whole columns of the images of the chunk (fft_reg<rows>); the chunk leaves through the
// addresses it came in by.  The buffer descriptor ends with the data, so the partial last chunk of a buffer needs no bounds
// code: loads behind the end return 0, stores there are dropped (whole rows, or whole images in the fused form).  In place:
// a workgroup reads its chunk completely before it writes any of it.  No twiddles beyond those inside fft_reg.
//
// k_rows2d<LGW> (cols = 64 .. 4096): a workgroup owns RT adjacent rows of the batch * rows lines of the buffer; the register
// networks, threads and RT are k_strided's (fws::net_of, strided_net.h), but lane = t + T * r with t fastest -- a load
// instruction of T threads covers T adjacent samples of a row -- and the exchange runs on a line-major, XOR-swizzled word map
// (fw2::row_word).  64-bit tile base, 32-bit offsets inside a tile of at most 256 KiB; the descriptor ends with the last
// row of the buffer, and rows past it neither load nor store.
#include "../csrc/device_common.h"
#include "../strided/strided_net.h"
#include "fft2d_kernels.h"

namespace fw2 {

using namespace fwa;

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// cols <= 32: rows (and, fused, columns) inside one 64-KiB chunk
// ---------------------------------------------------------------------------
template <int LGW, int LGH, int DIR>
__global__ __launch_bounds__(CHUNK_THREADS, 2) void k_chunk2d(v2f *buf, uint64_t n_samples, float row_scale, float col_scale)
{
    constexpr int W = 1 << LGW, H = 1 << LGH;
    static_assert(W <= 32 && H <= 32 && CHUNK % (W * H) == 0 && CHUNK == 32 * CHUNK_THREADS, "whole images per chunk");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *re = reinterpret_cast<float *>(smem), *im = re + CHUNK_PLANE;
    const uint32_t tid = threadIdx.x;
    const uint64_t e0 = (uint64_t)one_launch_block() * CHUNK;
    const uint64_t left = n_samples - e0;
    const uint32_t valid = left < CHUNK ? (uint32_t)left * 8u : CHUNK * 8u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(buf + e0, 0, valid, 0x00020000);
    // wave w walks samples [2048 w, 2048 w + 2048) of the chunk: access i covers samples 2048 w + 128 i + 2 lane, + 1
    const uint32_t p0 = (tid >> 6) * 2048 + 2 * (tid & 63);
    const uint32_t park = chunk_word(p0);  // chunk_word(p0 + 128 i) = park + 132 i, chunk_word(p + 1) = chunk_word(p) + 1

    v4f y[16];
    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        y[i] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, p0 * 8, i * 1024, AUX_NT));
    });
    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        re[park + 132 * i] = y[i].x; im[park + 132 * i] = y[i].y;
        re[park + 132 * i + 1] = y[i].z; im[park + 132 * i + 1] = y[i].w;
    });
    __syncthreads();

    {   // rows: samples 32 tid .. 32 tid + 31 = 32 / W whole rows, words 33 tid + j: only this thread's own
        float *mr = re + 33 * tid, *mi = im + 33 * tid;
        static_for<0, 32 / W>([&](auto g_) {
            constexpr int g = decltype(g_)::value;
            v2f z[W];
            static_for<0, W>([&](auto j_) { constexpr int j = decltype(j_)::value; z[j] = v2f{mr[g * W + j], mi[g * W + j]}; });
            fft_reg<W, DIR>(z);
            static_for<0, W>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                const v2f v = z[brev<W>(k)] * row_scale;
                mr[g * W + k] = v.x; mi[g * W + k] = v.y;
            });
        });
    }
    __syncthreads();

    if constexpr (LGH >= 1) {
        // columns: thread g * W + c takes column c of the 32 / H images inside samples [g * 32 W, (g + 1) * 32 W)
        const uint32_t base = (tid >> LGW) * (32 * W) + (tid & (W - 1));
        static_for<0, 32 / H>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            v2f z[H];
            uint32_t w[H];
            static_for<0, H>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                w[j] = chunk_word(base + (k * H + j) * W);
                z[j] = v2f{re[w[j]], im[w[j]]};
            });
            fft_reg<H, DIR>(z);
            static_for<0, H>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                const v2f v = z[brev<H>(j)] * col_scale;
                re[w[j]] = v.x; im[w[j]] = v.y;
            });
        });
        __syncthreads();
    }

    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        y[i] = v4f{re[park + 132 * i], im[park + 132 * i], re[park + 132 * i + 1], im[park + 132 * i + 1]};
    });
    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, y[i]), rsrc, p0 * 8, i * 1024, AUX_NT);
    });
}

// ---------------------------------------------------------------------------
// cols >= 64: RT adjacent rows per workgroup, P points per thread, two or three stages
// ---------------------------------------------------------------------------
template <int LGW, int DIR>
__global__ __launch_bounds__(fws::geometry(1u << LGW).threads) void k_rows2d(v2f *buf, uint64_t lines, float scale,
                                                                              uint32_t xcd_swizzle)
{
    constexpr int N = 1 << LGW;
    constexpr fws::Net K = fws::net_of(LGW);
    constexpr int P = K.points, T = N / P, RT = K.tile_cols, LGT = ilog2c(T);
    static_assert(K.r0 * K.r1 * K.r2 == N && P % K.r0 == 0 && P % K.r1 == 0 && P % K.r2 == 0, "the stages cover a row");
    static_assert(T * RT == geometry(2, N).row_threads && N * RT * 4 == geometry(2, N).row_lds_bytes, "geometry");
    static_assert((uint64_t)N * RT * 8 <= (256u << 10), "a tile is at most 256 KiB: 32-bit offsets inside it");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xch = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & (T - 1), r = tid >> LGT;
    const uint64_t line0 = (uint64_t)xcd_map(xcd_swizzle) * RT;
    const uint64_t left = lines - line0;  // >= 1: the grid is ceil(lines / RT)
    const uint32_t have = left < (uint64_t)RT ? (uint32_t)left : (uint32_t)RT;
    const bool live = r < have;  // the last tile of the buffer is partial
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(buf + line0 * N, 0, have * (uint32_t)(N * 8), 0x00020000);
    const uint32_t voff = (r * N + t) * 8;

    v2f x[P];
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = v2f{0.0f, 0.0f}; });
    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = buf_load<AUX_NT>(rsrc, voff, m * T * 8); });

    auto word = [r](uint32_t d) { return row_word(row_swizzle(LGW), (uint32_t)N, r, d); };
    fws::stage<N, P, K.r0, 1, DIR>(x, t);
    fws::exchange<N, P, K.r0, 1, true>(x, xch, t, word);
    fws::stage<N, P, K.r1, K.r0, DIR>(x, t);
    if constexpr (K.r2 > 1) {
        fws::exchange<N, P, K.r1, K.r0, false>(x, xch, t, word);
        fws::stage<N, P, K.r2, K.r0 * K.r1, DIR>(x, t);
    }

    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; buf_store<AUX_NT>(x[m] * scale, rsrc, voff, m * T * 8); });
}

// ---- launch ---------------------------------------------------------------------------------------------------------
template <int LGW, int LGH>
static const void *chunk_kernel(int dir)
{
    return dir == FWD ? reinterpret_cast<const void *>(&k_chunk2d<LGW, LGH, FWD>)
                      : reinterpret_cast<const void *>(&k_chunk2d<LGW, LGH, INV>);
}
template <int LGW>
static const void *chunk_kernel_lgh(int lgh, int dir)
{
    switch (lgh) {
        case 0: return chunk_kernel<LGW, 0>(dir);
        case 1: return chunk_kernel<LGW, 1>(dir);
        case 2: return chunk_kernel<LGW, 2>(dir);
        case 3: return chunk_kernel<LGW, 3>(dir);
        case 4: return chunk_kernel<LGW, 4>(dir);
        case 5: return chunk_kernel<LGW, 5>(dir);
        default: return nullptr;
    }
}
template <int LGW>
static const void *rows_kernel(int dir)
{
    return dir == FWD ? reinterpret_cast<const void *>(&k_rows2d<LGW, FWD>) : reinterpret_cast<const void *>(&k_rows2d<LGW, INV>);
}

// the row kernel of a shape: k_chunk2d<log2 cols, fused ? log2 rows : 0> or k_rows2d<log2 cols>
static KernelLaunch rows_launch(uint32_t rows, uint32_t cols, int dir)
{
    if (rows < MIN_LEN || rows > MAX_LEN || (rows & (rows - 1)) || cols < MIN_LEN || cols > MAX_LEN || (cols & (cols - 1)))
        return {};
    const Geometry g = geometry(rows, cols);
    const int lgh = g.fused ? fws::ilog2u(rows) : 0;
    const void *k = nullptr;
    switch (fws::ilog2u(cols)) {
        case 1: k = chunk_kernel_lgh<1>(lgh, dir); break;
        case 2: k = chunk_kernel_lgh<2>(lgh, dir); break;
        case 3: k = chunk_kernel_lgh<3>(lgh, dir); break;
        case 4: k = chunk_kernel_lgh<4>(lgh, dir); break;
        case 5: k = chunk_kernel_lgh<5>(lgh, dir); break;
        case 6: k = rows_kernel<6>(dir); break;
        case 7: k = rows_kernel<7>(dir); break;
        case 8: k = rows_kernel<8>(dir); break;
        case 9: k = rows_kernel<9>(dir); break;
        case 10: k = rows_kernel<10>(dir); break;
        case 11: k = rows_kernel<11>(dir); break;
        case 12: k = rows_kernel<12>(dir); break;
        default: return {};
    }
    return {k, (uint32_t)g.row_threads, g.row_lds_bytes};
}

hipError_t setup_fft2d_kernels(uint32_t rows, uint32_t cols)
{
    for (int dir : {FWD, INV}) {
        const KernelLaunch k = rows_launch(rows, cols, dir);
        if (!k.kernel) return hipErrorInvalidValue;
        if (hipError_t e = raise_lds_limit(k); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_fft2d_rows(int dir, uint32_t rows, uint32_t cols, v2f *buf, uint64_t batch, float row_scale,
                             float col_scale, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const KernelLaunch k = rows_launch(rows, cols, dir);
    if (!k.kernel) return hipErrorInvalidValue;
    if (batch > (~0ull) / (8ull * rows * cols)) return hipErrorInvalidValue;
    const Geometry g = geometry(rows, cols);
    uint64_t lines = batch * rows;
    const uint64_t blocks = row_blocks(g, lines, cols);
    if (g.chunked) {
        if (hipError_t e = check_grid(blocks); e != hipSuccess) return e;
        uint64_t n_samples = lines * cols;
        void *args[] = {&buf, &n_samples, &row_scale, &col_scale};
        return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
    }
    uint32_t xcd_swizzle = 1;
    if (hipError_t e = check_grid(blocks, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&buf, &lines, &row_scale, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
}

}  // namespace fw2
