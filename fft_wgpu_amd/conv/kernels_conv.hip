// kernels_conv.hip -- the fused FFT-convolution plans: dst[b] = ifft(fft(src[b]) * filter[b mod F]) for batched rows of
// n = 2 .. 4096 samples in one launch.  gfx950 only.  Geometry and the LDS word maps: conv_geom.h (the maps and their
// bank-conflict degrees are those of ../fft2d/fft2d_geom.h).
//
// A row is loaded once, transformed forward, multiplied by its filter row (a spectrum in natural bin order; conjugated on
// use when CONJ), transformed back and stored once, times `scale` (1, or 1 / n: an exact power of two).  Filter row of
// row b: b mod F, the row base filter + (b mod F) * n computed in 64 bits.  src and filter are never written; dst may be
// src: a workgroup reads all of its rows before it stores any of them (a barrier lies in between in both kernels).
//
// k_conv_small<LGW, CONJ> (n <= 32): the streaming shape of k_chunk2d<LGW, 0> -- one 256-thread workgroup per 64-KiB chunk,
// every wave walks its own 16 KiB in 16 loads of 1 KiB (16 bytes per lane), the chunk is parked plane-wise at
// fw2::chunk_word, thread t owns samples 32 t .. 32 t + 31 = 32 / n whole rows.  Per row: fft_reg<n, FWD>, the outputs
// taken in natural order (z[brev<n>(k)]), times the filter sample of bin k, fft_reg<n, INV>, scale, back in natural order.
// The 32 filter samples of a thread's rows are loaded straight into registers (16 bytes at a time; the row of a thread's
// first row by one 64-bit modulo, the following ones by counting), right behind the chunk's own loads.  src and dst have
// one descriptor each with the same offsets; both end with the data, so the partial last chunk needs no bounds code for
// them: loads behind the end return 0, stores there are dropped.  Rows behind the end look up no filter sample.
//
// k_conv<LGW, CONJ> (n = 64 .. 4096): the shape of k_rows2d -- RT adjacent rows per workgroup, T = n / P threads per row,
// lane = t + T r, thread t of a row holds elements t + T m before and after each of the two networks (fws::stage /
// fws::exchange on fw2::row_word), so the multiply is x[m] *= H[t + T m] with no exchange of its own.  The first exchange
// of the inverse network follows the reads of the forward network's last one: it takes the form with the leading barrier.
// Filter samples are per-lane 8-byte loads, adjacent lanes of a row on adjacent samples; up to n = 256 (8 or 16 points per
// thread) they are issued before the forward network, from 512 on (32 points per thread: 64 more live registers would cost
// a wave per SIMD at 512 / 1024 and spill at 2048 / 4096) at the multiply, eight at a time.  64-bit tile base, 32-bit
// offsets inside a tile of at most 256 KiB; the descriptors end with the last row the workgroup owns, and rows behind it
// neither load, look up a filter sample, nor store.  Twiddles: fws::g_tw only.
#include "../csrc/device_common.h"
#include "../strided/strided_net.h"
#include "conv_kernels.h"

namespace fwc {

using namespace fwa;

typedef unsigned v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const v2f *base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<v2f *>(base), 0, bytes, 0x00020000);
}

template <bool CONJ>
__device__ __forceinline__ v2f filter_mul(v2f a, v2f h)
{
    if constexpr (CONJ) return cmul_conj(a, h);
    else return cmul(a, h);
}

// ---------------------------------------------------------------------------
// n <= 32: 32 / n whole rows per thread inside one 64-KiB chunk
// ---------------------------------------------------------------------------
template <int LGW, bool CONJ>
__global__ __launch_bounds__(fw2::CHUNK_THREADS, 2) void k_conv_small(const v2f *src, const v2f *filter, v2f *dst, uint64_t batch,
                                                                       uint64_t filters, float scale)
{
    constexpr int W = 1 << LGW, ROWS = 32 / W;
    constexpr uint32_t CHUNK = fw2::CHUNK;
    static_assert(W >= 2 && W <= 32 && CHUNK == 32 * fw2::CHUNK_THREADS, "whole rows per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *re = reinterpret_cast<float *>(smem), *im = re + fw2::CHUNK_PLANE;
    const uint32_t tid = threadIdx.x;
    const uint64_t e0 = (uint64_t)one_launch_block() * CHUNK;
    const uint64_t left = batch * W - e0;  // >= 1: the grid is ceil(batch * n / 8192)
    const uint32_t valid = left < CHUNK ? (uint32_t)left * 8u : CHUNK * 8u;
    const __amdgpu_buffer_rsrc_t rs_src = span_rsrc(src + e0, valid), rs_dst = span_rsrc(dst + e0, valid);
    // wave w walks samples [2048 w, 2048 w + 2048) of the chunk: access i covers samples 2048 w + 128 i + 2 lane, + 1
    const uint32_t p0 = (tid >> 6) * 2048 + 2 * (tid & 63);
    const uint32_t park = fw2::chunk_word(p0);  // chunk_word(p0 + 128 i) = park + 132 i, chunk_word(p + 1) = chunk_word(p) + 1

    v4f y[16];
    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        y[i] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rs_src, p0 * 8, i * 1024, AUX_NT));
    });

    // the filter samples of this thread's rows, two per register quad: h[g * W / 2 + i] = bins 2 i, 2 i + 1 of row g
    const uint64_t row = (e0 + 32 * tid) >> LGW;  // the first of this thread's rows
    v4f h[16];
    {
        uint64_t f = row % filters;
        static_for<0, ROWS>([&](auto g_) {
            constexpr int g = decltype(g_)::value;
            const bool live = row + g < batch;
            const v4f *hp = reinterpret_cast<const v4f *>(filter + f * W);
            static_for<0, W / 2>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                h[g * (W / 2) + i] = live ? hp[i] : v4f{0.0f, 0.0f, 0.0f, 0.0f};
            });
            if (++f == filters) f = 0;
        });
    }

    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        re[park + 132 * i] = y[i].x; im[park + 132 * i] = y[i].y;
        re[park + 132 * i + 1] = y[i].z; im[park + 132 * i + 1] = y[i].w;
    });
    __syncthreads();

    {   // samples 32 tid .. 32 tid + 31 = ROWS whole rows, words 33 tid + j: only this thread's own
        float *mr = re + 33 * tid, *mi = im + 33 * tid;
        static_for<0, ROWS>([&](auto g_) {
            constexpr int g = decltype(g_)::value;
            v2f z[W], u[W];
            static_for<0, W>([&](auto j_) { constexpr int j = decltype(j_)::value; z[j] = v2f{mr[g * W + j], mi[g * W + j]}; });
            fft_reg<W, FWD>(z);  // bin k is left in z[brev<W>(k)]
            static_for<0, W>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                const v4f q = h[g * (W / 2) + k / 2];
                u[k] = filter_mul<CONJ>(z[brev<W>(k)], (k & 1) ? v2f{q.z, q.w} : v2f{q.x, q.y});
            });
            fft_reg<W, INV>(u);
            static_for<0, W>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                const v2f v = u[brev<W>(j)] * scale;
                mr[g * W + j] = v.x; mi[g * W + j] = v.y;
            });
        });
    }
    __syncthreads();

    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        y[i] = v4f{re[park + 132 * i], im[park + 132 * i], re[park + 132 * i + 1], im[park + 132 * i + 1]};
    });
    static_for<0, 16>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, y[i]), rs_dst, p0 * 8, i * 1024, AUX_NT);
    });
}

// ---------------------------------------------------------------------------
// n >= 64: RT adjacent rows per workgroup, P points per thread, both networks back to back
// ---------------------------------------------------------------------------
template <int N, int DIR, bool FIRST, class Word>
__device__ __forceinline__ void network(v2f (&x)[fws::net_of(ilog2c(N)).points], float *xch, uint32_t t, Word word)
{
    constexpr fws::Net K = fws::net_of(ilog2c(N));
    constexpr int P = K.points;
    fws::stage<N, P, K.r0, 1, DIR>(x, t);
    fws::exchange<N, P, K.r0, 1, FIRST>(x, xch, t, word);
    fws::stage<N, P, K.r1, K.r0, DIR>(x, t);
    if constexpr (K.r2 > 1) {
        fws::exchange<N, P, K.r1, K.r0, false>(x, xch, t, word);
        fws::stage<N, P, K.r2, K.r0 * K.r1, DIR>(x, t);
    }
}

template <int LGW, bool CONJ>
__global__ __launch_bounds__(fws::geometry(1u << LGW).threads) void k_conv(const v2f *src, const v2f *filter, v2f *dst, uint64_t batch,
                                                                            uint64_t filters, float scale, uint32_t xcd_swizzle)
{
    constexpr int N = 1 << LGW;
    constexpr fws::Net K = fws::net_of(LGW);
    constexpr int P = K.points, T = N / P, RT = K.tile_cols, LGT = ilog2c(T);
    constexpr bool EARLY = P < 32;  // the filter samples before the forward network; otherwise at the multiply
    static_assert(K.r0 * K.r1 * K.r2 == N && P % K.r0 == 0 && P % K.r1 == 0 && P % K.r2 == 0, "the stages cover a row");
    static_assert(T * RT == geometry(N).threads && N * RT * 4 == geometry(N).lds_bytes && RT == geometry(N).rows_per_block, "geometry");
    static_assert((uint64_t)N * RT * 8 <= (256u << 10), "a tile is at most 256 KiB: 32-bit offsets inside it");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xch = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & (T - 1), r = tid >> LGT;
    const uint64_t row0 = (uint64_t)xcd_map(xcd_swizzle) * RT;
    const uint64_t left = batch - row0;  // >= 1: the grid is ceil(batch / RT)
    const uint32_t have = left < (uint64_t)RT ? (uint32_t)left : (uint32_t)RT;
    const bool live = r < have;  // the last tile of the buffer is partial
    const __amdgpu_buffer_rsrc_t rs_src = span_rsrc(src + row0 * N, have * (uint32_t)(N * 8));
    const __amdgpu_buffer_rsrc_t rs_dst = span_rsrc(dst + row0 * N, have * (uint32_t)(N * 8));
    const uint32_t voff = (r * N + t) * 8;

    v2f x[P];
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = v2f{0.0f, 0.0f}; });
    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = buf_load<AUX_NT>(rs_src, voff, m * T * 8); });
    // bin t of this row's filter row; a dead row keeps the pointer it is given and never uses it: its points are zeros
    // before and after the forward network and take no part in the multiply
    const v2f *hp = live ? filter + ((row0 + r) % filters) * N + t : filter;
    v2f h[EARLY ? P : 1];
    if constexpr (EARLY)
        if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; h[m] = hp[m * T]; });

    auto word = [r](uint32_t d) { return fw2::row_word(fw2::row_swizzle(LGW), (uint32_t)N, r, d); };
    network<N, FWD, true>(x, xch, t, word);
    if (live) {
        if constexpr (EARLY) {
            static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = filter_mul<CONJ>(x[m], h[m]); });
        } else {
            // eight samples in flight at a time: all P of them beside the P points would spill
            static_for<0, P / 8>([&](auto g_) {
                constexpr int g = decltype(g_)::value;
                v2f q[8];
                static_for<0, 8>([&](auto i_) { constexpr int i = decltype(i_)::value; q[i] = hp[(8 * g + i) * T]; });
                static_for<0, 8>([&](auto i_) { constexpr int i = decltype(i_)::value; x[8 * g + i] = filter_mul<CONJ>(x[8 * g + i], q[i]); });
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    }
    // The inverse network gets a copy of t the compiler cannot trace back: it then looks its twiddles up again where it uses
    // them.  With the plain t it keeps every twiddle of the forward network alive for the inverse one (the same table
    // entries, conjugated on use): 2 P registers more across both networks.  Compiler figures at P = 32, plain t against
    // this: 512 points 269 registers (one wave per SIMD) against 153 (three), 1024 points 256 and 56 B of scratch per
    // lane against 159 and none, 2048 / 4096 points 928 / 988 B of scratch against 232 / 124.  Below P = 32 the twiddles are
    // kept (74 .. 142 registers, no scratch).
    uint32_t u = t;
    if constexpr (P == 32) asm volatile("" : "+v"(u));
    network<N, INV, false>(x, xch, u, word);

    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; buf_store<AUX_NT>(x[m] * scale, rs_dst, voff, m * T * 8); });
}

// ---- launch ---------------------------------------------------------------------------------------------------------
template <int LGW>
static const void *small_kernel(bool conj)
{
    return conj ? reinterpret_cast<const void *>(&k_conv_small<LGW, true>) : reinterpret_cast<const void *>(&k_conv_small<LGW, false>);
}
template <int LGW>
static const void *rows_kernel(bool conj)
{
    return conj ? reinterpret_cast<const void *>(&k_conv<LGW, true>) : reinterpret_cast<const void *>(&k_conv<LGW, false>);
}

// the kernel of a length: k_conv_small<log2 n> or k_conv<log2 n>
static KernelLaunch conv_launch(uint32_t n, bool conj)
{
    if (n < MIN_LEN || n > MAX_LEN || (n & (n - 1))) return {};
    const Geometry g = geometry(n);
    const void *k = nullptr;
    switch (fws::ilog2u(n)) {
        case 1: k = small_kernel<1>(conj); break;
        case 2: k = small_kernel<2>(conj); break;
        case 3: k = small_kernel<3>(conj); break;
        case 4: k = small_kernel<4>(conj); break;
        case 5: k = small_kernel<5>(conj); break;
        case 6: k = rows_kernel<6>(conj); break;
        case 7: k = rows_kernel<7>(conj); break;
        case 8: k = rows_kernel<8>(conj); break;
        case 9: k = rows_kernel<9>(conj); break;
        case 10: k = rows_kernel<10>(conj); break;
        case 11: k = rows_kernel<11>(conj); break;
        case 12: k = rows_kernel<12>(conj); break;
        default: return {};
    }
    return {k, (uint32_t)g.threads, g.lds_bytes};
}

hipError_t setup_conv_kernels(uint32_t n)
{
    for (bool conj : {false, true}) {
        const KernelLaunch k = conv_launch(n, conj);
        if (!k.kernel) return hipErrorInvalidValue;
        if (hipError_t e = raise_lds_limit(k); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_conv(uint32_t n, bool conj_filter, const v2f *src, const v2f *filter, v2f *dst, uint64_t batch,
                       uint64_t filters, float scale, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const KernelLaunch k = conv_launch(n, conj_filter);
    if (!k.kernel || filters == 0) return hipErrorInvalidValue;
    if (batch > (~0ull) / (8ull * n) || filters > (~0ull) / (8ull * n)) return hipErrorInvalidValue;
    const Geometry g = geometry(n);
    const uint64_t grid = blocks(g, batch);
    if (g.small) {
        if (hipError_t e = check_grid(grid); e != hipSuccess) return e;
        void *args[] = {&src, &filter, &dst, &batch, &filters, &scale};
        return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
    }
    uint32_t xcd_swizzle = 1;
    if (hipError_t e = check_grid(grid, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&src, &filter, &dst, &batch, &filters, &scale, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
}

}  // namespace fwc
