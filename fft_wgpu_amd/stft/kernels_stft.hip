// kernels_stft.hip -- the framed real-input plans: rfft (or its squared modulus) of overlapping, windowed frames of long
// real signals in one launch, n = 2 .. 4096.  gfx950 only.  Geometry, frame arithmetic and the LDS word maps: stft_geom.h.
//
// Frame g = s F + f is the n floats from src + s L + f hop on; it takes the place of row g of the real-input plans
// (../real/kernels_real.hip, whose forward arithmetic this is): z[j] = x[2j] w[2j] + i x[2j+1] w[2j+1], Z = FFT_M(z),
//     X[k] = (Z[k] + conj Zr[k]) / 2 + W_n^k (Z[k] - conj Zr[k]) / (2 i)     k < M,  Zr[k] = Z[(M - k) mod M]   (split_fwd)
//     X[M] = Re Z[0] - Im Z[0]
// and row g of dst receives X[0 .. M] (8-byte samples) or |X[0 .. M]|^2 (4-byte values), chosen by a uniform branch at the
// store: the bins are computed before it.
//
// Signal side.  Adjacent frames of a workgroup may belong to different signals, and L is anything: every lane forms its own
// 64-bit address, and a lane without a frame (the last workgroup is partial) issues no load.  Signal and window are read with
// the default cache policy -- neighbouring frames and every workgroup read them again.  PAIR (hop and L even: every frame
// starts on an 8-byte boundary) reads 8-byte pairs; otherwise every sample is a 4-byte load of its own, kept apart (sample()
// below) so that no access is wider than the 4 bytes it is aligned to.  The window (4 n bytes at a 16-byte aligned base) is
// always read in pairs.  WIN = false is the rectangular form: no window pointer is touched and no product is formed.
//
// k_stft_small<LGN> (n <= 64): one frame per thread, 256 per workgroup, fft_reg<M> and compile-time split twiddles; the
// result rows are parked in LDS at odd strides and leave as one contiguous span.  k_stft<LGM> (M = 64 .. 2048): k_real's
// forward form -- RT adjacent frames per workgroup, thread (t, r) holds elements t + T m of frame row0 + r, the stages and
// exchanges of fws on the word map fw2::row_word, the mirror through the same LDS plane -- with one descriptor on the dst
// side that ends with the last frame the workgroup owns.
//
// split_fwd, small_tw, unpark and the mirror phase restate kernels_real.hip's (that unit is frozen by its tests).
#include "../csrc/device_common.h"
#include "../strided/strided_net.h"
#include "stft_kernels.h"

namespace fwt {

using namespace fwa;

// X[k] from Z[k] and zr = Z[(M - k) mod M]; wo(o) = W_n^k * o
template <class Tw>
__device__ __forceinline__ v2f split_fwd(v2f z, v2f zr, Tw wo)
{
    const v2f e = v2f{z.x + zr.x, z.y - zr.y} * 0.5f;  // (Z + conj Zr) / 2
    const v2f o = v2f{z.y + zr.y, zr.x - z.x} * 0.5f;  // (Z - conj Zr) / (2 i)
    return e + wo(o);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(float *base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
template <int AUX>
__device__ __forceinline__ void buf_store32(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, AUX);
}

// One 4-byte sample.  A relaxed load at wavefront scope is a plain load that is never fused with its neighbour into one
// 8-byte access, which a frame that starts on an odd float would not be aligned for.
__device__ __forceinline__ float sample(const float *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// One 8-byte pair of a frame that starts on an 8-byte boundary, likewise never fused into a 16-byte access.
__device__ __forceinline__ v2f sample_pair(const float *p)
{
    return __builtin_bit_cast(v2f, __hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
}
// z[j] of a frame: {x[2j], x[2j+1]}, times {w[2j], w[2j+1]}
template <bool PAIR, bool WIN>
__device__ __forceinline__ v2f load_z(const float *frame, const float *window, uint32_t j)
{
    v2f z;
    if constexpr (PAIR) z = sample_pair(frame + 2 * j);
    else z = v2f{sample(frame + 2 * j), sample(frame + 2 * j + 1)};
    if constexpr (WIN) {
        const v2f w = *reinterpret_cast<const v2f *>(window + 2 * j);
        z = v2f{z.x * w.x, z.y * w.y};
    }
    return z;
}

// ---------------------------------------------------------------------------
// n <= 64: one frame per thread, 256 frames per workgroup
// ---------------------------------------------------------------------------
// W_n^k, k < n / 2, the value fws::g_tw holds, as a compile-time constant.  The products stay full complex multiplications
// even where a factor is 0 or 1: a NaN in either part of an operand then reaches both parts of the product.
template <int N, int K>
__device__ __forceinline__ v2f small_tw()
{
    constexpr float c = (float)cx_cos2pi(K, N), s = (float)-cx_sin2pi(K, N);
    return v2f{c, s};
}

// The first `units` 8-byte units of a span, thread tid taking units tid + 256 i, i < UNITS: LDS word(2 u), + 1 -> global.
template <int UNITS, class Word>
__device__ __forceinline__ void unpark(__amdgpu_buffer_rsrc_t rsrc, const float *lds, uint32_t tid, uint32_t units, Word word)
{
    static_for<0, UNITS>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        const uint32_t w = word(2 * (tid + SMALL_ROWS * i));
        const v2f y = v2f{lds[w], lds[w + 1]};
        if (tid + SMALL_ROWS * i < units) buf_store<AUX_NT>(y, rsrc, tid * 8, i * SMALL_ROWS * 8);
    });
}
// The same in 4-byte units: the first `words` words of a span, thread tid taking words tid + 256 i, i < WORDS.
template <int WORDS, class Word>
__device__ __forceinline__ void unpark32(__amdgpu_buffer_rsrc_t rsrc, const float *lds, uint32_t tid, uint32_t words, Word word)
{
    static_for<0, WORDS>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        const float y = lds[word(tid + SMALL_ROWS * i)];
        if (tid + SMALL_ROWS * i < words) buf_store32<AUX_NT>(y, rsrc, tid * 4, i * SMALL_ROWS * 4);
    });
}

template <int LGN, bool PAIR, bool WIN>
__global__ __launch_bounds__(SMALL_ROWS) void k_stft_small(const float *src, const float *window, float *dst, uint64_t frames,
                                                            uint64_t per_signal, uint64_t sig_len, uint32_t hop, uint32_t power)
{
    constexpr int N = 1 << LGN, M = N / 2;
    static_assert(N >= (int)MIN_LEN && N <= (int)fwr::SMALL_MAX, "one frame per thread");
    static_assert(small_power_stride(N) <= N + 3, "the power parking fits the spectrum parking");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lds = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * SMALL_ROWS;
    const uint64_t left = frames - row0;  // >= 1: the grid is ceil(frames / 256)
    const uint32_t have = left < (uint64_t)SMALL_ROWS ? (uint32_t)left : SMALL_ROWS;
    const bool live = tid < have;

    v2f z[M];
    static_for<0, M>([&](auto j_) { constexpr int j = decltype(j_)::value; z[j] = v2f{0.0f, 0.0f}; });
    if (live) {
        const float *frame = src + frame_start(row0 + tid, per_signal, sig_len, hop);
        static_for<0, M>([&](auto j_) { constexpr int j = decltype(j_)::value; z[j] = load_z<PAIR, WIN>(frame, window, j); });
    }
    fft_reg<M, FWD>(z);  // Z[k] is left in z[brev<M>(k)]
    v2f x[M + 1];
    static_for<0, M>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        x[k] = split_fwd(z[brev<M>(k)], z[brev<M>((M - k) % M)], [](v2f o) { return cmul(o, small_tw<N, k>()); });
    });
    x[M] = v2f{z[0].x - z[0].y, 0.0f};
    if (power) {
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(dst + row0 * (M + 1), have * (uint32_t)((M + 1) * 4));
        float *prow = lds + tid * small_power_stride(N);
        if (live) static_for<0, M + 1>([&](auto k_) { constexpr int k = decltype(k_)::value; prow[k] = x[k].x * x[k].x + x[k].y * x[k].y; });
        __syncthreads();
        unpark32<M + 1>(rs, lds, tid, have * (M + 1), [](uint32_t w) { return small_power_word(N, w); });
    } else {
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(dst + row0 * (N + 2), have * (uint32_t)((N + 2) * 4));
        float *srow = lds + tid * (N + 3);
        if (live) static_for<0, M + 1>([&](auto k_) { constexpr int k = decltype(k_)::value; srow[2 * k] = x[k].x; srow[2 * k + 1] = x[k].y; });
        __syncthreads();
        unpark<M + 1>(rs, lds, tid, have * (M + 1), [](uint32_t w) { return fwr::small_spec_word(N, w); });
    }
}

// ---------------------------------------------------------------------------
// n >= 128: RT adjacent frames per workgroup, P points of the M-point network per thread
// ---------------------------------------------------------------------------
template <int LGM, bool PAIR, bool WIN>
__global__ __launch_bounds__(fws::geometry(1u << LGM).threads) void k_stft(const float *src, const float *window, float *dst,
                                                                            uint64_t frames, uint64_t per_signal, uint64_t sig_len,
                                                                            uint32_t hop, uint32_t power, uint32_t xcd_swizzle)
{
    constexpr int M = 1 << LGM, N = 2 * M;
    constexpr fws::Net K = fws::net_of(LGM);
    constexpr int P = K.points, T = M / P, RT = K.tile_cols, LGT = ilog2c(T);
    static_assert(K.r0 * K.r1 * K.r2 == M && P % K.r0 == 0 && P % K.r1 == 0 && P % K.r2 == 0, "the stages cover a frame");
    static_assert(T * RT == geometry(N).threads && M * RT * 4 == geometry(N).lds_bytes && RT == geometry(N).rows_per_block, "geometry");
    static_assert((uint64_t)(M + 1) * RT * 8 <= (512u << 10), "32-bit offsets inside a tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xch = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & (T - 1), r = tid >> LGT;
    const uint64_t row0 = (uint64_t)xcd_map(xcd_swizzle) * RT;
    const uint64_t left = frames - row0;  // >= 1: the grid is ceil(frames / RT)
    const uint32_t have = left < (uint64_t)RT ? (uint32_t)left : (uint32_t)RT;
    const bool live = r < have;  // the last tile of the buffer is partial
    const uint32_t unit = power ? 4u : 8u;  // bytes per output value
    const __amdgpu_buffer_rsrc_t rs_dst = rows_rsrc(dst + row0 * (M + 1) * (unit / 4), have * (uint32_t)(M + 1) * unit);
    const uint32_t doff = (r * (M + 1) + t) * unit;  // X[t] of frame r

    v2f x[P];
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = v2f{0.0f, 0.0f}; });
    if (live) {
        const float *frame = src + frame_start(row0 + r, per_signal, sig_len, hop);
        static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = load_z<PAIR, WIN>(frame, window, t + T * m); });
    }

    auto word = [r](uint32_t d) { return fw2::row_word(fw2::row_swizzle(LGM), (uint32_t)M, r, d); };
    fws::stage<M, P, K.r0, 1, FWD>(x, t);
    fws::exchange<M, P, K.r0, 1, true>(x, xch, t, word);
    fws::stage<M, P, K.r1, K.r0, FWD>(x, t);
    if constexpr (K.r2 > 1) {
        fws::exchange<M, P, K.r1, K.r0, false>(x, xch, t, word);
        fws::stage<M, P, K.r2, K.r0 * K.r1, FWD>(x, t);
    }

    // the mirror Z[(M - d) mod M] of every point d = t + T m, through the plane the exchanges used: split_fwd, one plane at
    // a time so that a thread never holds more than three planes of its points: the real parts give e.x and o.y, which take
    // the places of Re Z and Re Zr; the imaginary parts give e.y and o.x, and X[d] leaves
    // (fresh() hands every phase a copy of t the compiler cannot trace back: it then computes the LDS words of a phase where
    // they are used instead of keeping 2 * points of them alive across all four)
    float oy[P];
    const float x_m = x[0].x - x[0].y;  // X[M] of the frame, in thread 0
    auto fresh = [](uint32_t v) { asm volatile("" : "+v"(v)); return v; };
    uint32_t u = fresh(t);
    __syncthreads();  // the reads of the last exchange
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; xch[word(u + T * m)] = x[m].x; });
    __syncthreads();
    u = fresh(t);
    static_for<0, P>([&](auto m_) {
        constexpr int m = decltype(m_)::value;
        const float zx = x[m].x, rx = xch[word((M - u - T * m) & (M - 1))];
        x[m].x = (zx + rx) * 0.5f; oy[m] = (rx - zx) * 0.5f;
    });
    __syncthreads();
    u = fresh(t);
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; xch[word(u + T * m)] = x[m].y; });
    __syncthreads();
    u = fresh(t);
    if (live) {
        static_for<0, P>([&](auto m_) {
            constexpr int m = decltype(m_)::value;
            const float zy = x[m].y, ry = xch[word((M - u - T * m) & (M - 1))];
            const v2f e = v2f{x[m].x, (zy - ry) * 0.5f}, o = v2f{(zy + ry) * 0.5f, oy[m]};
            const v2f v = e + cmul(o, fws::tw_n<N>(t + T * m));
            if (power) buf_store32<AUX_NT>(v.x * v.x + v.y * v.y, rs_dst, doff, m * T * 4);
            else buf_store<AUX_NT>(v, rs_dst, doff, m * T * 8);
        });
        if (t == 0) {
            if (power) buf_store32<AUX_NT>(x_m * x_m, rs_dst, (r * (M + 1) + M) * 4, 0);
            else buf_store<AUX_NT>(v2f{x_m, 0.0f}, rs_dst, (r * (M + 1) + M) * 8, 0);
        }
    }
}

// ---- launch ---------------------------------------------------------------------------------------------------------
template <int LGN>
static const void *small_kernel(bool pair, bool win)
{
    if (pair) return win ? reinterpret_cast<const void *>(&k_stft_small<LGN, true, true>) : reinterpret_cast<const void *>(&k_stft_small<LGN, true, false>);
    return win ? reinterpret_cast<const void *>(&k_stft_small<LGN, false, true>) : reinterpret_cast<const void *>(&k_stft_small<LGN, false, false>);
}
template <int LGM>
static const void *rows_kernel(bool pair, bool win)
{
    if (pair) return win ? reinterpret_cast<const void *>(&k_stft<LGM, true, true>) : reinterpret_cast<const void *>(&k_stft<LGM, true, false>);
    return win ? reinterpret_cast<const void *>(&k_stft<LGM, false, true>) : reinterpret_cast<const void *>(&k_stft<LGM, false, false>);
}

// the kernel of a length: k_stft_small<log2 n> or k_stft<log2 n - 1>, in one of its four forms
static KernelLaunch stft_launch(uint32_t n, bool pair, bool win)
{
    if (n < MIN_LEN || n > MAX_LEN || (n & (n - 1))) return {};
    const Geometry g = geometry(n);
    const void *k = nullptr;
    switch (fws::ilog2u(n)) {
        case 1: k = small_kernel<1>(pair, win); break;
        case 2: k = small_kernel<2>(pair, win); break;
        case 3: k = small_kernel<3>(pair, win); break;
        case 4: k = small_kernel<4>(pair, win); break;
        case 5: k = small_kernel<5>(pair, win); break;
        case 6: k = small_kernel<6>(pair, win); break;
        case 7: k = rows_kernel<6>(pair, win); break;
        case 8: k = rows_kernel<7>(pair, win); break;
        case 9: k = rows_kernel<8>(pair, win); break;
        case 10: k = rows_kernel<9>(pair, win); break;
        case 11: k = rows_kernel<10>(pair, win); break;
        case 12: k = rows_kernel<11>(pair, win); break;
        default: return {};
    }
    return {k, (uint32_t)g.threads, g.lds_bytes};
}

hipError_t setup_stft_kernels(uint32_t n)
{
    for (bool pair : {false, true})
        for (bool win : {false, true}) {
            const KernelLaunch k = stft_launch(n, pair, win);
            if (!k.kernel) return hipErrorInvalidValue;
            if (hipError_t e = raise_lds_limit(k); e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t launch_stft(uint32_t n, uint32_t hop, uint64_t sig_len, uint64_t signals, bool power, const float *src, const float *window,
                       float *dst, hipStream_t st)
{
    if (hop == 0 || sig_len < n) return hipErrorInvalidValue;
    uint64_t per_signal = frames_per_signal(n, hop, sig_len);
    if (signals == 0) return hipSuccess;
    if (per_signal > (~0ull) / signals) return hipErrorInvalidValue;
    uint64_t frames = signals * per_signal;
    const KernelLaunch k = stft_launch(n, pair_loads(hop, sig_len), window != nullptr);
    if (!k.kernel) return hipErrorInvalidValue;
    if (frames > (~0ull) / (4ull * (n + 2))) return hipErrorInvalidValue;
    const Geometry g = geometry(n);
    const uint64_t grid = fwt::blocks(g, frames);
    uint32_t pw = power ? 1u : 0u;
    if (g.small) {
        if (hipError_t e = check_grid(grid); e != hipSuccess) return e;
        void *args[] = {&src, &window, &dst, &frames, &per_signal, &sig_len, &hop, &pw};
        return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
    }
    uint32_t xcd_swizzle = 1;
    if (hipError_t e = check_grid(grid, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&src, &window, &dst, &frames, &per_signal, &sig_len, &hop, &pw, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
}

}  // namespace fwt
