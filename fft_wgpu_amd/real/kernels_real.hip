// kernels_real.hip -- the real-input plans: rfft and irfft of batched rows in one launch, n = 2 .. 4096.  gfx950 only.
// Geometry, the LDS word maps and their bank-conflict degrees: real_geom.h.
//
// A row of n reals is read as M = n / 2 complex samples z[j] = x[2j] + i x[2j+1]; with Z = FFT_M(z) and the mirror
// Zr[k] = Z[(M - k) mod M]
//     X[k] = (Z[k] + conj Zr[k]) / 2 + W_n^k (Z[k] - conj Zr[k]) / (2 i)     k < M          (split_fwd)
//     X[M] = Re Z[0] - Im Z[0]
// and back, with Xr[k] = X[M - k] and Im X[0], Im X[M] replaced by 0 (selected away, never multiplied),
//     Z'[k] = (X[k] + conj Xr[k]) + i conj(W_n^k) (X[k] - conj Xr[k])         k < M          (split_inv)
// whose unscaled inverse transform z' holds n * irfft(X): x[2j] = Re z'[j], x[2j+1] = Im z'[j].  The scaled kind
// multiplies by 1 / n, an exact power of two, in the store.
//
// k_real_small<LGN> (n <= 64): one row per thread -- fft_reg<M> in registers and the split with compile-time twiddles
// (small_tw) -- and 256 rows per workgroup.  The 256 rows are one contiguous span on either side; it moves between global
// memory and LDS in 8-byte units, adjacent lanes on adjacent units (the park / unpark of k_chunk2d), and is parked at
// padded, odd row strides so that the per-thread row accesses are conflict-free.  The last workgroup is partial: units
// and rows past the end neither load nor store.
//
// k_real<LGM> (M = 64 .. 2048): the shape of k_rows2d -- a workgroup owns RT adjacent rows, thread t of a row holds
// elements t + T m before and after every stage (fws::stage / fws::exchange on the word map fw2::row_word).  Forward: after
// the last stage every thread fetches the mirror of its own points through the same LDS plane, real parts, then imaginary
// parts, and stores its X[d]; thread 0 of a row also stores X[M].  Inverse: a thread loads X[d] and X[M - d] from global
// memory (the mirrored run is a reversed contiguous run), forms Z', runs the stages and stores n floats.  Twiddles W_n^d,
// d < M, come from fws::g_tw.  64-bit tile base, 32-bit offsets inside the tile; one descriptor per side (row pitches 4 n
// and 8 (M + 1) bytes), each ending with the last row the workgroup owns; rows past it neither load nor store.  Spectrum
// rows start only 8-byte aligned: every access is 8 bytes.
#include "../csrc/device_common.h"
#include "../strided/strided_net.h"
#include "real_kernels.h"

namespace fwr {

using namespace fwa;

// X[k] from Z[k] and zr = Z[(M - k) mod M]; wo(o) = W_n^k * o
template <class Tw>
__device__ __forceinline__ v2f split_fwd(v2f z, v2f zr, Tw wo)
{
    const v2f e = v2f{z.x + zr.x, z.y - zr.y} * 0.5f;  // (Z + conj Zr) / 2
    const v2f o = v2f{z.y + zr.y, zr.x - z.x} * 0.5f;  // (Z - conj Zr) / (2 i)
    return e + wo(o);
}
// Z'[k] from X[k] and xr = X[M - k]; wb(b) = conj(W_n^k) * b
template <class Tw>
__device__ __forceinline__ v2f split_inv(v2f x, v2f xr, Tw wb)
{
    const v2f a = v2f{x.x + xr.x, x.y - xr.y};  // X + conj Xr
    const v2f c = wb(v2f{x.x - xr.x, x.y + xr.y});  // conj(W) (X - conj Xr)
    return v2f{a.x - c.y, a.y + c.x};  // a + i c
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(float *base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}

// ---------------------------------------------------------------------------
// n <= 64: one row per thread, 256 rows per workgroup
// ---------------------------------------------------------------------------
// W_n^k, k < n / 2, the value fws::g_tw holds, as a compile-time constant.  The products stay full complex multiplications
// even where a factor is 0 or 1: a NaN in either part of an operand then reaches both parts of the product.
template <int N, int K>
__device__ __forceinline__ v2f small_tw()
{
    constexpr float c = (float)cx_cos2pi(K, N), s = (float)-cx_sin2pi(K, N);
    return v2f{c, s};
}

// The first `units` 8-byte units of a span, thread tid taking units tid + 256 i, i < UNITS: global -> LDS word(2 u), + 1.
template <int UNITS, class Word>
__device__ __forceinline__ void park(__amdgpu_buffer_rsrc_t rsrc, float *lds, uint32_t tid, uint32_t units, Word word)
{
    v2f y[UNITS];
    static_for<0, UNITS>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        y[i] = v2f{0.0f, 0.0f};
        if (tid + SMALL_ROWS * i < units) y[i] = buf_load<AUX_NT>(rsrc, tid * 8, i * SMALL_ROWS * 8);
    });
    static_for<0, UNITS>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        const uint32_t w = word(2 * (tid + SMALL_ROWS * i));
        lds[w] = y[i].x; lds[w + 1] = y[i].y;
    });
}
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

template <int LGN, int DIR>
__global__ __launch_bounds__(SMALL_ROWS) void k_real_small(float *real, float *spec, uint64_t batch, float scale)
{
    constexpr int N = 1 << LGN, M = N / 2;
    static_assert(N >= (int)MIN_LEN && N <= (int)SMALL_MAX, "one row per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lds = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * SMALL_ROWS;
    const uint64_t left = batch - row0;  // >= 1: the grid is ceil(batch / 256)
    const uint32_t have = left < (uint64_t)SMALL_ROWS ? (uint32_t)left : SMALL_ROWS;
    const __amdgpu_buffer_rsrc_t rs_real = rows_rsrc(real + row0 * N, have * (uint32_t)(N * 4));
    const __amdgpu_buffer_rsrc_t rs_spec = rows_rsrc(spec + row0 * (N + 2), have * (uint32_t)((N + 2) * 4));
    auto real_word = [](uint32_t w) { return small_real_word(N, w); };
    auto spec_word = [](uint32_t w) { return small_spec_word(N, w); };
    float *rrow = lds + tid * (N + 1), *srow = lds + tid * (N + 3);  // this thread's row in either parking
    const bool live = tid < have;

    if constexpr (DIR == FWD) {
        park<M>(rs_real, lds, tid, have * M, real_word);
        __syncthreads();
        v2f z[M];
        static_for<0, M>([&](auto j_) { constexpr int j = decltype(j_)::value; z[j] = v2f{rrow[2 * j], rrow[2 * j + 1]}; });
        __syncthreads();  // every row is in registers: the spectrum parking may overwrite the real one
        fft_reg<M, FWD>(z);  // Z[k] is left in z[brev<M>(k)]
        static_for<0, M>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            const v2f v = split_fwd(z[brev<M>(k)], z[brev<M>((M - k) % M)], [](v2f o) { return cmul(o, small_tw<N, k>()); });
            if (live) { srow[2 * k] = v.x; srow[2 * k + 1] = v.y; }
        });
        if (live) { srow[2 * M] = z[0].x - z[0].y; srow[2 * M + 1] = 0.0f; }  // X[M]
        __syncthreads();
        unpark<M + 1>(rs_spec, lds, tid, have * (M + 1), spec_word);
    } else {
        park<M + 1>(rs_spec, lds, tid, have * (M + 1), spec_word);
        __syncthreads();
        v2f x[M + 1], z[M];
        static_for<0, M + 1>([&](auto k_) { constexpr int k = decltype(k_)::value; x[k] = v2f{srow[2 * k], srow[2 * k + 1]}; });
        __syncthreads();
        z[0] = v2f{x[0].x + x[M].x, x[0].x - x[M].x};  // Im X[0] and Im X[M] take no part
        static_for<1, M>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            z[k] = split_inv(x[k], x[M - k], [](v2f b) { return cmul_conj(b, small_tw<N, k>()); });
        });
        fft_reg<M, INV>(z);
        if (live)
            static_for<0, M>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                const v2f v = z[brev<M>(j)] * scale;
                rrow[2 * j] = v.x; rrow[2 * j + 1] = v.y;
            });
        __syncthreads();
        unpark<M>(rs_real, lds, tid, have * M, real_word);
    }
}

// ---------------------------------------------------------------------------
// n >= 128: RT adjacent rows per workgroup, P points of the M-point network per thread
// ---------------------------------------------------------------------------
template <int LGM, int DIR>
__global__ __launch_bounds__(fws::geometry(1u << LGM).threads) void k_real(float *real, float *spec, uint64_t batch, float scale,
                                                                            uint32_t xcd_swizzle)
{
    constexpr int M = 1 << LGM, N = 2 * M;
    constexpr fws::Net K = fws::net_of(LGM);
    constexpr int P = K.points, T = M / P, RT = K.tile_cols, LGT = ilog2c(T);
    static_assert(K.r0 * K.r1 * K.r2 == M && P % K.r0 == 0 && P % K.r1 == 0 && P % K.r2 == 0, "the stages cover a row");
    static_assert(T * RT == geometry(N).threads && M * RT * 4 == geometry(N).lds_bytes && RT == geometry(N).rows_per_block, "geometry");
    static_assert((uint64_t)(M + 1) * RT * 8 <= (512u << 10), "32-bit offsets inside a tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xch = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & (T - 1), r = tid >> LGT;
    const uint64_t row0 = (uint64_t)xcd_map(xcd_swizzle) * RT;
    const uint64_t left = batch - row0;  // >= 1: the grid is ceil(batch / RT)
    const uint32_t have = left < (uint64_t)RT ? (uint32_t)left : (uint32_t)RT;
    const bool live = r < have;  // the last tile of the buffer is partial
    const __amdgpu_buffer_rsrc_t rs_real = rows_rsrc(real + row0 * N, have * (uint32_t)(N * 4));
    const __amdgpu_buffer_rsrc_t rs_spec = rows_rsrc(spec + row0 * (N + 2), have * (uint32_t)((N + 2) * 4));
    const uint32_t roff = (r * M + t) * 8;        // z[t] of row r: the real row read as M complex samples
    const uint32_t soff = (r * (M + 1) + t) * 8;  // X[t] of row r

    v2f x[P];
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = v2f{0.0f, 0.0f}; });
    if constexpr (DIR == FWD) {
        if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = buf_load<AUX_NT>(rs_real, roff, m * T * 8); });
    } else {
        // X[M - d], d = t + T m: at (T - t) + T (P - 1 - m), T - t >= 1
        const uint32_t moff = (r * (M + 1) + T - t) * 8;
        if (live)
            static_for<0, P>([&](auto m_) {
                constexpr int m = decltype(m_)::value;
                v2f a = buf_load<AUX_NT>(rs_spec, soff, m * T * 8), b = buf_load<AUX_NT>(rs_spec, moff, (P - 1 - m) * T * 8);
                if constexpr (m == 0)
                    if (t == 0) { a.y = 0.0f; b.y = 0.0f; }  // Im X[0], Im X[M]: selected away
                const uint32_t d = t + T * m;
                x[m] = split_inv(a, b, [d](v2f c) { return cmul_conj(c, fws::tw_n<N>(d)); });
            });
    }

    auto word = [r](uint32_t d) { return fw2::row_word(fw2::row_swizzle(LGM), (uint32_t)M, r, d); };
    fws::stage<M, P, K.r0, 1, DIR>(x, t);
    fws::exchange<M, P, K.r0, 1, true>(x, xch, t, word);
    fws::stage<M, P, K.r1, K.r0, DIR>(x, t);
    if constexpr (K.r2 > 1) {
        fws::exchange<M, P, K.r1, K.r0, false>(x, xch, t, word);
        fws::stage<M, P, K.r2, K.r0 * K.r1, DIR>(x, t);
    }

    if constexpr (DIR == FWD) {
        // the mirror Z[(M - d) mod M] of every point d = t + T m, through the plane the exchanges used
        // split_fwd, one plane at a time so that a thread never holds more than three planes of its points: the real parts
        // give e.x and o.y, which take the places of Re Z and Re Zr; the imaginary parts give e.y and o.x, and X[d] leaves
        // (fresh() hands every phase a copy of t the compiler cannot trace back: it then computes the LDS words of a phase
        // where they are used instead of keeping 2 * points of them alive across all four)
        float oy[P];
        const float x_m = x[0].x - x[0].y;  // X[M] of the row, in thread 0
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
                buf_store<AUX_NT>(e + cmul(o, fws::tw_n<N>(t + T * m)), rs_spec, soff, m * T * 8);
            });
            if (t == 0) buf_store<AUX_NT>(v2f{x_m, 0.0f}, rs_spec, (r * (M + 1) + M) * 8, 0);
        }
    } else {
        if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; buf_store<AUX_NT>(x[m] * scale, rs_real, roff, m * T * 8); });
    }
}

// ---- launch ---------------------------------------------------------------------------------------------------------
template <int LGN>
static const void *small_kernel(int dir)
{
    return dir == FWD ? reinterpret_cast<const void *>(&k_real_small<LGN, FWD>) : reinterpret_cast<const void *>(&k_real_small<LGN, INV>);
}
template <int LGM>
static const void *rows_kernel(int dir)
{
    return dir == FWD ? reinterpret_cast<const void *>(&k_real<LGM, FWD>) : reinterpret_cast<const void *>(&k_real<LGM, INV>);
}

// the kernel of a length: k_real_small<log2 n> or k_real<log2 n - 1>
static KernelLaunch real_launch(uint32_t n, int dir)
{
    if (n < MIN_LEN || n > MAX_LEN || (n & (n - 1))) return {};
    const Geometry g = geometry(n);
    const void *k = nullptr;
    switch (fws::ilog2u(n)) {
        case 1: k = small_kernel<1>(dir); break;
        case 2: k = small_kernel<2>(dir); break;
        case 3: k = small_kernel<3>(dir); break;
        case 4: k = small_kernel<4>(dir); break;
        case 5: k = small_kernel<5>(dir); break;
        case 6: k = small_kernel<6>(dir); break;
        case 7: k = rows_kernel<6>(dir); break;
        case 8: k = rows_kernel<7>(dir); break;
        case 9: k = rows_kernel<8>(dir); break;
        case 10: k = rows_kernel<9>(dir); break;
        case 11: k = rows_kernel<10>(dir); break;
        case 12: k = rows_kernel<11>(dir); break;
        default: return {};
    }
    return {k, (uint32_t)g.threads, g.lds_bytes};
}

hipError_t setup_real_kernels(uint32_t n)
{
    for (int dir : {FWD, INV}) {
        const KernelLaunch k = real_launch(n, dir);
        if (!k.kernel) return hipErrorInvalidValue;
        if (hipError_t e = raise_lds_limit(k); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_real(int dir, uint32_t n, float *real, float *spec, uint64_t batch, float scale, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const KernelLaunch k = real_launch(n, dir);
    if (!k.kernel) return hipErrorInvalidValue;
    if (batch > (~0ull) / (4ull * (n + 2))) return hipErrorInvalidValue;
    const Geometry g = geometry(n);
    const uint64_t grid = blocks(g, batch);
    if (g.small) {
        if (hipError_t e = check_grid(grid); e != hipSuccess) return e;
        void *args[] = {&real, &spec, &batch, &scale};
        return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
    }
    uint32_t xcd_swizzle = 1;
    if (hipError_t e = check_grid(grid, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&real, &spec, &batch, &scale, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)grid), dim3(k.threads), args, k.lds, st);
}

}  // namespace fwr
