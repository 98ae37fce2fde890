// kernels_strided.hip -- the strided-batch (column) plans: every column of a row-major n x howmany matrix is its own DFT
// over the rows, in place, one pass over memory.  gfx950 only.  Geometry and the reasons for it: strided_geom.h.
//
// One workgroup owns a tile of W adjacent columns by all n rows: lane = column + W * t, so every load / store instruction of
// a wave moves whole W*8-byte row segments.  Thread t of a column holds the P rows t + T*m (T = n / P threads per column)
// before AND after every stage: a Stockham stage of radix R with sub-block size J reads x[idx + m*n/R], idx = t + T*g
// (g < P/R) -- thread t's own points g + m*P/R -- and writes output q of butterfly idx to element (idx - j)*R + j + q*J,
// j = idx mod J, times W_n^{(idx - j) q}.  Between two stages the points change threads through LDS, plane-wise (real
// parts, then imaginary parts: n * W floats); after the last stage element t + T*m is back in thread t's register m, so
// the result leaves in natural order through the same addresses the input came in by.
// LDS word of element d of column c: W * (d ^ ((d >> log2 r0) & 3)) + c.  The first stage writes elements r0 apart from
// adjacent threads (a bank-aligned stride); the XOR moves them to different rows mod 4, later stages and every read touch
// adjacent elements from adjacent threads: no access has a bank conflict at W = 16 (two threads per 32-lane group) or at
// W = 8 (four).
// Twiddles: W_4096^k, k < 2048, evaluated in double at compile time and rounded to f32 once (cplx.h: cx_cos2pi); W_n^e is
// entry e * 4096 / n, negated for the upper half.  The inverse conjugates on use.  No sinf / cosf runs on the device.
// howmany is any positive integer: rows are then only 8-byte aligned, so every sample moves as one 8-byte access, and the
// lanes of the last tile past `howmany` neither load nor store.  Matrices of at most 2 GiB go through one buffer descriptor
// with 32-bit offsets (BIG = false); larger ones through 64-bit pointers (BIG = true).  The matrix base is 64-bit in both.
#include "../csrc/device_common.h"
#include "strided_kernels.h"
#include "strided_net.h"

namespace fws {

using namespace fwa;

// The rows row0 + i * row_step of one column of one matrix.  The caller masks: a lane whose column does not exist calls
// neither load nor store.
template <bool BIG>
struct Rows;
template <>
struct Rows<false> {  // the whole matrix is at most 2^31 bytes: offsets of existing samples fit 32 bits
    __amdgpu_buffer_rsrc_t r;
    uint32_t voff, rstep;
    __device__ __forceinline__ Rows(v2f *matrix, uint32_t n, uint64_t howmany, uint32_t row0, uint32_t row_step, uint64_t col)
        : r(__builtin_amdgcn_make_buffer_rsrc(matrix, 0, (uint32_t)(n * howmany * 8), 0x00020000)),
          voff((uint32_t)((row0 * howmany + col) * 8)), rstep((uint32_t)(row_step * howmany * 8))
    {
    }
    __device__ __forceinline__ v2f load(uint32_t i) const { return buf_load<AUX_NT>(r, voff, i * rstep); }
    __device__ __forceinline__ void store(uint32_t i, v2f v) const { buf_store<AUX_NT>(v, r, voff, i * rstep); }
};
template <>
struct Rows<true> {
    v2f *p;
    uint64_t rstep;  // elements
    __device__ __forceinline__ Rows(v2f *matrix, uint32_t, uint64_t howmany, uint32_t row0, uint32_t row_step, uint64_t col)
        : p(matrix + (row0 * howmany + col)), rstep(row_step * howmany)
    {
    }
    __device__ __forceinline__ v2f load(uint32_t i) const { return __builtin_nontemporal_load(p + i * rstep); }
    __device__ __forceinline__ void store(uint32_t i, v2f v) const { __builtin_nontemporal_store(v, p + i * rstep); }
};

// ---------------------------------------------------------------------------
// n <= 32: one thread, one column, no exchange; 32 / n steps of 256 adjacent columns per workgroup.
// ---------------------------------------------------------------------------
template <int LGN, int DIR, bool BIG>
__global__ __launch_bounds__(SMALL_THREADS) void k_strided_small(v2f *buf, uint64_t howmany, uint32_t wgs, float scale,
                                                                 uint32_t xcd_swizzle)
{
    constexpr int N = 1 << LGN, STEPS = (int)SMALL_MAX / N;
    const uint32_t bid = xcd_map(xcd_swizzle);
    const uint32_t wg = bid % wgs;
    const uint64_t mat = bid / wgs;
    v2f *matrix = buf + mat * N * howmany;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        const uint64_t col = ((uint64_t)wg * STEPS + i) * SMALL_THREADS + threadIdx.x;
        const Rows<BIG> rows(matrix, N, howmany, 0, 1, col);
        if (col < howmany) {
            v2f x[N];
            static_for<0, N>([&](auto j_) { constexpr int j = decltype(j_)::value; x[j] = rows.load(j); });
            fft_reg<N, DIR>(x);
            static_for<0, N>([&](auto k_) { constexpr int k = decltype(k_)::value; rows.store(k, x[brev<N>(k)] * scale); });
        }
    }
}

// ---------------------------------------------------------------------------
// n >= 64: W columns per workgroup, P points per thread, two or three stages.
// ---------------------------------------------------------------------------
// (the stages and the exchange between them: strided_net.h)
template <int LGN, int DIR, bool BIG>
__global__ __launch_bounds__(geometry(1u << LGN).threads) void k_strided(v2f *buf, uint64_t howmany, uint32_t tiles,
                                                                         float scale, uint32_t xcd_swizzle)
{
    constexpr int N = 1 << LGN;
    constexpr Net K = net_of(LGN);
    constexpr int P = K.points, T = N / P, W = K.tile_cols, LGW = ilog2c(W), LGR0 = ilog2c(K.r0);
    static_assert(K.r0 * K.r1 * K.r2 == N && P % K.r0 == 0 && P % K.r1 == 0 && P % K.r2 == 0, "the stages cover n");
    static_assert(T % 4 == 0 && K.r0 >= 4 && T * W == geometry(N).threads && N * W * 4 == geometry(N).lds_bytes, "geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xch = reinterpret_cast<float *>(smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t c = tid & (W - 1), t = tid >> LGW;
    const uint32_t bid = xcd_map(xcd_swizzle);
    const uint32_t tile = bid % tiles;
    const uint64_t mat = bid / tiles;
    const uint64_t col = (uint64_t)tile * W + c;
    const bool live = col < howmany;  // the last tile of a row of tiles is partial
    const Rows<BIG> rows(buf + mat * N * howmany, N, howmany, t, T, col);

    v2f x[P];
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = v2f{0.0f, 0.0f}; });
    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = rows.load(m); });

    stage<N, P, K.r0, 1, DIR>(x, t);
    auto word = [c](uint32_t d) { return (d ^ ((d >> LGR0) & 3u)) * W + c; };
    exchange<N, P, K.r0, 1, true>(x, xch, t, word);
    stage<N, P, K.r1, K.r0, DIR>(x, t);
    if constexpr (K.r2 > 1) {
        exchange<N, P, K.r1, K.r0, false>(x, xch, t, word);
        stage<N, P, K.r2, K.r0 * K.r1, DIR>(x, t);
    }

    if (live) static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; rows.store(m, x[m] * scale); });
}

// ---- launch ---------------------------------------------------------------------------------------------------------
template <int LGN, int DIR, bool BIG>
static const void *kernel_of()
{
    if constexpr ((1u << LGN) <= SMALL_MAX) return reinterpret_cast<const void *>(&k_strided_small<LGN, DIR, BIG>);
    else return reinterpret_cast<const void *>(&k_strided<LGN, DIR, BIG>);
}
template <int LGN>
static const void *kernel_of_lg(int dir, bool big)
{
    if (dir == FWD) return big ? kernel_of<LGN, FWD, true>() : kernel_of<LGN, FWD, false>();
    return big ? kernel_of<LGN, INV, true>() : kernel_of<LGN, INV, false>();
}
static KernelLaunch strided_launch(uint32_t n, int dir, bool big)
{
    const void *k = nullptr;
    switch (n) {
        case 2: k = kernel_of_lg<1>(dir, big); break;
        case 4: k = kernel_of_lg<2>(dir, big); break;
        case 8: k = kernel_of_lg<3>(dir, big); break;
        case 16: k = kernel_of_lg<4>(dir, big); break;
        case 32: k = kernel_of_lg<5>(dir, big); break;
        case 64: k = kernel_of_lg<6>(dir, big); break;
        case 128: k = kernel_of_lg<7>(dir, big); break;
        case 256: k = kernel_of_lg<8>(dir, big); break;
        case 512: k = kernel_of_lg<9>(dir, big); break;
        case 1024: k = kernel_of_lg<10>(dir, big); break;
        case 2048: k = kernel_of_lg<11>(dir, big); break;
        case 4096: k = kernel_of_lg<12>(dir, big); break;
        default: return {};
    }
    const Geometry g = geometry(n);
    return {k, (uint32_t)g.threads, g.lds_bytes};
}

hipError_t setup_strided_kernels(uint32_t n)
{
    for (int dir : {FWD, INV})
        for (bool big : {false, true}) {
            const KernelLaunch k = strided_launch(n, dir, big);
            if (!k.kernel) return hipErrorInvalidValue;
            if (hipError_t e = raise_lds_limit(k); e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t launch_strided(int dir, uint32_t n, v2f *buf, uint64_t howmany, uint64_t batch, float scale, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    if (howmany == 0 || howmany > (~0ull) / (8ull * MAX_LEN)) return hipErrorInvalidValue;
    const bool big = (uint64_t)n * howmany * 8 > (1ull << 31);
    const KernelLaunch k = strided_launch(n, dir, big);
    if (!k.kernel) return hipErrorInvalidValue;
    const uint64_t wgs = wgs_per_matrix(geometry(n), howmany);
    if (batch > 0x7fffffffull / wgs) return hipErrorInvalidValue;
    const uint64_t blocks = batch * wgs;
    uint32_t xcd_swizzle = 1, per_matrix = (uint32_t)wgs;
    if (hipError_t e = check_grid(blocks, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&buf, &howmany, &per_matrix, &scale, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
}

}  // namespace fws
