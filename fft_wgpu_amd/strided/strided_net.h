// strided_net.h -- the register networks of the 64 .. 4096-point transforms that keep P points per thread (device code,
// gfx950 only): the compile-time twiddle table, one Stockham stage on a thread's points and the exchange between two stages.
// Shared by k_strided (kernels_strided.hip: the columns of a matrix) and k_rows2d (../fft2d/kernels_fft2d.hip: its rows);
// the two differ in which lanes hold which line and in the LDS word of an element, which the caller hands to exchange<>.
//
// Thread t of a line holds the P elements t + T*m (T = N / P threads per line) before AND after every stage: a Stockham stage
// of radix R with sub-block size J reads x[idx + m*N/R], idx = t + T*g (g < P/R) -- thread t's own points g + m*P/R -- and
// writes output q of butterfly idx to element (idx - j)*R + j + q*J, j = idx mod J, times W_N^{(idx - j) q}.  Between two
// stages the points change threads through LDS, plane-wise (real parts, then imaginary parts); after the last stage element
// t + T*m is back in thread t's register m.
// Twiddles: W_4096^k, k < 2048, evaluated in double at compile time and rounded to f32 once (cplx.h: cx_cos2pi); W_N^e is
// entry e * 4096 / N, negated for the upper half.  The inverse conjugates on use.  No sinf / cosf runs on the device.
#pragma once
#include "../csrc/device_common.h"

namespace fws {

using namespace fwa;

struct TwTable {
    float v[4096];  // {re, im} of W_4096^k = exp(-2 pi i k / 4096), k < 2048
};
constexpr TwTable make_tw_table()
{
    TwTable t{};
    for (int k = 0; k < 2048; ++k) {
        t.v[2 * k] = (float)cx_cos2pi(k, 4096);
        t.v[2 * k + 1] = (float)-cx_sin2pi(k, 4096);
    }
    return t;
}
__device__ const TwTable g_tw alignas(16) = make_tw_table();

template <int N>
__device__ __forceinline__ v2f tw_n(uint32_t e)  // W_N^e, 0 <= e < N
{
    const uint32_t i = e * (4096 / N);
    const v2f w = reinterpret_cast<const v2f *>(g_tw.v)[i & 2047u];
    return (i & 2048u) ? -w : w;
}

// Stage of radix R with sub-block size J on the P points of thread t.  Output q of butterfly g is left in x[g + q*P/R]; it
// is element dest<..>(t, g) + q*J of the line (exchange below), or, after the last stage, element t + T*(g + q*P/R).
template <int N, int P, int R, int J, int DIR>
__device__ __forceinline__ void stage(v2f (&x)[P], uint32_t t)
{
    constexpr int G = P / R, T = N / P;
    static_for<0, G>([&](auto g_) {
        constexpr int g = decltype(g_)::value;
        v2f v[R];
        static_for<0, R>([&](auto m_) { constexpr int m = decltype(m_)::value; v[m] = x[g + m * G]; });
        fft_reg<R, DIR>(v);
        const uint32_t idx = t + T * g;
        const uint32_t sJ = idx & ~(uint32_t)(J - 1);
        static_for<0, R>([&](auto q_) {
            constexpr int q = decltype(q_)::value;
            v2f y = v[brev<R>(q)];
            if constexpr (q != 0 && J * R < N) y = cmul_tw<DIR>(y, tw_n<N>(sJ * q));
            x[g + q * G] = y;
        });
    });
}

// The points of a stage<N, P, R, J> go to the threads of the next stage: plane-wise through xch; word(d) is the LDS word of
// element d of this thread's line.
template <int N, int P, int R, int J, bool FIRST, class Word>
__device__ __forceinline__ void exchange(v2f (&x)[P], float *xch, uint32_t t, Word word)
{
    constexpr int G = P / R, T = N / P;
    auto dest = [&](int g, int q) {
        const uint32_t idx = t + T * g, j = idx & (uint32_t)(J - 1);
        return (idx - j) * R + j + q * J;
    };
    if constexpr (!FIRST) __syncthreads();  // the reads of the exchange before this one
    static_for<0, G>([&](auto g_) {
        static_for<0, R>([&](auto q_) {
            constexpr int g = decltype(g_)::value, q = decltype(q_)::value;
            xch[word(dest(g, q))] = x[g + q * G].x;
        });
    });
    __syncthreads();
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m].x = xch[word(t + T * m)]; });
    __syncthreads();
    static_for<0, G>([&](auto g_) {
        static_for<0, R>([&](auto q_) {
            constexpr int g = decltype(g_)::value, q = decltype(q_)::value;
            xch[word(dest(g, q))] = x[g + q * G].y;
        });
    });
    __syncthreads();
    static_for<0, P>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m].y = xch[word(t + T * m)]; });
}

}  // namespace fws
