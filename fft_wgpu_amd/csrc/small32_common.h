// small32_common.h -- the 32-point-per-thread network, written once: geometry and exchange offset maps (Net32), the in-place
// exchange, the stage-1 and last-stage butterflies, and the twiddle helper.  Included through small32_kernel.h by
// kernels_small32{,b}.hip (k_small32) and through rows32.h by kernels_rows32{,b,c}.hip (k_rows32) and kernels_cols32.hip
// (k_cols32, k_colsw); a kernel adds its addressing, the role of a lane when it writes and reads, and its store.
#pragma once
#include "device_common.h"

namespace fwa {

// Positions in an exchange buffer are padded by one float per 32 (conflict-free b32 accesses).
constexpr uint32_t pad32(uint32_t p) { return p + p / 32; }

// n = 2^LGN as radix 32 | exchange | radix R1, and above 1024 | second exchange | radix R2; butterfly t = 0 .. T-1 of a
// stage is one lane.  Same Stockham recurrence per stage, radix R: idx = s*J + j, inputs idx + m*n/R, output q at
// s*R*J + j + q*J times W_n^{s*J*q}.  The ex*_w / ex*_r maps give, for register i of a lane, the compile-time part of the
// position it is written to / refilled from.  The lane's part stays in the kernels, with the role a lane has there: 33*t
// to write the first exchange, P(t) = t + (t >> 5) to read either, (t - t_lo)*R1 + t_lo + t_hi*R1 (t_hi = t >> 5,
// t_lo = t & 31) to write the second.  (As helper functions of t these come out of the optimiser in another canonical form
// and k_small32 / k_rows32 get another instruction order; nobody has measured that one.)
template <int LGN>
struct Net32 {
    static constexpr int N = 1 << LGN;
    static constexpr int T = N / 32;                        // lanes per transform = radix-32 butterflies
    static constexpr int R1 = LGN < 10 ? N / 32 : 32;       // second radix
    static constexpr bool TWO = (32 * R1 == N);             // n <= 1024: two stages, one exchange
    static constexpr int R2 = TWO ? 1 : N / (32 * R1);      // third radix: 2, 4, 8, 16, 32 for 2^11 .. 2^15
    static constexpr int B1 = 32 / R1, B2 = 32 / R2;        // butterflies per lane in stage 1 / stage 2
    static constexpr int J2 = 32 * R1;
    static constexpr int RL = TWO ? R1 : R2, JL = TWO ? 32 : J2;  // the last stage: output q of butterfly idx at idx + q*JL
    static constexpr int PN = pad32(N);                     // padded floats per transform

    // stage 0 (radix 32, J = 1, s = t) leaves output q in x[brev(q)]; it goes to position t*32 + q (padded: 33*t + q)
    static constexpr uint32_t ex1_w(int i) { return brev<32>(i); }
    // -> stage 1 (radix R1, J = 32): butterfly b of lane t is idx = t + b*T, input m at idx + m*N/R1
    static constexpr uint32_t ex1_r(int i) { return pad32((i / R1) * T + (i % R1) * (N / R1)); }
    // Output q of stage-1 butterfly b sits at sJ*R1 + j + q*32 with sJ = (t & ~31) + b*T, j = t & 31 (T is a multiple of
    // 32 here): lane part (t & ~31)*R1 + (t & 31), padded by (t >> 5)*R1; constant part b*T*R1 + q*32
    static constexpr uint32_t ex2_w(int i) { return pad32((i / R1) * T * R1 + brev<R1>(i % R1) * 32); }
    // -> stage 2 (radix R2, J = N/R2, s = 0): butterfly b is idx = t + b*T < N/R2, input m at idx + m*N/R2
    static constexpr uint32_t ex2_r(int i) { return pad32((i / R2) * T + (i % R2) * (N / R2)); }
};

// In-place exchange: register i deposits its value at wp[wbase + WOFF(i)] and is refilled from rp[rbase + ROFF(i)]; real
// parts first (x[i].y still holds the old imaginary part meanwhile), then imaginary parts.  Every position is a
// lane-dependent base plus a compile-time offset: for the padding P(p) = p + p/32, P(a + b) = P(a) + P(b) whenever b
// is a multiple of 32 or a + (b mod 32) < 32 -- so each access is one ds instruction with an immediate offset.
// Buffers and lane bases (and t of stage1 below) come by reference, as the closures this replaces captured them: by value
// the base arithmetic is folded into the addresses before it is reassociated, and k_small32<15> gets longer address chains.
template <uint32_t (*WOFF)(int), uint32_t (*ROFF)(int)>
__device__ __forceinline__ void exchange32(v2f (&x)[32], float *const &wp, const uint32_t &wbase, const float *const &rp,
                                           const uint32_t &rbase)
{
    static_for<0, 32>([&](auto i_) { constexpr int i = decltype(i_)::value; wp[wbase + WOFF(i)] = x[i].x; });
    __syncthreads();
    static_for<0, 32>([&](auto i_) { constexpr int i = decltype(i_)::value; x[i].x = rp[rbase + ROFF(i)]; });
    __syncthreads();
    static_for<0, 32>([&](auto i_) { constexpr int i = decltype(i_)::value; wp[wbase + WOFF(i)] = x[i].y; });
    __syncthreads();
    static_for<0, 32>([&](auto i_) { constexpr int i = decltype(i_)::value; x[i].y = rp[rbase + ROFF(i)]; });
}

// x[brev<R>(q)] *= W_N^{e*q} for q = 1 .. R-1 with 7 + R/8 - 1 table look-ups instead of R - 1:
// W^{e(8a + b)} = W^{8ea} * W^{eb} (one extra rounding on the twiddles that are products, as in k_tile).
// In two halves so that a kernel can issue the look-ups long before it needs them (they depend on the thread index only):
// issued at the point of use, behind the data loads, each costs its wave an exposed cache latency.
template <int R, int N>
struct Twiddles {
    v2f pb[8], pa[R / 8];
};
template <int R, int N>
__device__ __forceinline__ void twiddle_fetch(Twiddles<R, N> &w, const v2f *__restrict__ tw, uint32_t e)
{
    static_assert(R == 16 || R == 32, "radix");
    static_for<1, 8>([&](auto b_) { constexpr int b = decltype(b_)::value; w.pb[b] = tw_lookup<N>(tw, e * b); });
    static_for<1, R / 8>([&](auto a_) { constexpr int a = decltype(a_)::value; w.pa[a] = tw_lookup<N>(tw, e * (8 * a)); });
}
template <int R, int N, int DIR>
__device__ __forceinline__ void twiddle_apply(v2f (&x)[R], const Twiddles<R, N> &w)
{
    static_for<1, R>([&](auto q_) {
        constexpr int q = decltype(q_)::value;
        constexpr int a = q / 8, b = q % 8, r = brev<R>(q);
        if constexpr (a == 0) x[r] = cmul_tw<DIR>(x[r], w.pb[b]);
        else if constexpr (b == 0) x[r] = cmul_tw<DIR>(x[r], w.pa[a]);
        else x[r] = cmul_tw<DIR>(x[r], cmul(w.pa[a], w.pb[b]));
    });
}
template <int R, int N, int DIR>
__device__ __forceinline__ void twiddle_outputs(v2f (&x)[R], const v2f *__restrict__ tw, uint32_t e)
{
    Twiddles<R, N> w;
    twiddle_fetch<R, N>(w, tw, e);
    twiddle_apply<R, N, DIR>(x, w);
}

// Stage 1 of the three-stage sizes: the B1 radix-R1 butterflies of lane t (butterfly b is idx = t + b*T) and their
// twiddles W_N^{sJ*q}, sJ = idx & ~31 (output q: position sJ*R1 + j + q*32); the look-ups prefetched by stage1_fetch
// (PREFETCHED) or made at the point of use (w1 is not read then).  k_cols32 (B1 = 1) spells its stage 1 out.
template <int LGN>
using Stage1Twiddles = Twiddles<Net32<LGN>::R1, Net32<LGN>::N>[Net32<LGN>::B1];
template <int LGN>
__device__ __forceinline__ void stage1_fetch(Stage1Twiddles<LGN> &w1, const v2f *tw, const uint32_t &t)
{
    using G = Net32<LGN>;
    static_for<0, G::B1>([&](auto b_) { constexpr int b = decltype(b_)::value; twiddle_fetch<G::R1, G::N>(w1[b], tw, (t + b * G::T) & ~31u); });
}
template <int LGN, int DIR, bool PREFETCHED>
__device__ __forceinline__ void stage1(v2f (&x)[32], const Stage1Twiddles<LGN> &w1, const v2f *tw, const uint32_t &t)
{
    using G = Net32<LGN>;
    static_for<0, G::B1>([&](auto b_) {
        constexpr int b = decltype(b_)::value;
        v2f(&z)[G::R1] = *reinterpret_cast<v2f(*)[G::R1]>(&x[b * G::R1]);
        fft_reg<G::R1, DIR>(z);
        if constexpr (PREFETCHED) twiddle_apply<G::R1, G::N, DIR>(z, w1[b]);
        else twiddle_outputs<G::R1, G::N, DIR>(z, tw, (t + b * G::T) & ~31u);
    });
}

// Last stage (s = 0: no twiddle): the 32/R radix-R butterflies of a lane; output q of butterfly b is handed to
// store(b_, q_, value) with b and q as compile-time constants.  It belongs at idx + q*JL, idx = lane + b*T.
template <int R, int DIR, class Store>
__device__ __forceinline__ void last_stage(v2f (&x)[32], Store store)
{
    static_for<0, 32 / R>([&](auto b_) {
        constexpr int b = decltype(b_)::value;
        v2f(&z)[R] = *reinterpret_cast<v2f(*)[R]>(&x[b * R]);
        fft_reg<R, DIR>(z);
        static_for<0, R>([&](auto q_) { store(b_, q_, z[brev<R>(decltype(q_)::value)]); });
    });
}

}  // namespace fwa
