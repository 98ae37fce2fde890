// small32_kernel.h -- k_small32 (one-launch kernels for n = 512 .. 32768) as a template shared by its two translation
// units (kernels_small32.hip: 512 .. 4096 + the launcher; kernels_small32b.hip: 8192 .. 32768).
#pragma once
#include "small32_common.h"

namespace fwa {

// ---------------------------------------------------------------------------
// (Below 512 the same structure loses badly -- n/32 = 2 .. 8 threads per transform make every load instruction a
// 16..64-byte-per-transform gather: 0.09 / 0.17 / 0.54 of the roofline at 64 / 128 / 256 against 0.70 for k_small16,
// profiles/round2/sweep_small32_below_512.jsonl -- so k_small16 keeps n <= 256.)
// n = 512 .. 32768: 32 points per thread, register stages 32 x 16 | 32 x 32 | 32 x 32 x 2 | 32 x 32 x 4 | 32 x 32 x 8 |
// 32 x 32 x 16 | 32 x 32 x 32, i.e. ONE exchange at 512 / 1024 and TWO above (k_small16: two / three), each through a
// float buffer -- real parts, then imaginary parts.  n/32 threads per transform, 256-thread workgroups (512 / 1024 at
// 16384 / 32768) with 33 KiB of LDS (66 / 132 KiB): 256 KiB of loads in flight per CU (k_small16 at 8192 / 16384:
// 128 KiB; measured 0.37 / 0.40 -> 0.63 / 0.66 of the roofline).  The network itself (geometry, exchanges, stages) is Net32
// and its helpers in small32_common.h; here: per-transform SRD, one role (transform xf, butterfly t), linear store.
// ---------------------------------------------------------------------------
// The body for workgroup index `blk` (k_small32: blk = blockIdx.x; tools/archive/small32_persist_probe.hip walks it through a
// persistent loop, measured no faster: profiles/round3/probe_small32_persistent_negative.txt).
// PREFETCH: where the twiddle-table look-ups are issued.  At the point of use (0) each costs its wave an exposed cache
// latency between the last data load landing and the exchange; they depend on the thread index only, so they can go out
// BEFORE the data loads (bit 0: the twiddles of stage 0, bit 1: those of stage 1 of the three-stage sizes) or right BEHIND
// them, before the wait for the data (bits 2, 3).  Per size, at the 32-GiB footprint, interleaved, bit-identical results
// (tools/archive/small32_prefetch_probe.hip).  With the plain block -> chunk map (profiles/round5/probe_small32_twiddle_prefetch.jsonl):
// 2^10 0.775 -> 0.790, 2^11 0.740 -> 0.790, 2^12 0.705 -> 0.738, 2^13 0.717 -> 0.739.  With the pair map of one_launch_block
// (device_common.h), which came later and lifts the point-of-use form by more (probe_small32_twiddle_prefetch_pair_map.jsonl):
// 2^10 0.807 -> 0.814 (behind), 2^11 0.806 -> 0.807 (both stages, before), 2^12 0.774 -> 0.778 (behind) -- kept -- and 2^13
// 0.787 -> 0.758: back at the point of use, as 2^14 / 2^15 (spills from stage 1 on, or a worse schedule: - 1 ... - 9 %).
constexpr int small32_prefetch_default(int lgn) { return lgn == 11 ? 3 : (lgn == 10 || lgn == 12) ? 4 : 0; }

template <int LGN, int DIR, int PREFETCH = small32_prefetch_default(LGN)>
__device__ __forceinline__ void small32_body(const v2f *__restrict__ src, v2f *__restrict__ dst, const v2f *__restrict__ tw,
                                             uint64_t batch, float scale, uint64_t blk, uint32_t tid)
{
    static_assert(LGN >= 9 && LGN <= 15, "k_small32 covers n = 512 .. 32768");
    using G = Net32<LGN>;
    constexpr int N = G::N, T = G::T;
    constexpr int WG = LGN <= 13 ? 256 : T;                     // workgroup size; XPW transforms per workgroup
    constexpr int XPW = WG / T;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t xf = tid / T, t = tid % T;
    float *lf = reinterpret_cast<float *>(smem) + xf * G::PN;
    // buffer (SRD) addressing: one per-lane offset, the per-access part is a scalar (no address VGPR per access); the
    // descriptor ends with the last valid transform of the batch, so surplus lanes of a ragged last workgroup read
    // zeros and their stores are dropped
    const uint64_t first = blk * XPW;
    const uint64_t left = batch - first;
    const uint32_t valid_bytes = (uint32_t)(left < (uint64_t)XPW ? left : (uint64_t)XPW) * (N * 8u);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<v2f *>(src + first * N), 0, valid_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(dst + first * N, 0, valid_bytes, 0x00020000);
    const uint32_t voff = (xf * N + t) * 8;

    const uint32_t t_hi = t >> 5, t_lo = t & 31;
    const uint32_t rbase = t + t_hi;  // P(t): every read position is element t plus a constant

    Twiddles<32, N> w0;
    Stage1Twiddles<LGN> w1;
    if constexpr (PREFETCH & 1) twiddle_fetch<32, N>(w0, tw, t);
    if constexpr (!G::TWO && (PREFETCH & 2)) stage1_fetch<LGN>(w1, tw, t);
    v2f x[32];
    static_for<0, 32>([&](auto m_) { constexpr int m = decltype(m_)::value; x[m] = buf_load<AUX_NT>(rin, voff, m * T * 8); });
    if constexpr (PREFETCH & 4) twiddle_fetch<32, N>(w0, tw, t);   // behind the data loads, before the wait for them
    if constexpr (!G::TWO && (PREFETCH & 8)) stage1_fetch<LGN>(w1, tw, t);
    fft_reg<32, DIR>(x);
    if constexpr (PREFETCH & 5) twiddle_apply<32, N, DIR>(x, w0);
    else twiddle_outputs<32, N, DIR>(x, tw, t);
    // -> stage 1, or the last stage (radix R1, J = 32): lane bases 33*t to write, P(t) to read (Net32)
    exchange32<G::ex1_w, G::ex1_r>(x, lf, 33 * t, lf, rbase);
    if constexpr (!G::TWO) {
        stage1<LGN, DIR, (PREFETCH & 10) != 0>(x, w1, tw, t);
        __syncthreads();  // every read of the first exchange is done before its buffer is rewritten
        exchange32<G::ex2_w, G::ex2_r>(x, lf, (t - t_lo) * G::R1 + t_lo + t_hi * G::R1, lf, rbase);
    }
    // last stage: output q of butterfly idx = t + b*T at idx + q*JL
    last_stage<G::RL, DIR>(x, [&](auto b_, auto q_, const v2f &v) {
        buf_store<AUX_NT>(v * scale, rout, voff, (decltype(b_)::value * T + decltype(q_)::value * G::JL) * 8);
    });
}

template <int LGN, int DIR, int PREFETCH = small32_prefetch_default(LGN)>
__global__ __launch_bounds__((LGN <= 13 ? 256 : (1 << (LGN - 5))), 4) void k_small32(const v2f *__restrict__ src,
                                                                                    v2f *__restrict__ dst,
                                                                                    const v2f *__restrict__ tw,
                                                                                    uint64_t batch, float scale)
{
    small32_body<LGN, DIR, PREFETCH>(src, dst, tw, batch, scale, one_launch_block(), threadIdx.x);
}

constexpr uint32_t small32_xpw(uint32_t lg_n) { return lg_n <= 13 ? 256u / (1u << (lg_n - 5)) : 1u; }  // lg_n >= 6
constexpr size_t small32_lds(uint32_t lg_n)
{
    return (size_t)small32_xpw(lg_n) * pad32(1u << lg_n) * sizeof(float);
}
// n = 2^LGN; 8192 .. 32768 are instantiated in kernels_small32b.hip, a translation unit of its own so that the library builds
// in parallel
template <int LGN>
hipError_t launch_small32_n(int dir, const v2f *src, v2f *dst, const v2f *tw, uint64_t batch, float scale, hipStream_t st)
{
    constexpr uint32_t xpw = small32_xpw(LGN);
    const uint64_t blocks = (batch + xpw - 1) / xpw;
    if (hipError_t e = check_grid(blocks); e != hipSuccess) return e;
    const dim3 g((uint32_t)blocks), b(LGN <= 13 ? 256 : (1 << (LGN - 5)));
    if (dir == FWD) hipLaunchKernelGGL((k_small32<LGN, FWD>), g, b, small32_lds(LGN), st, src, dst, tw, batch, scale);
    else hipLaunchKernelGGL((k_small32<LGN, INV>), g, b, small32_lds(LGN), st, src, dst, tw, batch, scale);
    return hipGetLastError();
}
extern template hipError_t launch_small32_n<13>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);
extern template hipError_t launch_small32_n<14>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);
extern template hipError_t launch_small32_n<15>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);

}  // namespace fwa
