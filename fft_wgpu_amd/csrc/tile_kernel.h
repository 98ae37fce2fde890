// tile_kernel.h -- k_tile, the generic 16-point-per-thread tile kernel of the multi-pass paths, as a template shared by its two
// translation units (kernels_tiled.hip: launcher + forward; kernels_tiled_inv.hip: inverse).
#pragma once
#include "tile_body.h"

namespace fwa {

template <int LGL, int CW, int DIR, int MODE, bool BUF, int ROLE>
__global__ __launch_bounds__(((1 << LGL) / 16) * CW) void k_tile(TileArgs a)
{
    constexpr int AOUT = (ROLE == ROLE_FIRST || ROLE == ROLE_MIDDLE) ? AUX_SC1 : (ROLE == ROLE_LAST ? AUX_NT : AUX_DEFAULT);
    constexpr int AIN = (ROLE == ROLE_FIRST) ? AUX_NT : AUX_DEFAULT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // XCD-aware block -> tile mapping, bit 0 only: each XCD gets a contiguous run of tiles (xcd_map, device_common.h).  Bit 2
    // (adjacent tiles for the two residents of a CU) means nothing for these small workgroups and is ignored, as the
    // header's description of "xcd_swizzle" says: values without bit 0 leave every kernel of the plan unswizzled.
    const uint32_t bid = xcd_map(a.xcd_swizzle & 1u);
    const uint32_t tile = bid % a.tile_count;
    const uint32_t rest = bid / a.tile_count;
    const uint32_t d1 = rest % a.d1_count;
    const uint64_t b = rest / a.d1_count;
    const v2f *in = a.in + b * a.in_sb + d1 * a.in_s1 + tile * a.in_st;
    v2f *out = a.out + b * a.out_sb + d1 * a.out_s1 + tile * a.out_st;
    tile_body<LGL, CW, DIR, MODE, BUF, AIN, AOUT>(in, out, tile * CW, a.tw, a.tw_lo, a.tw_hi, a.pitch, a.out_stride, a.scale,
                                                   reinterpret_cast<v2f *>(smem), threadIdx.x);
}

// k_tile of one direction by mode, length, buffer form and role: COLS passes come as first or middle pass, ROWS_T is always
// the last; the 64-bit-pointer form (BUF = false, only above 4-GiB tiles) has no policy bits.  The inverse direction is
// instantiated in kernels_tiled_inv.hip, a translation unit of its own so that the library builds in parallel.
template <int DIR>
const void *tile_kernel(int mode, uint32_t lg_l, bool buf, int role)
{
    auto of = [lg_l](auto mode_, auto buf_, auto role_) -> const void * {
        constexpr int M = decltype(mode_)::value, R = decltype(role_)::value;
        constexpr bool B = decltype(buf_)::value;
        switch (lg_l) {
            case 6: return reinterpret_cast<const void *>(&k_tile<6, TILE_CW, DIR, M, B, R>);
            case 7: return reinterpret_cast<const void *>(&k_tile<7, TILE_CW, DIR, M, B, R>);
            case 8: return reinterpret_cast<const void *>(&k_tile<8, TILE_CW, DIR, M, B, R>);
            case 9: return reinterpret_cast<const void *>(&k_tile<9, TILE_CW, DIR, M, B, R>);
            case 10: return reinterpret_cast<const void *>(&k_tile<10, TILE_CW, DIR, M, B, R>);
            default: return nullptr;
        }
    };
    using COLS = std::integral_constant<int, TILE_COLS>;
    using ROWS_T = std::integral_constant<int, TILE_ROWS_T>;
    using NO_ROLE = std::integral_constant<int, 0>;
    if (!buf) return mode == TILE_COLS ? of(COLS{}, std::false_type{}, NO_ROLE{}) : of(ROWS_T{}, std::false_type{}, NO_ROLE{});
    if (mode != TILE_COLS) return of(ROWS_T{}, std::true_type{}, std::integral_constant<int, ROLE_LAST>{});
    return role == ROLE_MIDDLE ? of(COLS{}, std::true_type{}, std::integral_constant<int, ROLE_MIDDLE>{})
                               : of(COLS{}, std::true_type{}, std::integral_constant<int, ROLE_FIRST>{});
}
extern template const void *tile_kernel<INV>(int mode, uint32_t lg_l, bool buf, int role);

}  // namespace fwa
