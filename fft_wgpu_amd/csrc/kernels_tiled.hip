// kernels_tiled.hip -- the building block of the 2- and 3-pass paths: k_tile (template: tile_kernel.h); launcher and the
// forward instantiations (inverse: kernels_tiled_inv.hip).
#include "tile_kernel.h"

namespace fwa {

// kernel = nullptr: no such length
static KernelLaunch tile_launch(int dir, int mode, uint32_t lg_l, bool buf, int role)
{
    if (!tile_supported(lg_l)) return {};
    return {dir == FWD ? tile_kernel<FWD>(mode, lg_l, buf, role) : tile_kernel<INV>(mode, lg_l, buf, role),
            (1u << lg_l) / 16 * TILE_CW, (int)tile_lds(lg_l, TILE_CW)};
}

hipError_t setup_tile_kernels()
{
    hipError_t e = hipSuccess;
    for (uint32_t lg_l = 6; lg_l <= 10; ++lg_l)
        for (int dir : {FWD, INV})
            for (int mode : {TILE_COLS, TILE_ROWS_T})
                for (bool buf : {false, true})
                    for (int role : {ROLE_FIRST, ROLE_MIDDLE})
                        if (e == hipSuccess) e = raise_lds_limit(tile_launch(dir, mode, lg_l, buf, role));
    return e;
}

hipError_t launch_tile(int dir, int mode, uint32_t lg_l, const TileArgs &a, uint64_t batch, hipStream_t st)
{
    const uint64_t blocks = batch * a.d1_count * a.tile_count;
    if (blocks == 0) return hipSuccess;
    TileArgs copy = a;
    if (hipError_t e = check_grid(blocks, &copy.xcd_swizzle); e != hipSuccess) return e;
    // 32-bit byte offsets inside one tile?  COLS: L rows of `pitch`; ROWS_T: cw rows of `pitch` in, L outputs of out_stride
    const uint64_t L = 1ull << lg_l, cw = a.cw;
    const uint64_t span_in = (cw * a.pitch + L) * 8, span_out = (L * a.out_stride + cw) * 8;
    const uint64_t span = (mode == TILE_COLS) ? L * a.pitch * 8 + cw * 8 : (span_in > span_out ? span_in : span_out);
    const KernelLaunch k = tile_launch(dir, mode, lg_l, span < (1ull << 32), (int)a.role);
    if (!k.kernel || a.cw != TILE_CW) return hipErrorInvalidValue;
    void *args[] = {&copy};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
}

}  // namespace fwa
