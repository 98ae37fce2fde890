// kernels_1m.hip -- (3/3) the n = 2^20 two-pass pipeline (headline config C3): the launchers of k_p1_1m / k_p2_1m (tile_1m.h).
//
// Replaces the 20 global-memory radix-2 passes of reference src/kernel/fft4.wgsl:36-101 by two passes of
// register-resident 32 x 32 FFTs: one HBM round trip plus one round trip through a cache-sized ring.
#include "tile_1m.h"

namespace fwa {

// Pickers.  1024 x 16-column tiles, 512 threads, two workgroups per CU.
static KernelLaunch p1_1m_launch(int dir)
{
    return {dir == FWD ? reinterpret_cast<const void *>(&k_p1_1m<FWD>) : reinterpret_cast<const void *>(&k_p1_1m<INV>),
            Geom::THREADS, Geom::XCH_BYTES + Geom::TWI_BYTES + Geom::TWO_BYTES};
}
static KernelLaunch p2_1m_launch(int dir)
{
    return {dir == FWD ? reinterpret_cast<const void *>(&k_p2_1m<FWD>) : reinterpret_cast<const void *>(&k_p2_1m<INV>),
            Geom::THREADS, Geom::XCH_BYTES + Geom::TWI_BYTES};
}

hipError_t setup_1m_kernels()
{
    hipError_t e = hipSuccess;
    for (int dir : {FWD, INV}) {
        if (e == hipSuccess) e = raise_lds_limit(p1_1m_launch(dir));
        if (e == hipSuccess) e = raise_lds_limit(p2_1m_launch(dir));
    }
    return e;
}

// 64 tiles per transform: the grid is always a multiple of 8, the swizzle stands as given.
hipError_t launch_p1_1m(int dir, const v2f *src, v2f *ring, const v2f *tw_inner, const v2f *tw_outer,
                        uint32_t n_transforms, uint32_t swz, hipStream_t st)
{
    if (n_transforms == 0) return hipSuccess;
    const KernelLaunch k = p1_1m_launch(dir);
    const uint64_t blocks = (uint64_t)n_transforms * Geom::TILES;
    if (hipError_t e = check_grid(blocks); e != hipSuccess) return e;
    void *args[] = {&src, &ring, &tw_inner, &tw_outer, &swz};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
}

hipError_t launch_p2_1m(int dir, const v2f *ring, v2f *dst, const v2f *tw_inner, uint32_t n_transforms,
                        float scale, uint32_t swz, hipStream_t st)
{
    if (n_transforms == 0) return hipSuccess;
    const KernelLaunch k = p2_1m_launch(dir);
    const uint64_t blocks = (uint64_t)n_transforms * Geom::TILES;
    if (hipError_t e = check_grid(blocks); e != hipSuccess) return e;
    void *args[] = {&ring, &dst, &tw_inner, &scale, &swz};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, k.lds, st);
}

}  // namespace fwa
