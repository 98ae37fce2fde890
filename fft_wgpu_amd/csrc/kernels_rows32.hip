// kernels_rows32.hip -- k_rows32, the last pass of the two-pass plans (512 .. 4096-point rows with the transposed store):
// picker, launcher and the 512 / 1024-point instantiations (template: rows32.h; 2048 / 4096: kernels_rows32b.hip / c.hip).
#include "rows32.h"

namespace fwa {

// kernel = nullptr: no such row length, or no ring input of that width at this row length
static KernelLaunch rows32_launch(int dir, uint32_t lg_l, uint32_t in_cw)
{
    if (!rows32_supported(lg_l) || (in_cw && !rows32_ring_supported(lg_l, in_cw))) return {};
    const uint32_t threads = (uint32_t)rows32_rows((int)lg_l) << (lg_l - 5);
    switch (lg_l) {
        case 9: return {rows32_kernel<9>(dir, in_cw), threads, Rows32<9, rows32_rows(9)>::LDS_BYTES};
        case 10: return {rows32_kernel<10>(dir, in_cw), threads, Rows32<10, rows32_rows(10)>::LDS_BYTES};
        case 11: return {rows32_kernel<11>(dir, in_cw), threads, Rows32<11, rows32_rows(11)>::LDS_BYTES};
        default: return {rows32_kernel<12>(dir, in_cw), threads, Rows32<12, rows32_rows(12)>::LDS_BYTES};
    }
}

hipError_t setup_rows32_kernels()
{
    hipError_t e = hipSuccess;
    for (uint32_t lg_l = 9; lg_l <= 12; ++lg_l)
        for (int dir : {FWD, INV})
            for (uint32_t in_cw : {0u, 32u, 64u})
                if (e == hipSuccess) e = raise_lds_limit(rows32_launch(dir, lg_l, in_cw));
    return e;
}

// n = n1 * 2^lg_l per transform, n * 8 < 2^32; `in`: n1 rows of 2^lg_l contiguous samples (in_cw = 0) or the
// tile-contiguous ring of k_colsw (in_cw = its tile width); out[k1 + n1*k2]
hipError_t launch_rows32(int dir, uint32_t lg_l, const v2f *in, v2f *out, const v2f *tw, uint32_t n1, uint64_t in_sb,
                         uint64_t out_sb, uint32_t n_transforms, float scale, uint32_t xcd_swizzle, uint32_t in_cw,
                         hipStream_t st)
{
    if (n_transforms == 0) return hipSuccess;
    const KernelLaunch k = rows32_launch(dir, lg_l, in_cw);
    if (!k.kernel || n1 < 16 || (n1 & (n1 - 1)) || ((uint64_t)n1 << lg_l) > (1ull << 28)) return hipErrorInvalidValue;
    const uint64_t blocks = (uint64_t)n_transforms * (n1 / rows32_rows((int)lg_l));
    if (hipError_t e = check_grid(blocks, &xcd_swizzle); e != hipSuccess) return e;
    void *args[] = {&in, &out, &tw, &n1, &in_sb, &out_sb, &scale, &xcd_swizzle};
    return hipLaunchKernel(k.kernel, dim3((uint32_t)blocks), dim3(k.threads), args, (size_t)k.lds, st);
}

}  // namespace fwa
