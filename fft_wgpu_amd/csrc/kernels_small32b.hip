// kernels_small32b.hip -- the 8192 .. 32768-point instantiations of k_small32 (small32_kernel.h), a translation unit of
// their own so that the library builds in parallel.
#include "small32_kernel.h"

namespace fwa {

template hipError_t launch_small32_n<13>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);
template hipError_t launch_small32_n<14>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);
template hipError_t launch_small32_n<15>(int, const v2f *, v2f *, const v2f *, uint64_t, float, hipStream_t);

// 16384 / 32768-point transforms need 66 / 132 KiB of dynamic LDS (8192: 33 KiB, inside the default limit)
hipError_t setup_small32_kernels()
{
    const KernelLaunch ks[] = {{reinterpret_cast<const void *>(&k_small32<14, FWD>), 512, (int)small32_lds(14)},
                               {reinterpret_cast<const void *>(&k_small32<14, INV>), 512, (int)small32_lds(14)},
                               {reinterpret_cast<const void *>(&k_small32<15, FWD>), 1024, (int)small32_lds(15)},
                               {reinterpret_cast<const void *>(&k_small32<15, INV>), 1024, (int)small32_lds(15)}};
    hipError_t e = hipSuccess;
    for (const KernelLaunch &k : ks)
        if (e == hipSuccess) e = raise_lds_limit(k);
    return e;
}

}  // namespace fwa
