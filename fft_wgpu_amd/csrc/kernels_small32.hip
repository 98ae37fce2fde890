// kernels_small32.hip -- one-launch kernels for n = 512 .. 32768, 32 points per thread: launcher and the 512 .. 4096
// instantiations (template: small32_kernel.h; 8192 .. 32768: kernels_small32b.hip).
#include "small32_kernel.h"

namespace fwa {

hipError_t launch_small32(int dir, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint64_t batch, float scale,
                          hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    uint32_t lg_n = 0;
    while ((1u << lg_n) < n) ++lg_n;
    switch (lg_n) {
        case 9: return launch_small32_n<9>(dir, src, dst, tw, batch, scale, st);
        case 10: return launch_small32_n<10>(dir, src, dst, tw, batch, scale, st);
        case 11: return launch_small32_n<11>(dir, src, dst, tw, batch, scale, st);
        case 12: return launch_small32_n<12>(dir, src, dst, tw, batch, scale, st);
        case 13: return launch_small32_n<13>(dir, src, dst, tw, batch, scale, st);
        case 14: return launch_small32_n<14>(dir, src, dst, tw, batch, scale, st);
        case 15: return launch_small32_n<15>(dir, src, dst, tw, batch, scale, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace fwa
