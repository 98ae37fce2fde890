// lab_absent.cpp -- what the product library links where the laboratory library links kernels_lab_*.hip (internal.h):
// kLab = false, and the laboratory launchers of kernels.h as stubs.  No plan reaches a stub: fwa_plan_set_i64 refuses,
// when !kLab, every key and path that leads to one (tuning.cpp), and FAM_LAB_RING belongs to path 5 alone.
#include "kernels.h"

namespace fwa {

const bool kLab = false;

hipError_t launch_small16(int, const v2f *, v2f *, const v2f *, uint32_t, uint64_t, float, bool, hipStream_t)
{
    return hipErrorNotSupported;
}
size_t ring_ctl_bytes(uint64_t) { return 0; }
hipError_t setup_lab_1m_kernels() { return hipSuccess; }
hipError_t launch_ring_1m(int, const v2f *, v2f *, v2f *, const v2f *, const v2f *, uint32_t *, uint32_t, uint32_t, uint32_t,
                          uint32_t, float, hipStream_t)
{
    return hipErrorNotSupported;
}

}  // namespace fwa
