// kernels_rows32b.hip -- the 2048-point instantiations of k_rows32 (rows32.h), a translation unit of their own so that the
// library builds in parallel (4096: kernels_rows32c.hip).
#include "rows32.h"

namespace fwa {

template const void *rows32_kernel<11>(int dir, uint32_t in_cw);

}  // namespace fwa
