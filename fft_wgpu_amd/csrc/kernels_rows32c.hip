// kernels_rows32c.hip -- the 4096-point instantiations of k_rows32 (rows32.h).
#include "rows32.h"

namespace fwa {

template const void *rows32_kernel<12>(int dir, uint32_t in_cw);

}  // namespace fwa
