// kernels_tiled_inv.hip -- the inverse-direction instantiations of k_tile (tile_kernel.h), a translation unit of their own so
// that the library builds in parallel.
#include "tile_kernel.h"

namespace fwa {

template const void *tile_kernel<INV>(int mode, uint32_t lg_l, bool buf, int role);

}  // namespace fwa
