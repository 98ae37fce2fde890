// lab_present.cpp -- linked into the laboratory library beside kernels_lab_*.hip, which define the laboratory launchers of
// kernels.h (the product links lab_absent.cpp instead: internal.h).  A host file of its own: a constant defined in a .hip
// file is emitted into the device code too.
#include "kernels.h"

namespace fwa {

const bool kLab = true;

}  // namespace fwa
