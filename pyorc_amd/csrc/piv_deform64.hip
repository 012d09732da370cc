// The 64 x 64 window of frame t against the 64 x 64 window of the warped frame t+1 (piv_deform_impl.h, "window deformation pass").
#include "piv_deform_impl.h"

namespace lspiv {
hipError_t launch_piv_deform64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_deform<64>(p, dtype, s);
}
}  // namespace lspiv
