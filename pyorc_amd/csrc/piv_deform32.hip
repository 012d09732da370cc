// The 32 x 32 window of frame t against the 32 x 32 window of the warped frame t+1 (piv_deform_impl.h, "window deformation pass").
#include "piv_deform_impl.h"

namespace lspiv {
hipError_t launch_piv_deform32(const PivParams& p, int dtype, hipStream_t s) {
  return launch_deform<32>(p, dtype, s);
}
}  // namespace lspiv
