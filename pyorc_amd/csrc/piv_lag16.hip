// The 16 x 16 window of frame t against the 16 x 16 window of frame t + k at a per-window lag k and integer offset (piv_lag_impl.h;
// INTEGRATION.md section 2k).
#include "piv_lag_impl.h"

namespace lspiv {
hipError_t launch_piv_lag16(const PivParams& p, int dtype, hipStream_t s) {
  return launch_lag<16>(p, dtype, s);
}
}  // namespace lspiv
