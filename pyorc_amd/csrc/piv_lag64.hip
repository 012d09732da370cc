// The 64 x 64 window of frame t against the 64 x 64 window of frame t + k at a per-window lag k and integer offset (piv_lag_impl.h;
// INTEGRATION.md section 2k).
#include "piv_lag_impl.h"

namespace lspiv {
hipError_t launch_piv_lag64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_lag<64>(p, dtype, s);
}
}  // namespace lspiv
