// The 16 x 16 window of frame t against the 16 x 16 window of frame t+1 at a per-window integer offset (piv_fft_impl.h, "shifted kernel"),
// per pair (multi-pass PIV) and summed over the pairs of a run (multi-pass ensemble, "shifted ensemble kernel").
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_shift16(const PivParams& p, int dtype, hipStream_t s) {
  return launch_shift<16>(p, dtype, s);
}
hipError_t launch_piv_shift_ensemble16(const PivParams& p, int dtype, hipStream_t s) {
  return launch_shift_ensemble<16>(p, dtype, s);
}
}  // namespace lspiv
