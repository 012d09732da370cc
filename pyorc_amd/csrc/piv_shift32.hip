// The 32 x 32 window of frame t against the 32 x 32 window of frame t+1 at a per-window integer offset (piv_fft_impl.h, "shifted kernel").
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_shift32(const PivParams& p, int dtype, hipStream_t s) {
  return launch_shift<32>(p, dtype, s);
}
}  // namespace lspiv
