// The valid samples of the 64 x 64 window of frame t against those of the 64 x 64 window of frame t+1 under an image mask (piv_masked_impl.h).
#include "piv_masked_impl.h"
#include "piv_masked.h"

namespace lspiv {
hipError_t launch_piv_masked64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_masked<64>(p, dtype, s);
}
}  // namespace lspiv
