// The valid samples of the 32 x 32 window of frame t against those of the 32 x 32 window of frame t+1 under an image mask (piv_masked_impl.h).
#include "piv_masked_impl.h"
#include "piv_masked.h"

namespace lspiv {
hipError_t launch_piv_masked32(const PivParams& p, int dtype, hipStream_t s) {
  return launch_masked<32>(p, dtype, s);
}
}  // namespace lspiv
