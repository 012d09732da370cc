// The 64 x 64 window of frame t against the 64 x 64 window of frame t+1 through the symmetric phase-only filter (piv_spof_impl.h), per pair
// and summed over the pairs of a run ("filtered ensemble kernel").
#include "piv_spof_impl.h"
#include "piv_spof.h"

namespace lspiv {
hipError_t launch_piv_spof64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_spof<64>(p, dtype, s);
}
hipError_t launch_piv_spof_ensemble64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_spof_ensemble<64>(p, dtype, s);
}
}  // namespace lspiv
