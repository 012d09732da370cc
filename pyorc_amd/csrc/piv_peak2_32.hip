// The 32 x 32 window pair with the second correlation peak next to the first (piv_peak2_impl.h).
#include "piv_peak2_impl.h"

namespace lspiv {
hipError_t launch_piv_peak2_32(const PivParams& p, int dtype, hipStream_t s) {
  return launch_peak2<32>(p, dtype, s);
}
}  // namespace lspiv
