// The 16 x 16 window pair with the second correlation peak next to the first (piv_peak2_impl.h).
#include "piv_peak2_impl.h"

namespace lspiv {
hipError_t launch_piv_peak2_16(const PivParams& p, int dtype, hipStream_t s) {
  return launch_peak2<16>(p, dtype, s);
}
}  // namespace lspiv
