// An even square interrogation window 4 .. 14 searched inside a 16 x 16 search area (piv_fft_impl.h, "search-area mode").
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_search16(const PivParams& p, int dtype, hipStream_t s) {
  return launch_search<16>(p, dtype, s);
}
}  // namespace lspiv
