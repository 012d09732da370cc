// An even square interrogation window 4 .. 62 searched inside a 64 x 64 search area (piv_fft_impl.h, "search-area mode").
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_search64(const PivParams& p, int dtype, hipStream_t s) {
  return launch_search<64>(p, dtype, s);
}
}  // namespace lspiv
