// An even square interrogation window 4 .. 30 searched inside a 32 x 32 search area (piv_fft_impl.h, "search-area mode").
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_search32(const PivParams& p, int dtype, hipStream_t s) {
  return launch_search<32>(p, dtype, s);
}
}  // namespace lspiv
