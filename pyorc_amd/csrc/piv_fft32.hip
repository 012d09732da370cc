// 32x32 interrogation windows: instantiation of the fused FFT kernels (piv_fft_impl.h).
#include "piv_fft_impl.h"

namespace lspiv {
hipError_t launch_piv_fft32(const PivParams& p, int dtype, bool ensemble, hipStream_t s) {
  return launch_fft<32>(p, dtype, ensemble, s);
}
}  // namespace lspiv

// test hook (include/lspiv.h): the paired column map as this translation unit compiles it
extern "C" int lspiv_debug_unpack_map(int i, int* col, int* col_rt, int* lane) {
  if (i < 0 || i >= 32 || !col || !col_rt || !lane) return 1;   // LSPIV_EINVAL
  *col = lspiv::unpack_col(i);
  *col_rt = lspiv::unpack_col_of(i);
  *lane = lspiv::unpack_lane(i);
  return 0;
}
