// Launch declarations of the masked per-pair kernels (piv_masked_impl.h).  hipErrorInvalidValue for another
// window size, a search window, offsets, a warped stack, no mask, or k_min outside 2 .. N^2.
#pragma once
#include "common.h"

namespace lspiv {
hipError_t launch_piv_masked16(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_masked32(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_masked64(const PivParams& p, int dtype, hipStream_t s);
}  // namespace lspiv
