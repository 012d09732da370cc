// Launch declarations of the SPOF phase-filtered kernels (piv_spof_impl.h): per pair, and summed over the pairs
// of a run by one owner per window.  hipErrorInvalidValue for another window size, a search window, offsets, a warped stack or rescue lists.
#pragma once
#include "common.h"

namespace lspiv {
hipError_t launch_piv_spof16(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_spof32(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_spof64(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_spof_ensemble16(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_spof_ensemble32(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_spof_ensemble64(const PivParams& p, int dtype, hipStream_t s);
}  // namespace lspiv
