// The peak finder on a plane volume that has no frames behind it (piv_direct.hip, peaks_kernel): ffpiv.u_v_displacement on caller-supplied
// planes, and lspiv_ensemble_finish / lspiv_ensemble_sliding_finish when the frames of the sum are not all at hand (an imported state, a
// chunk that could not be retained).  The float64 rescue pass re-evaluates a flagged window from the frames; here there is nothing to go
// back to but the plane, and nothing else is needed: the plane's float32 samples ARE the input, so the arg-max is exact and the only
// error is the float32 arithmetic of the fit (hardware log2, 1-ulp reciprocal) -- up to 2e-3 of max(|result|, 0.05 px) on broad, low
// peaks, 20 times the parity gate.  With refit_k > 0 the windows common.h's peak_cond flags at that k (near_tie = false) get the fit of
// their five samples again as log((double)x + 1e-7) in float64; every other window keeps the bits of the float32 fit, which are the bits
// of the fused kernels.  Declared here, and not in common.h, because nothing the fused PIV kernels see changes with it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lspiv {
// n_refit (device, may be nullptr): incremented once per re-fitted plane.  refit_k = 0: launch_peaks_from_planes of common.h.
hipError_t launch_peaks_from_planes(const float* planes, uint32_t n_planes, int wy, int wx, int border_mode, float* u, float* v,
                                    float refit_k, uint32_t* n_refit, hipStream_t s);
}  // namespace lspiv
