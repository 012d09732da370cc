// Second correlation peak: launch declarations of the second-peak per-pair kernels (piv_peak2_impl.h) and of
// the generic kernel on planes in HBM (piv_peak2_planes.hip), and the ONE place the rule's floor and the fit of the second peak live --
// both kernels call peak2_floor and peak2_fit, so the same plane gives the same bits on either path.
//
// The rule, on the fft-shifted plane: with (ip, jp) the primary peak (first maximum in row-major order), p1 its height and r the
// exclusion radius, a sample s at (i, j) is a candidate when s >= 1e-5, (i, j) lies outside the box |i - ip| <= r and |j - jp| <= r
// (clipped at the plane edge, no wrap) and s >= each of its existing 4-neighbours (one inside the box counts).  The second peak is the
// largest candidate, the first in row-major order among equals.
#pragma once
#include "common.h"

namespace lspiv {

// hipErrorInvalidValue for another window size, a search window, offsets, a warped stack, a mask, no output or a radius outside 1 .. N / 4
hipError_t launch_piv_peak2_16(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_peak2_32(const PivParams& p, int dtype, hipStream_t s);
hipError_t launch_piv_peak2_64(const PivParams& p, int dtype, hipStream_t s);
// planes: n_planes fft-shifted planes of wy x wx in HBM (a NaN plane is a skipped window) -> out: n_planes x {u2, v2, corr2, peak_ratio}
hipError_t launch_second_peak(const float* planes, uint32_t n_planes, int wy, int wx, int r, int border_mode, int v_neg, float* out,
                              hipStream_t s);

// s >= 1e-5 for a float32 sample: 1e-5f is the float32 just BELOW 1e-5, so the comparison with the real number is the strict one with it.
// Five times the plane gate of 2e-6: float32 noise around an isolated peak is no peak
constexpr float kPeak2Floor = 1e-5f;
__device__ __forceinline__ bool peak2_floor(float s) { return s > kPeak2Floor; }

struct Peak2 { float u, v, corr, ratio; };

// The four outputs of a window from its primary height p1 and its second peak at shifted (i2, j2) on a wy x wx plane: c0 its height, up /
// down = the samples at (i2 -+ 1, j2), left / right at (i2, j2 -+ 1) (anything when the peak is on the border: they are not used there).
// The primary's rule: the 3-point log-Gaussian fit on plane + 1e-7 inside (v_log_f32 and a 1-ulp reciprocal as in find_peak), the
// border mode on the plane border.  found = false (no candidate): corr2 = 0, peak_ratio = +inf, u2 = v2 = NaN
__device__ __forceinline__ Peak2 peak2_fit(float p1, bool found, int i2, int j2, float c0, float up, float down, float left, float right,
                                           int wy, int wx, int border_mode, int v_neg) {
  Peak2 q;
  if (!found) {
    q.u = q.v = __builtin_nanf("");
    q.corr = 0.0f;
    q.ratio = __builtin_inff();
    return q;
  }
  const float l0 = __builtin_amdgcn_logf(c0 + kEpsPeak);
  q.v = (float)i2 + gauss_offset_fast(__builtin_amdgcn_logf(up + kEpsPeak), l0, __builtin_amdgcn_logf(down + kEpsPeak)) - (float)(wy / 2);
  q.u = (float)j2 + gauss_offset_fast(__builtin_amdgcn_logf(left + kEpsPeak), l0, __builtin_amdgcn_logf(right + kEpsPeak)) - (float)(wx / 2);
  if (i2 == 0 || i2 == wy - 1 || j2 == 0 || j2 == wx - 1) border_result(border_mode, j2 - wx / 2, i2 - wy / 2, q.u, q.v);
  if (v_neg) q.v = -q.v;
  q.corr = c0;
  q.ratio = p1 / c0;
  return q;
}

}  // namespace lspiv
