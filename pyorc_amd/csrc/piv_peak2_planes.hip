// Second correlation peak on planes that already exist in HBM: cross_corr output, return_planes, an ensemble's
// mean planes.  One wave per plane, any (wy, wx), run-time geometry; the rule and the fit are those of the fused kernels (piv_peak2.h:
// peak2_floor, peak2_fit), so the fused kernels' own planes give their own bits back.  The simple path the register path is checked
// against: every sample is read where it lies, a neighbour that does not exist is replaced by the sample itself (s >= s holds).
#include "piv_peak2.h"

namespace lspiv {

constexpr int kPeak2Block = 256;   // four planes per block

// larger value first, equal values -> the smaller row-major index (np.argmax)
__device__ __forceinline__ void wave_first_max(float& v, int& idx) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float pv = __shfl_xor(v, o, 64);
    const int pi = __shfl_xor(idx, o, 64);
    const bool take = (pv > v) || (pv == v && pi < idx);
    v = take ? pv : v;
    idx = take ? pi : idx;
  }
}

__global__ __launch_bounds__(kPeak2Block) void second_peak_kernel(const float* planes, uint32_t n_planes, int wy, int wx, int r, int border_mode,
                                                                  int v_neg, float* out) {
  const int lane = threadIdx.x & 63;
  const uint32_t g = blockIdx.x * (uint32_t)(kPeak2Block / 64) + (threadIdx.x >> 6);
  if (g >= n_planes) return;   // whole waves
  const int n = wy * wx;
  const float* pl = planes + (size_t)g * n;
  constexpr int NONE = 0x7fffffff;
  // the primary: first maximum in row-major order, a NaN ranks as the maximum (a skipped window's plane is NaN throughout)
  float best = -__builtin_inff();
  int bi = NONE;
  for (int o = lane; o < n; o += 64) {
    float x = pl[o];
    x = (x != x) ? __builtin_inff() : x;
    if (x > best || bi == NONE) { best = x; bi = o; }
  }
  wave_first_max(best, bi);
  const float p1 = pl[bi];
  const int ip = bi / wx, jp = bi - ip * wx;
  // the candidates: a lane meets its samples in ascending row-major order, so a strict > keeps the first of equals
  float b2 = 0.0f;
  int o2 = NONE;
  for (int o = lane; o < n; o += 64) {
    const int i = o / wx, j = o - i * wx;
    const float s = pl[o];
    const float up = pl[i > 0 ? o - wx : o], down = pl[i < wy - 1 ? o + wx : o];
    const float left = pl[j > 0 ? o - 1 : o], right = pl[j < wx - 1 ? o + 1 : o];
    const bool in_box = (unsigned)(i - ip + r) <= (unsigned)(2 * r) && (unsigned)(j - jp + r) <= (unsigned)(2 * r);
    const bool ok = peak2_floor(s) && s > b2 && !in_box && s >= up && s >= down && s >= left && s >= right;
    b2 = ok ? s : b2;
    o2 = ok ? o : o2;
  }
  wave_first_max(b2, o2);
  const bool found = o2 != NONE;
  const int i2 = found ? o2 / wx : 0, j2 = found ? o2 - (o2 / wx) * wx : 0;
  const bool inside = found && i2 > 0 && i2 < wy - 1 && j2 > 0 && j2 < wx - 1;   // the four neighbours exist
  const int oc = inside ? o2 : 0;
  const float cu = pl[inside ? oc - wx : 0], cd = pl[inside ? oc + wx : 0], cl = pl[inside ? oc - 1 : 0], cr = pl[inside ? oc + 1 : 0];
  Peak2 q = peak2_fit(p1, found, i2, j2, b2, cu, cd, cl, cr, wy, wx, border_mode, v_neg);
  if (p1 != p1) q.u = q.v = q.corr = q.ratio = __builtin_nanf("");
  if (lane == 0) {
    float* dst = out + 4 * (size_t)g;
    dst[0] = q.u; dst[1] = q.v; dst[2] = q.corr; dst[3] = q.ratio;
  }
}

hipError_t launch_second_peak(const float* planes, uint32_t n_planes, int wy, int wx, int r, int border_mode, int v_neg, float* out,
                              hipStream_t s) {
  if (n_planes == 0) return hipSuccess;
  if (!planes || !out || wy < 4 || wx < 4 || wy > 4096 || wx > 4096 || r < 1 || r > (wy < wx ? wy : wx) / 4) return hipErrorInvalidValue;
  const uint32_t per_block = kPeak2Block / 64;
  hipLaunchKernelGGL(second_peak_kernel, dim3((n_planes + per_block - 1) / per_block), dim3(kPeak2Block), 0, s, planes, n_planes, wy, wx, r,
                     border_mode, v_neg, out);
  return hipGetLastError();
}

}  // namespace lspiv
