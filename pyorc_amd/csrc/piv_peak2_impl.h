// Second correlation peak for the per-pair PIV kernels (gfx950): the one-window-per-job kernels on the 16 / 32 /
// 64-point transforms that hand out, next to u, v, corr_max and s2n, the height of the second highest correlation peak, the peak ratio
// and the runner-up vector -- what validation by peak ratio needs, without the planes crossing PCIe.
//
// The job is the shifted kernel's at zero offset (piv_fft_impl.h: correlate_job<..., SHIFT> with p.shift == nullptr -> plane_max ->
// find_peak with its rescue records), so u, v, corr_max, s2n and the planes are that kernel's bits; the epilogue below follows it.
// When find_peak returns, the lane still holds row y of the plane in registers (lane = un-shifted row y, register = un-shifted column
// x) and the whole plane is parked in LDS (row y at buf[y * LDS_ROW + x]).  The rule (piv_peak2.h) speaks of the fft-shifted plane:
// shifted row i = (y + N / 2) mod N, shifted column j = (x + N / 2) mod N, and a neighbour exists when its SHIFTED index stays inside
// 0 .. N - 1 -- it then sits at the un-shifted index +- 1 mod N, which is always a valid row of the buffer.
//   * The lane takes its two neighbour rows from LDS four columns at a time (ds_read_b128: N / 2 reads per lane), its horizontal
//     neighbours are registers; N samples, each against the running best (which starts at the floor), the largest of its neighbours and
//     the box -- eight VALU instructions a sample --, a running (value, shifted column) in ascending shifted column, so that a strict >
//     keeps the first of equals.
//   * The group reduces to the largest value (on the bit patterns: candidates are positive) and then to the smallest (row, column) among
//     the lanes that hold it: the first maximum in row-major order.
//   * Four LDS reads around it and peak2_fit (piv_peak2.h), the arithmetic the generic kernel on planes shares.
// The primary's position is found again from what find_peak leaves behind (peak_row is register-only and handed to find_peak as
// ip_known; the column is one LDS read per lane and one reduction), so that find_peak itself stays as it is.
// The second peak is taken on the float32 plane at the float32 arg-max: the float64 rescue pass corrects u, v and leaves these alone.
#pragma once
#include "piv_fft_impl.h"
#include "piv_peak2.h"

namespace lspiv {

// c = this lane's row of the plane, buf = the plane as find_peak parked it, (vmax, ip) = the primary's height and shifted row
template <int N>
__device__ __forceinline__ Peak2 second_peak(const float* buf, int lg, const float (&c)[N], float vmax, int ip, const PivParams& p) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "the second-peak kernels are 16, 32 or 64 px");
  constexpr int LR = Geo<N>::LDS_ROW, C = N / 2, M = N - 1, NONE = 1 << 20;
  const int sh = (lg + C) & M;                                    // this lane's shifted row, and its shifted column in the per-lane reads
  const float rowv = buf[((ip + C) & M) * LR + lg];               // the primary's row, one sample per lane
  const int jp = group_min_i<N>(rowv == vmax ? sh : NONE);        // first shifted column holding the maximum (find_peak's jp)
  // the box as ONE unsigned comparison per sample: (unsigned)(j - lo) <= 2 r, with lo out of reach for a lane whose row is outside it
  const int r = p.peak_excl;
  const unsigned span = 2u * (unsigned)r;
  const int lo = (unsigned)(sh - ip + r) <= span ? jp - r : NONE;
  // a neighbour row that does not exist is the lane's own row (s >= s holds); a column that does not exist is left out at compile time
  const float* up = buf + (sh != 0 ? (lg - 1) & M : lg) * LR;
  const float* down = buf + (sh != M ? (lg + 1) & M : lg) * LR;
  // The comparisons run on the BIT PATTERNS, which order like the values for the non-negative floats of a clipped plane (common.h,
  // half_max_i): v_max3_i32 / v_cmp_*_i32 need no quieting of NaNs on the operands that come from LDS.  A candidate is positive (above
  // the floor), so a -0 among the neighbours -- the smallest integer -- changes nothing
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  int best = __builtin_bit_cast(int, kPeak2Floor);                // (s > floor and s > the best so far are one comparison)
  int bj = 0;
#pragma unroll
  for (int kk = 0; kk < N / 4; ++kk) {
    const int k = (kk + C / 4) & (N / 4 - 1);                     // four columns at a time, in ascending SHIFTED column
    const i32x4 a = *reinterpret_cast<const i32x4*>(up + 4 * k);
    const i32x4 b = *reinterpret_cast<const i32x4*>(down + 4 * k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = 4 * k + e, j = (x + C) & M;
      const int s = __builtin_bit_cast(int, c[x]);
      int nb = max(a[e], b[e]);                                   // the largest existing neighbour
      if (j != 0) nb = max(nb, __builtin_bit_cast(int, c[(x - 1) & M]));
      if (j != M) nb = max(nb, __builtin_bit_cast(int, c[(x + 1) & M]));
      const bool ok = s > best && s >= nb && (unsigned)(j - lo) > span;
      best = ok ? s : best;
      bj = ok ? j : bj;
    }
  }
  const float row_best = best > __builtin_bit_cast(int, kPeak2Floor) ? __builtin_bit_cast(float, best) : 0.0f;   // 0: no candidate in this row
  const float m = group_max_nonneg<N>(row_best);
  const int pos = group_min_i<N>((row_best == m && m > 0.0f) ? ((sh << 8) | bj) : NONE);
  const bool found = pos != NONE;
  const int i2 = found ? pos >> 8 : C, j2 = found ? pos & 255 : C;   // (no candidate: the reads below stay inside the buffer)
  const int y2 = (i2 + C) & M, x2 = (j2 + C) & M;
  const float cu = buf[((y2 - 1) & M) * LR + x2];
  const float cd = buf[((y2 + 1) & M) * LR + x2];
  const float cl = buf[y2 * LR + ((x2 - 1) & M)];
  const float cr = buf[y2 * LR + ((x2 + 1) & M)];
  __builtin_amdgcn_wave_barrier();
  return peak2_fit(vmax, found, i2, j2, m, cu, cd, cl, cr, N, N, p.border_mode, p.peak2_v_neg);
}

// registers (ROCm 7.2, -Rpass-analysis=kernel-resource-usage, no scratch in any of the 36 variants; uint8 | float32 | float64, over the four
// variants with / without signal score and planes): 16-point 60 - 62 | 60 - 69 | 64 - 74 VGPRs, 32-point 92 - 93 | 96 - 100 | 110 - 112,
// 64-point 185 - 186 | 185 - 206 | 202 - 206: inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 / 4 / 2 waves per SIMD) at every size,
// and within 8 VGPRs of the shifted kernel's figures: the epilogue starts when the transforms' registers are free.  The generic kernel
// on planes (piv_peak2_planes.hip): 37 VGPRs, no scratch
template <typename T, int N, bool PLANES, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_peak2_kernel(PivParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using G = Geo<N>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane / G::LG;
  const int lg = lane & (G::LG - 1);
  float* buf = smem + (wave * G::GROUPS + grp) * G::LDS_JOB;
  const int partner_byte = partner_byte_of<N>(lane, lg);
  const uint32_t nb = gridDim.x;                                   // XCD-aware block order, as piv_fft_kernel
  const uint32_t q = nb >> 3, r = nb & 7u;
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  const uint32_t blk = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  // a job is ONE window of one pair; jobs past the end recompute the last job and store nothing
  uint32_t job = (blk * WAVES_PER_BLOCK + wave) * G::GROUPS + grp;
  const bool job_valid = job < p.n_tiles;
  job = job_valid ? job : p.n_tiles - 1;
  const uint32_t pair = p.div_nwin.div(job);
  TileRef t[2];
  t[0].pair = t[1].pair = pair;
  t[0].win = t[1].win = job - pair * p.n_win;
  t[0].valid = job_valid;
  t[1].valid = false;

  float xr[N], xi[N], mean[2];
  bool skip[2];
  correlate_job<T, N, WANT_NZ, false, false, true>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);   // (p.shift == nullptr: zero offsets)

  float row_max, u, v;
  const uint32_t g = job;
  const float vmax = plane_max<N>(xr, row_max);
  const int ip = peak_row<N>(lg, vmax, row_max);
  find_peak<N>(buf, lg, xr, vmax, row_max, p, u, v, p.rescue_hdr && job_valid && !skip[0], g, ip);
  Peak2 s2 = second_peak<N>(buf, lg, xr, vmax, ip, p);
  float cm = vmax, sn = vmax * __builtin_amdgcn_rcpf(mean[0]);
  if (skip[0]) u = v = cm = sn = s2.u = s2.v = s2.corr = s2.ratio = __builtin_nanf("");
  if (job_valid && lg == 0) {
    p.u[g] = u; p.v[g] = v; p.cmax[g] = cm; p.s2n[g] = sn;
    f32x4 o;
    o[0] = s2.u; o[1] = s2.v; o[2] = s2.corr; o[3] = s2.ratio;
    *reinterpret_cast<f32x4*>(p.peak2 + 4 * (size_t)g) = o;
  }
  if constexpr (PLANES) {
    if (job_valid) store_plane_rows<N>(p.planes + (size_t)g * G::NN, lg, xr, skip[0]);
  }
}

template <typename T, int N, bool WANT_NZ>
static hipError_t launch_peak2_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_tiles + jobs_per_block - 1) / jobs_per_block;
  if (p.planes)
    hipLaunchKernelGGL((piv_fft_peak2_kernel<T, N, true, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  else
    hipLaunchKernelGGL((piv_fft_peak2_kernel<T, N, false, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_peak2(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "the second-peak kernels are 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_tiles == 0 || p.n_tiles != p.n_pairs * p.n_win || p.H < N || p.W < N || p.shifted || p.shift ||
      p.warped || p.mask || p.win_keep || !p.peak2 || ((uintptr_t)p.peak2 & 15u) || p.peak_excl < 1 || p.peak_excl > N / 4 || !p.u || !p.v ||
      !p.cmax || !p.s2n)
    return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_peak2_t<uint8_t, N, true>(p, s) : launch_peak2_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_peak2_t<float, N, true>(p, s) : launch_peak2_t<float, N, false>(p, s);
    case 2: return nz ? launch_peak2_t<double, N, true>(p, s) : launch_peak2_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lspiv
