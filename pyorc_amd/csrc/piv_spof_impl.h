// SPOF phase-filtered correlation (gfx950): the one-window-per-job kernels on the 16 / 32 / 64-point transforms
// with the symmetric phase-only filter between the cross spectrum and the inverse transform.
//
// The shifted kernel's job at zero offset (piv_fft_impl.h: one window per job, one plane per inverse transform, the full-plane epilogue,
// both windows in the stack's type T through prepare_pair) with every bin of the cross spectrum replaced by R / sqrt(|R|) while the half
// spectrum sits in registers.  The reference's Rn = conj(fft2 a) fft2 b / N^2 goes through numpy's ifft2 (which divides by N^2); the
// device's R is Rn / N^2 (finish_pair's scale) and its inverse is unnormalised, so
//     plane = sum Rn / sqrt(|Rn|) / N^2 = sum R / sqrt(N^2 |R|):   the factor on the scaled R is rsqrt(N^2 |R|).
// |R| = sqrt(Rr^2 + Ri^2) and the factor come from v_sqrt_f32 / v_rsq_f32 (1 ulp each).  Bins whose squared magnitude is below kSpofTiny
// go to zero: the map is continuous there, such a bin would contribute sqrt(|R|) / N < 1e-17^(1/2) / 16 = 2e-10 to any sample.  A
// zero-variance window has scale 0, so R = 0 in every bin and the plane is exactly zero; a non-finite sample gives NaN bins, which the
// comparison sends to zero as well (the plane is NaN through `skip`, as everywhere).
// The mean of the plane is NOT its DC bin here: an NCC plane of non-negative windows is non-negative and the clip removes rounding
// only, a filtered plane has true negative lobes -- the clipped registers are added up (N per lane in a tree, then the group reduction).
// No float64 rescue: the rescue passes re-evaluate a plane by direct lag sums of the samples, a filtered plane has no such form.  The
// kernels are launched without rescue lists and find_peak is called with note = false.
#pragma once
#include "piv_fft_impl.h"

namespace lspiv {

constexpr float kSpofTiny = 1e-34f;   // |R|^2 below this (|R| < 1e-17): the bin is dropped

// R -> R / sqrt(N^2 |R|) in place on the half spectrum of every lane; no live array beyond Rr / Ri
template <int N>
__device__ __forceinline__ void spof_filter(float (&Rr)[N / 2 + 1], float (&Ri)[N / 2 + 1]) {
  constexpr float nn = (float)Geo<N>::NN;
#pragma unroll
  for (int ky = 0; ky <= N / 2; ++ky) {
    const float m2 = Rr[ky] * Rr[ky] + Ri[ky] * Ri[ky];
    const float f = m2 > kSpofTiny ? __builtin_amdgcn_rsqf(nn * __builtin_amdgcn_sqrtf(m2)) : 0.0f;   // (NaN compares false)
    Rr[ky] *= f;
    Ri[ky] *= f;
  }
}

// float64 rows, narrowed half a row at a time: load_center's conversion and arithmetic (the same bits; the signal score is an integer
// count, so its order is free), but at most N / 2 samples of float64 in flight and the score taken half by half, before the statistics.
// With prepare_pair's order -- the whole row in flight, then score and statistics of 64 samples in one block next to window A -- the
// 64-point kernels with the signal score took 256 VGPRs and 52 - 72 bytes of scratch
template <int N>
__device__ __forceinline__ float load_center_f64(const double* row, float (&x)[N], bool want_nz, bool nz_pos, int& nonzero, bool& finite) {
  static_assert(Geo<N>::FULL, "every lane of the group holds a row");
  int c = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int k = h * (N / 4); k < (h + 1) * (N / 4); ++k) {
      const f64x2 v = *reinterpret_cast<const f64x2_u*>(row + 2 * k);
      x[2 * k + 0] = (float)v[0]; x[2 * k + 1] = (float)v[1];
    }
    if (want_nz) {
#pragma unroll
      for (int k = h * (N / 2); k < (h + 1) * (N / 2); ++k) c += (nz_pos ? x[k] > 0.0f : x[k] != 0.0f) ? 1 : 0;   // center_clip_f's score
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (want_nz) nonzero = group_sum_i<N>(c);
  int unused = 0;
  return center_clip_f<N>(x, false, nz_pos, unused, finite);
}
// prepare_pair (SEQ) on float64 rows through load_center_f64
template <int N>
__device__ __forceinline__ void prepare_pair_f64(const double* rowa, const double* rowb, float (&xr)[N], float (&xi)[N], bool want_nz, float thr,
                                                 bool nz_pos, float& scale, float& hi, bool& skip) {
  bool finite = true;
  int nza = Geo<N>::NN, nzb = Geo<N>::NN;
  const float inv_a = load_center_f64<N>(rowa, xr, want_nz, nz_pos, nza, finite);
  const float inv_b = load_center_f64<N>(rowb, xi, want_nz, nz_pos, nzb, finite);
  float rho;
  finish_pair<N>(inv_a, inv_b, rho, scale, hi);
#pragma unroll
  for (int j = 0; j < N; ++j) xi[j] *= rho;
  skip = !finite || (want_nz && below_threshold<N>(nza, nzb, thr));
}

// correlate_job's SINGLE path with the filter: xr = the clipped plane (lane = row y, register = column x), mean = the mean of the clipped plane
template <typename T, int N, bool WANT_NZ>
__device__ __forceinline__ void correlate_spof(const PivParams& p, const TileRef& t, float* buf, int lg, int partner_byte, float (&xr)[N],
                                               float (&xi)[N], bool& skip, float& mean) {
  constexpr int H = N / 2;
  float Rr[H + 1], Ri[H + 1];
  float scale, hi;
  const uint32_t wrow = p.div_ncols.div(t.win);
  const uint32_t wcol = t.win - wrow * (uint32_t)p.n_cols;
  const int64_t off = ((int64_t)t.pair * p.H + (int64_t)(wrow * p.sy + lg)) * p.W + (int64_t)wcol * p.sx;
  const T* rowa = static_cast<const T*>(p.frames) + off;
  if constexpr (sizeof(T) == 8) {
    prepare_pair_f64<N>(rowa, rowa + p.frame_elems, xr, xi, WANT_NZ, p.signal_threshold, p.nz_positive != 0, scale, hi, skip);
  } else {
    RowRaw<T, N> ra, rb;
    ra.fetch(rowa);
    rb.fetch(rowa + p.frame_elems);
    if constexpr (sizeof(T) == 1)
      prepare_pair(ra, rb, xr, xi, WANT_NZ, p.signal_threshold, p.nz_positive != 0, scale, hi, skip);
    else   // one window after the other (prepare_pair, SEQ), as the shifted kernel
      prepare_pair<T, N, true>(ra, rb, xr, xi, WANT_NZ, p.signal_threshold, p.nz_positive != 0, scale, hi, skip);
  }
  scale *= p.std_gain2;              // the filter is not linear: the "std_ddof" gain has to be on R before it
  fft_n<false>(xr, xi);              // along x
  transpose2<N>(buf, lg, xr, xi);    // lane = kx, regs = y
  fft_n<false>(xr, xi);              // along y -> Z[ky][kx]
  cross_spectrum_half<N>(partner_byte, xr, xi, scale, Rr, Ri);
  spof_filter<N>(Rr, Ri);
  __builtin_amdgcn_sched_barrier(0);
  // Q = R' for ky <= N/2, the conjugate of the mirrored lane above (|R| is the same in both halves): the imaginary plane comes out ~0
#pragma unroll
  for (int ky = 0; ky <= H; ++ky) { xr[ky] = Rr[ky]; xi[ky] = Ri[ky]; }
#pragma unroll
  for (int ky = 1; ky < H; ++ky) {
    xr[N - ky] = bperm_f(partner_byte, Rr[ky]);
    xi[N - ky] = -bperm_f(partner_byte, Ri[ky]);
  }
  __builtin_amdgcn_sched_barrier(0);
  fft_n<true>(xr, xi);                 // along ky
  transpose2<N>(buf, lg, xr, xi);      // lane = y, regs = kx
  fft_n<true>(xr, xi);                 // along kx
#pragma unroll
  for (int j = 0; j < N; ++j) xr[j] = __builtin_amdgcn_fmed3f(xr[j], 0.0f, hi);
  mean = group_sum<N>(tree_sum<N>(xr)) * (1.0f / Geo<N>::NN);
}

// registers (ROCm 7.2, -Rpass-analysis=kernel-resource-usage, no scratch in any variant; uint8 | float32 | float64, over the four variants
// with / without signal score and planes): 16-point 51 - 56 | 56 - 60 | 56 - 60 VGPRs, 32-point 100 - 105 | 104 - 109 | 100 - 108, 64-point
// 199 - 204 | 203 - 208 | 203 - 214: inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 / 4 / 2 waves per SIMD) at every size
template <typename T, int N, bool PLANES, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_spof_kernel(PivParams p) {
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
  TileRef t;
  t.pair = p.div_nwin.div(job);
  t.win = job - t.pair * p.n_win;
  t.valid = job_valid;

  float xr[N], xi[N], mean;
  bool skip;
  correlate_spof<T, N, WANT_NZ>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);

  float row_max, u, v;
  const uint32_t g = job;
  const float vmax = plane_max<N>(xr, row_max);
  find_peak<N>(buf, lg, xr, vmax, row_max, p, u, v, false, g);
  float cm = vmax, sn = vmax * __builtin_amdgcn_rcpf(mean);
  if (skip) u = v = cm = sn = __builtin_nanf("");
  if (job_valid && lg == 0) {
    p.u[g] = u; p.v[g] = v; p.cmax[g] = cm; p.s2n[g] = sn;
  }
  if constexpr (PLANES) {
    if (job_valid) store_plane_rows<N>(p.planes + (size_t)g * G::NN, lg, xr, skip);
  }
}

// ---- filtered ensemble kernel: piv_fft_shift_ensemble_kernel's skeleton at zero offset on the filtered planes ----------------------------
// A job owns ONE window and walks the pairs of the chunk in order, one plane per inverse transform: a window's sum is a function of its
// own samples alone, added up in absolute pair order by its single owner (no atomics, no segments) -- the same bits for EVERY chunking,
// odd chunk starts included.  corr_sum / corr_count / the per-pair cmax and s2n are written as piv_fft_ensemble_kernel writes them.
// registers (ROCm 7.2, no scratch in any variant; uint8 | float32 | float64, without - with the signal score): 16-point 58 | 60 - 62 |
// 65 - 67 VGPRs, 32-point 105 | 104 - 110 | 103 - 118, 64-point 207 | 206 | 206 - 216: inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 / 4 / 2 waves per SIMD) at every size
template <typename T, int N, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_spof_ensemble_kernel(PivParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using G = Geo<N>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane / G::LG;
  const int lg = lane & (G::LG - 1);
  float* buf = smem + (wave * G::GROUPS + grp) * G::LDS_JOB;
  const int partner_byte = partner_byte_of<N>(lane, lg);
  const uint32_t job = (blockIdx.x * WAVES_PER_BLOCK + wave) * G::GROUPS + grp;
  const bool valid = job < p.n_win;
  const uint32_t w = valid ? job : p.n_win - 1;   // jobs past the end recompute the last window and store nothing
  float cnt = 0.0f;
  for (uint32_t pair = 0; pair < p.n_pairs; ++pair) {
    const TileRef t = {pair, w, valid};
    float xr[N], xi[N], mean;
    bool skip;
    correlate_spof<T, N, WANT_NZ>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);
    float row_max;
    const float vmax = plane_max<N>(xr, row_max);
    float cm = vmax, sn = vmax * __builtin_amdgcn_rcpf(mean);
    const bool keep = valid && !skip && (cm >= p.corr_min) && (sn >= p.s2n_min);  // NaN s2n compares false
    cm = keep ? cm : 0.0f;
    sn = keep ? sn : 0.0f;
    cnt += (cm > 1e-6f) ? 1.0f : 0.0f;
    if (valid && lg == 0) {
      p.cmax[(size_t)pair * p.n_win + w] = cm;
      p.s2n[(size_t)pair * p.n_win + w] = sn;
    }
    if (keep) accumulate_planes<N>(p.corr_sum + (size_t)w * G::NN, lg, xr, true, xi, false);   // (the empty second slot adds +0)
  }
  if (valid && lg == 0) p.corr_count[w] += cnt;
}

template <typename T, int N, bool WANT_NZ>
static hipError_t launch_spof_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_tiles + jobs_per_block - 1) / jobs_per_block;
  if (p.planes)
    hipLaunchKernelGGL((piv_fft_spof_kernel<T, N, true, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  else
    hipLaunchKernelGGL((piv_fft_spof_kernel<T, N, false, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_spof(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "filtered correlation is 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_tiles == 0 || p.n_tiles != p.n_pairs * p.n_win || p.H < N || p.W < N || p.shifted || p.warped ||
      p.win_keep || p.rescue_hdr || !p.u || !p.v || !p.cmax || !p.s2n)
    return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_spof_t<uint8_t, N, true>(p, s) : launch_spof_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_spof_t<float, N, true>(p, s) : launch_spof_t<float, N, false>(p, s);
    case 2: return nz ? launch_spof_t<double, N, true>(p, s) : launch_spof_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

template <typename T, int N, bool WANT_NZ>
static hipError_t launch_spof_ensemble_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_win + jobs_per_block - 1) / jobs_per_block;
  hipLaunchKernelGGL((piv_fft_spof_ensemble_kernel<T, N, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_spof_ensemble(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "filtered correlation is 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_win == 0 || p.n_pairs == 0 || p.H < N || p.W < N || p.shifted || p.warped || p.win_keep ||
      !p.corr_sum || !p.corr_count || !p.cmax || !p.s2n)
    return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_spof_ensemble_t<uint8_t, N, true>(p, s) : launch_spof_ensemble_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_spof_ensemble_t<float, N, true>(p, s) : launch_spof_ensemble_t<float, N, false>(p, s);
    case 2: return nz ? launch_spof_ensemble_t<double, N, true>(p, s) : launch_spof_ensemble_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lspiv
