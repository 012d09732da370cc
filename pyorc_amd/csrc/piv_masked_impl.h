// Image mask for the per-pair PIV kernels (gfx950): the one-window-per-job kernels on the 16 / 32 / 64-point
// transforms that correlate only the VALID samples of each window.
//
// The shifted kernel's job at zero offset (piv_fft_impl.h: one window per job, one plane per inverse transform, the full-plane epilogue with
// find_peak and its rescue records) with the window's row of the mask next to its two sample rows.  With M the window of the mask
// (p.mask: H x W bytes, non-zero = valid, the same for every frame) and k = sum M:
//     mean = sum M A / k,  std = sqrt(sum M (A - mean)^2 / k),  a^ = max((A - mean) / std, 0) on valid samples, EXACTLY 0 on excluded ones,
//     plane = clip(fftshift(irfft2(conj(rfft2 a^) rfft2 b^)) / k, 0, 1);   k < p.k_min: NaN throughout (`skip`).
// An excluded sample never enters the arithmetic -- it is selected away, not multiplied by zero --, so a NaN / Inf there changes no bit.
//
// Form of the mask on the device: the caller's bytes, as they are.  A lane loads the N bytes of its row (N / 4 dwords, the loader of the
// uint8 rows) and folds them at once into ONE BIT PER SAMPLE (1 VGPR at 16 / 32, 2 at 64) and the row's count (v_bcnt), so the N / 4 dwords
// live only while the registers of the transforms are still free; no canonical copy, no workspace.
//   uint8 rows: the packed sample dwords are ANDed with 0xFF per valid byte while the mask dwords are there; k, sum and sum of squares are
//     the integer v_dot4 sums of stats_u8 over the ANDed bytes (exact), and an excluded byte -- now 0 -- centres to -mean * g <= 0, which
//     the zero clip of center_u8 takes to exactly 0: no select after the AND, the bits are not kept at all.
//   float rows: the mean of valid samples can be negative, the clip selects nothing: a sample is ANDed with the sign-extended bit
//     (v_bfe_i32 + v_and_b32) after the load -- before any sum sees it --, after the pivot (center_clip_masked) and after centring.
//     float64 rows are narrowed half a row at a time as load_center_f64 does (piv_spof_impl.h).
// The scale on the cross spectrum is finish_pair's times N^2 / k (the divisor of the plane is k, not N^2), "std_ddof" is (k - 1) / k per
// window; with k = N^2 both factors are exactly 1 and (N^2 - 1) / N^2, the plain kernels' values.  The plane is non-negative before the
// clip, so its mean over all N^2 samples is the DC bin as in correlate_job.  signal_threshold is the share among the VALID samples.
#pragma once
#include "piv_fft_impl.h"

namespace lspiv {

template <int N>
struct MaskRow {
  uint32_t bits[(N + 31) / 32];   // bit j & 31 of word j / 32: sample j of this lane's row is valid
  // x where sample j is valid, +0 elsewhere -- a select on the bits of x (j is a constant after unrolling)
  __device__ __forceinline__ float pick(int j, float x) const {
    const int on = -(int)((bits[j >> 5] >> (j & 31)) & 1u);
    return __builtin_bit_cast(float, __builtin_bit_cast(int, x) & on);
  }
};

// the N mask bytes of a row -> bits; each_word(k, ff) sees 0xFF in every valid byte of dword k; returns the window's count k
template <int N, typename F>
__device__ __forceinline__ int mask_row(const uint8_t* q, MaskRow<N>& m, F&& each_word) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "masked correlation is 16, 32 or 64 px");
  RowRaw<uint8_t, N> raw;
  raw.fetch(q);
  int cnt = 0;
#pragma unroll
  for (int w = 0; w < (N + 31) / 32; ++w) m.bits[w] = 0u;
#pragma unroll
  for (int k = 0; k < N / 4; ++k) {
    const uint32_t one = (((((raw.w[k] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | raw.w[k]) & 0x80808080u) >> 7);   // 0x01 in every non-zero byte
    cnt += __builtin_popcount(one);
    each_word(k, one * 0xFFu);
    // bytes 0 .. 3 -> bits 21 .. 24 of the product (the sixteen partial products land on distinct bits: no carries)
    m.bits[k >> 3] |= ((one * 0x00204081u >> 21) & 0xFu) << (4 * (k & 7));
  }
  return group_sum_i<N>(cnt);
}

// stats_u8 over the valid bytes (the rows are ANDed already: excluded bytes are zero and add nothing to any sum)
template <int N>
__device__ __forceinline__ RowStats stats_u8_masked(const RowRaw<uint8_t, N>& raw, uint32_t k, bool want_nz, int& nonzero) {
  uint32_t s = 0, q = 0;
#pragma unroll
  for (int w = 0; w < N / 4; ++w) {
    s = __builtin_amdgcn_udot4(raw.w[w], 0x01010101u, s, false);
    q = __builtin_amdgcn_udot4(raw.w[w], raw.w[w], q, false);
  }
  if (want_nz) {
    int nz = 0;
#pragma unroll
    for (int w = 0; w < N / 4; ++w) {
      const uint32_t t = ~(((raw.w[w] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | raw.w[w] | 0x7F7F7F7Fu);
      nz += 4 - __builtin_popcount(t);
    }
    nonzero = group_sum_i<N>(nz);
  }
  const uint32_t S = (uint32_t)group_sum_i<N>((int)s);
  const uint32_t Q = (uint32_t)group_sum_i<N>((int)q);
  RowStats st;
  const float fk = (float)k;
  st.mean = (float)S / fk;                                   // S < 2^24: one rounding, none at k = N^2
  const uint64_t k2var = (uint64_t)Q * k - (uint64_t)S * (uint64_t)S;
  const float var = (float)k2var / (fk * fk);
  st.inv_std = k2var != 0 ? __builtin_amdgcn_rsqf(var) : 0.0f;
  return st;
}

// position (row * N + column) of the window's first valid sample in row-major order, 0 for a window without one
template <int N>
__device__ __forceinline__ int first_valid(const MaskRow<N>& m, int lg) {
  constexpr int NONE = 1 << 20;
  int c;
  if constexpr (N <= 32) c = m.bits[0] ? __builtin_ctz(m.bits[0]) : NONE;
  else c = m.bits[0] ? __builtin_ctz(m.bits[0]) : m.bits[1] ? 32 + __builtin_ctz(m.bits[1]) : NONE;
  const int f = group_min_i<N>(c >= NONE ? NONE : lg * N + c);
  return f >= NONE ? 0 : f;
}

// center_clip_f over the valid samples: x holds the row with the excluded samples zero already.  The sums run over x - pivot, the pivot a
// valid sample of the window (first_valid; 0 at full coverage, where the pairwise sums are exact for a constant window as in the plain
// kernels and the bits stay theirs): a CONSTANT valid region has exactly zero variance for any k, as the float64 reference finds it --
// the sum of k equal float32 values over k is no exact mean when k is no power of two, and the variance of that rounding would be
// normalised up to a full-scale plane
template <int N>
__device__ __forceinline__ float center_clip_masked(float (&x)[N], const MaskRow<N>& m, float pivot, float inv_k, bool want_nz, bool nz_pos,
                                                    int& nonzero, bool& finite) {
  if (want_nz) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) c += (nz_pos ? x[k] > 0.0f : x[k] != 0.0f) ? 1 : 0;
    nonzero = group_sum_i<N>(c);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = m.pick(k, x[k] - pivot);
  const float s = group_sum<N>(tree_sum<N>(x));
  const float mean = s * inv_k;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float d = m.pick(k, x[k] - mean);
    acc[k & 3] = fmaf(d, d, acc[k & 3]);
    x[k] = fmaxf(d, 0.0f);
  }
  const float ssq = group_sum<N>((acc[0] + acc[1]) + (acc[2] + acc[3]));
  finite = finite && (fabsf(s) <= 3.0e38f) && (ssq <= 3.0e38f);
  const float var = ssq * inv_k;
  return var > 0.0f ? __builtin_amdgcn_rsqf(var) : 0.0f;
}
template <int N>
__device__ __forceinline__ float load_center_masked_row(const float* row, const MaskRow<N>& m, float pivot, float inv_k, float (&x)[N],
                                                        bool want_nz, bool nz_pos, int& nonzero, bool& finite) {
  load_row_f32<N>(row, x);
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = m.pick(k, x[k]);
  return center_clip_masked<N>(x, m, pivot, inv_k, want_nz, nz_pos, nonzero, finite);
}
template <int N>
__device__ __forceinline__ float load_center_masked_row(const double* row, const MaskRow<N>& m, float pivot, float inv_k, float (&x)[N],
                                                        bool want_nz, bool nz_pos, int& nonzero, bool& finite) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {   // at most N / 2 samples of float64 in flight
#pragma unroll
    for (int k = h * (N / 4); k < (h + 1) * (N / 4); ++k) {
      const f64x2 v = *reinterpret_cast<const f64x2_u*>(row + 2 * k);
      x[2 * k + 0] = m.pick(2 * k + 0, (float)v[0]);
      x[2 * k + 1] = m.pick(2 * k + 1, (float)v[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return center_clip_masked<N>(x, m, pivot, inv_k, want_nz, nz_pos, nonzero, finite);
}

// share of signal samples among the k valid ones, for both windows
__device__ __forceinline__ bool below_threshold_masked(int nza, int nzb, float fk, float thr) {
  const float fa = (float)nza / fk, fb = (float)nzb / fk;
  return !(fa >= thr && fb >= thr);
}

// xr = the clipped plane (lane = row y, register = column x), mean = the mean of the plane over all N^2 samples
template <typename T, int N, bool WANT_NZ>
__device__ __forceinline__ void correlate_masked(const PivParams& p, const TileRef& t, float* buf, int lg, int partner_byte, float (&xr)[N],
                                                 float (&xi)[N], bool& skip, float& mean) {
  constexpr int H = N / 2;
  float Rr[H + 1], Ri[H + 1];
  float scale, hi, rho, fk;
  const uint32_t wrow = p.div_ncols.div(t.win);
  const uint32_t wcol = t.win - wrow * (uint32_t)p.n_cols;
  const int64_t moff = (int64_t)(wrow * p.sy + lg) * p.W + (int64_t)wcol * p.sx;   // inside the frame: the grid's windows are
  const T* rowa = static_cast<const T*>(p.frames) + (int64_t)t.pair * p.frame_elems + moff;
  const bool nz_pos = p.nz_positive != 0;
  int nza = 0, nzb = 0;
  uint32_t k;
  if constexpr (sizeof(T) == 1) {
    RowRaw<uint8_t, N> ra, rb;
    ra.fetch(rowa);
    rb.fetch(rowa + p.frame_elems);
    MaskRow<N> m;
    k = (uint32_t)mask_row<N>(p.mask + moff, m, [&](int w, uint32_t ff) { ra.w[w] &= ff; rb.w[w] &= ff; });
    fk = (float)k;
    const RowStats sa = stats_u8_masked<N>(ra, k, WANT_NZ, nza);
    const RowStats sb = stats_u8_masked<N>(rb, k, WANT_NZ, nzb);
    finish_pair<N>(sa.inv_std, sb.inv_std, rho, scale, hi);
    center_u8<N>(ra, sa.mean, 1.0f, xr);
    center_u8<N>(rb, sb.mean, rho, xi);
    skip = false;
  } else {
    MaskRow<N> m;
    k = (uint32_t)mask_row<N>(p.mask + moff, m, [](int, uint32_t) {});
    fk = (float)k;
    const float inv_k = 1.0f / fk;
    // the pivots: each window's first valid sample (inside the window: position 0 for a window without valid samples), 0 at full coverage
    const int fv = first_valid<N>(m, lg);
    const int64_t poff = (int64_t)(fv / N - lg) * p.W + (fv & (N - 1));   // from this lane's row
    const bool full = k == (uint32_t)Geo<N>::NN;
    const float pva = full ? 0.0f : (float)rowa[poff], pvb = full ? 0.0f : (float)rowa[p.frame_elems + poff];
    bool finite = true;
    const float inv_a = load_center_masked_row<N>(rowa, m, pva, inv_k, xr, WANT_NZ, nz_pos, nza, finite);
    __builtin_amdgcn_sched_barrier(0);
    const float inv_b = load_center_masked_row<N>(rowa + p.frame_elems, m, pvb, inv_k, xi, WANT_NZ, nz_pos, nzb, finite);
    finish_pair<N>(inv_a, inv_b, rho, scale, hi);
#pragma unroll
    for (int j = 0; j < N; ++j) xi[j] *= rho;
    skip = !finite;
  }
  skip = skip || k < p.k_min || (WANT_NZ && below_threshold_masked(nza, nzb, fk, p.signal_threshold));
  // divisor k in place of N^2; "std_ddof": (k - 1) / k of THIS window (k >= 2 wherever the plane is kept)
  scale *= (float)Geo<N>::NN / fk;
  if (p.std_gain2 != 1.0f) scale *= (fk - 1.0f) / fk;
  scale = k < p.k_min ? 0.0f : scale;   // (k = 0: no NaN into the transforms; the plane is NaN through `skip` either way)
  fft_n<false>(xr, xi);              // along x
  transpose2<N>(buf, lg, xr, xi);    // lane = kx, regs = y
  fft_n<false>(xr, xi);              // along y -> Z[ky][kx]
  cross_spectrum_half<N>(partner_byte, xr, xi, scale, Rr, Ri);
  __builtin_amdgcn_sched_barrier(0);
  // Q = R for ky <= N/2, the conjugate of the mirrored lane above: the imaginary plane comes out ~0
#pragma unroll
  for (int ky = 0; ky <= H; ++ky) { xr[ky] = Rr[ky]; xi[ky] = Ri[ky]; }
#pragma unroll
  for (int ky = 1; ky < H; ++ky) {
    xr[N - ky] = bperm_f(partner_byte, Rr[ky]);
    xi[N - ky] = -bperm_f(partner_byte, Ri[ky]);
  }
  mean = bperm_f(lane0_byte_of<N>(), xr[0]);   // the DC bin (correlate_job)
  __builtin_amdgcn_sched_barrier(0);
  fft_n<true>(xr, xi);                 // along ky
  transpose2<N>(buf, lg, xr, xi);      // lane = y, regs = kx
  fft_n<true>(xr, xi);                 // along kx
#pragma unroll
  for (int j = 0; j < N; ++j) xr[j] = __builtin_amdgcn_fmed3f(xr[j], 0.0f, hi);
}

// registers (ROCm 7.2, -Rpass-analysis=kernel-resource-usage, no scratch in any of the 36 variants; uint8 | float32 | float64, over the four
// variants with / without signal score and planes): 16-point 49 - 51 | 58 - 68 | 59 - 64 VGPRs, 32-point 93 - 94 | 106 - 114 | 106 - 114,
// 64-point 184 - 185 | 194 - 210 | 195 - 209: inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 / 4 / 2 waves per SIMD) at every size.
// The mask as bits costs the 64-point float64 kernels nothing against their SPOF siblings (203 - 214); one byte per pixel would have held
// 16 more VGPRs through both windows' loads there
template <typename T, int N, bool PLANES, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_masked_kernel(PivParams p) {
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
  // a job is ONE window of one pair (a window's result is a function of its own samples and its own mask alone); jobs past the end
  // recompute the last job and store nothing
  uint32_t job = (blk * WAVES_PER_BLOCK + wave) * G::GROUPS + grp;
  const bool job_valid = job < p.n_tiles;
  job = job_valid ? job : p.n_tiles - 1;
  TileRef t;
  t.pair = p.div_nwin.div(job);
  t.win = job - t.pair * p.n_win;
  t.valid = job_valid;

  float xr[N], xi[N], mean;
  bool skip;
  correlate_masked<T, N, WANT_NZ>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);

  float row_max, u, v;
  const uint32_t g = job;
  const float vmax = plane_max<N>(xr, row_max);
  find_peak<N>(buf, lg, xr, vmax, row_max, p, u, v, p.rescue_hdr && job_valid && !skip, g);
  float cm = vmax, sn = vmax * __builtin_amdgcn_rcpf(mean);
  if (skip) u = v = cm = sn = __builtin_nanf("");
  if (job_valid && lg == 0) {
    p.u[g] = u; p.v[g] = v; p.cmax[g] = cm; p.s2n[g] = sn;
  }
  if constexpr (PLANES) {
    if (job_valid) store_plane_rows<N>(p.planes + (size_t)g * G::NN, lg, xr, skip);
  }
}

template <typename T, int N, bool WANT_NZ>
static hipError_t launch_masked_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_tiles + jobs_per_block - 1) / jobs_per_block;
  if (p.planes)
    hipLaunchKernelGGL((piv_fft_masked_kernel<T, N, true, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  else
    hipLaunchKernelGGL((piv_fft_masked_kernel<T, N, false, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_masked(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "masked correlation is 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_tiles == 0 || p.n_tiles != p.n_pairs * p.n_win || p.H < N || p.W < N || p.shifted || p.warped ||
      p.win_keep || !p.mask || p.k_min < 2 || p.k_min > (uint32_t)Geo<N>::NN || !p.u || !p.v || !p.cmax || !p.s2n)
    return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_masked_t<uint8_t, N, true>(p, s) : launch_masked_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_masked_t<float, N, true>(p, s) : launch_masked_t<float, N, false>(p, s);
    case 2: return nz ? launch_masked_t<double, N, true>(p, s) : launch_masked_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lspiv
