// Window deformation pass (gfx950): the mixed-type per-pair kernel on the 16 / 32 / 64-point transforms.
//
// The shifted kernel's job (piv_fft_impl.h: one window per job, one plane per inverse transform, the full-plane epilogue) with the two
// windows of a pair coming from two arrays of two sample types: window A from frame t in the stack's own type T, window B -- at the SAME
// position, zero offset -- from the float32 workspace deform_warp_kernel filled with frame t+1 sampled along the predicted field
// (PivParams::warped).  u, v are the RESIDUAL against that field; launch_add_nodes adds the window's own node after the rescue pass.
// Arithmetic order: float32 stacks take prepare_pair's float path on both windows, i.e. the shifted kernel's order exactly (zero nodes
// on a float32 stack give that kernel's planes bit for bit); uint8 stacks keep the exact integer statistics for window A and take the
// float path for window B (its samples are multiples of 1 / 4096, no bytes), float64 stacks narrow A as the shifted kernel does.
#pragma once
#include "piv_fft_impl.h"

namespace lspiv {

// both windows -> xr = a'' (mean-offset, zero-clipped), xi = rho b'' (prepare_pair), A as T, B as float32
template <typename T, int N>
__device__ __forceinline__ void prepare_pair_mixed(const T* rowa, const float* rowb, float (&xr)[N], float (&xi)[N], bool want_nz, float thr,
                                                   bool nz_pos, float& scale, float& hi, bool& skip) {
  bool finite = true;
  int nza = Geo<N>::NN, nzb = Geo<N>::NN;
  float inv_a, rho;
  RowRaw<float, N> rb;
  rb.fetch(rowb);
  if constexpr (sizeof(T) == 1) {
    RowRaw<uint8_t, N> ra;
    ra.fetch(rowa);
    const RowStats sa = stats_u8<N>(ra, want_nz, nza);
    center_u8<N>(ra, sa.mean, 1.0f, xr);
    inv_a = sa.inv_std;
  } else {
    RowRaw<T, N> ra;
    ra.fetch(rowa);
    inv_a = load_center<N>(ra, xr, want_nz, nz_pos, nza, finite);
  }
  __builtin_amdgcn_sched_barrier(0);   // one window after the other (prepare_pair, SEQ)
  const float inv_b = load_center<N>(rb, xi, want_nz, nz_pos, nzb, finite);
  finish_pair<N>(inv_a, inv_b, rho, scale, hi);
#pragma unroll
  for (int j = 0; j < N; ++j) xi[j] *= rho;
  skip = !finite || (want_nz && below_threshold<N>(nza, nzb, thr));
}

// correlate_job's SINGLE path on the mixed pair: xr = the clipped plane (lane = row y, register = column x), mean = its DC bin
template <typename T, int N, bool WANT_NZ>
__device__ __forceinline__ void correlate_deform(const PivParams& p, const TileRef& t, float* buf, int lg, int partner_byte, float (&xr)[N],
                                                 float (&xi)[N], bool& skip, float& mean) {
  constexpr int H = N / 2;
  float Rr[H + 1], Ri[H + 1];
  float scale, hi;
  const uint32_t wrow = p.div_ncols.div(t.win);
  const uint32_t wcol = t.win - wrow * (uint32_t)p.n_cols;
  const int64_t off = ((int64_t)t.pair * p.H + (int64_t)(wrow * p.sy + lg)) * p.W + (int64_t)wcol * p.sx;
  prepare_pair_mixed<T, N>(static_cast<const T*>(p.frames) + off, p.warped + off, xr, xi, WANT_NZ, p.signal_threshold, p.nz_positive != 0,
                           scale, hi, skip);
  scale *= p.std_gain2;
  fft_n<false>(xr, xi);              // along x
  transpose2<N>(buf, lg, xr, xi);    // lane = kx, regs = y
  fft_n<false>(xr, xi);              // along y -> Z[ky][kx]
  cross_spectrum_half<N>(partner_byte, xr, xi, scale, Rr, Ri);
  __builtin_amdgcn_sched_barrier(0);
  // Q = R for ky <= N/2, the conjugate of the mirrored lane above: the imaginary plane comes out ~0 (correlate_job, SINGLE)
#pragma unroll
  for (int ky = 0; ky <= H; ++ky) { xr[ky] = Rr[ky]; xi[ky] = Ri[ky]; }
#pragma unroll
  for (int ky = 1; ky < H; ++ky) {
    xr[N - ky] = bperm_f(partner_byte, Rr[ky]);
    xi[N - ky] = -bperm_f(partner_byte, Ri[ky]);
  }
  mean = bperm_f(lane0_byte_of<N>(), xr[0]);
  __builtin_amdgcn_sched_barrier(0);
  fft_n<true>(xr, xi);                 // along ky
  transpose2<N>(buf, lg, xr, xi);      // lane = y, regs = kx
  fft_n<true>(xr, xi);                 // along kx
#pragma unroll
  for (int j = 0; j < N; ++j) xr[j] = __builtin_amdgcn_fmed3f(xr[j], 0.0f, hi);
}

// registers (ROCm 7.2, -Rpass-analysis=kernel-resource-usage, no scratch in any variant; uint8 | float32 | float64, over the four variants
// with / without signal score and planes): 16-point 53 - 63 | 57 - 59 | 57 - 59 VGPRs, 32-point 94 - 102 | 96 - 101 | 96 - 107, 64-point
// 187 - 208 | 198 - 210 | 198 - 210: inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 / 4 / 2 waves per SIMD) at every size
template <typename T, int N, bool PLANES, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_deform_kernel(PivParams p) {
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
  correlate_deform<T, N, WANT_NZ>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);

  float row_max, u, v;
  const uint32_t g = job;
  const float vmax = plane_max<N>(xr, row_max);
  find_peak<N, true>(buf, lg, xr, vmax, row_max, p, u, v, p.rescue_hdr && job_valid && !skip, g);
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
static hipError_t launch_deform_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_tiles + jobs_per_block - 1) / jobs_per_block;
  if (p.planes)
    hipLaunchKernelGGL((piv_fft_deform_kernel<T, N, true, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  else
    hipLaunchKernelGGL((piv_fft_deform_kernel<T, N, false, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_deform(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "deformation passes are 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_tiles == 0 || p.H < N || p.W < N || !p.warped || p.win_keep) return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_deform_t<uint8_t, N, true>(p, s) : launch_deform_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_deform_t<float, N, true>(p, s) : launch_deform_t<float, N, false>(p, s);
    case 2: return nz ? launch_deform_t<double, N, true>(p, s) : launch_deform_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lspiv
