// Per-window frame lag for the per-pair PIV kernels (gfx950): window A of frame t against the window of frame
// t + k at a per-window integer offset, k = p.lag[pair * n_win + window] in 1 .. 16 -- multi-frame PIV for slow flow: a displacement of
// a fraction of a pixel per frame interval is measured over k intervals and divided by k (launch_lag_divide, piv_lag_tables.hip).
//
// The job is the shifted kernel's (piv_fft_impl.h: one window per job, one plane per inverse transform, XCD-aware block order,
// correlate_job<..., SHIFT> -> plane_max -> find_peak with its rescue records); the one difference is the address of window B's rows,
//   off + k * frame_elems + dy * W + dx      instead of      off + frame_elems + dy * W + dx
// (correlate_job, LAG): one byte load and one 64-bit multiply-add per row pointer.  With k = 1 everywhere the kernel computes the
// shifted kernel's bits.  The table is ALWAYS there: the fill kernel writes the clipped lags of a uniform or per-window lag, the
// predictor those of the adaptive form, so the PIV kernel has one form and reads no frame past the stack whatever the caller asked for.
// u, v are the RESIDUAL of the frame pair (t, t + k), as for the shifted kernel; the rescue pass steps p.lag[g] frames (piv_rescue.hip).
// registers (ROCm 7.2, no scratch in any of the 36 variants; uint8 | float32 | float64, over the four variants with / without signal score
// and planes; VGPRs, then waves per SIMD): 16-point 52 - 55 | 57 - 69 | 61 - 74 (8 | 7 - 8 | 6 - 8), 32-point 92 - 93 | 96 - 100 | 110 - 112
// (5 | 4 - 5 | 4), 64-point 184 - 186 | 184 - 206 | 205 - 208 (2 | 2 | 2): the shifted kernel's counts variant by variant, but for 2 VGPRs
// more in one float64 variant at 32 points, and inside the bounds of piv_fft_kernel (kWavesPerSimd: 4 at 16 points, 4 | 4 | 2 at 32, 2 at
// 64) at every size.  `python tools/kres.py pyorc_amd/csrc/piv_lag32.hip lag_kernel` prints the table.
#pragma once
#include "piv_fft_impl.h"

namespace lspiv {

// (the body is piv_fft_shift_kernel's, copied, with LAG set in correlate_job: one shared __device__ body for the two kernels moved 92
// instruction lines of the 32-point shifted unit, and the existing kernels keep their instructions -- a fix there belongs here too)
template <typename T, int N, bool PLANES, bool WANT_NZ>
__global__ __launch_bounds__(BLOCK, (kWavesPerSimd<T, N>)) void piv_fft_lag_kernel(PivParams p) {
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
  correlate_job<T, N, WANT_NZ, false, false, true, false, true>(p, t, buf, lg, partner_byte, xr, xi, skip, mean);

  float row_max, u, v;
  const uint32_t g = job;
  const float vmax = plane_max<N>(xr, row_max);
  find_peak<N>(buf, lg, xr, vmax, row_max, p, u, v, p.rescue_hdr && job_valid && !skip[0], g);
  float cm = vmax, sn = vmax * __builtin_amdgcn_rcpf(mean[0]);
  if (skip[0]) u = v = cm = sn = __builtin_nanf("");
  if (job_valid && lg == 0) {
    p.u[g] = u; p.v[g] = v; p.cmax[g] = cm; p.s2n[g] = sn;
  }
  if constexpr (PLANES) {
    if (job_valid) store_plane_rows<N>(p.planes + (size_t)g * G::NN, lg, xr, skip[0]);
  }
}

template <typename T, int N, bool WANT_NZ>
static hipError_t launch_lag_t(const PivParams& p, hipStream_t s) {
  using G = Geo<N>;
  constexpr uint32_t jobs_per_block = WAVES_PER_BLOCK * G::GROUPS;
  const uint32_t blocks = (p.n_tiles + jobs_per_block - 1) / jobs_per_block;
  if (p.planes)
    hipLaunchKernelGGL((piv_fft_lag_kernel<T, N, true, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  else
    hipLaunchKernelGGL((piv_fft_lag_kernel<T, N, false, WANT_NZ>), dim3(blocks), dim3(BLOCK), G::LDS_BYTES, s, p);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_lag(const PivParams& p, int dtype, hipStream_t s) {
  static_assert(Geo<N>::FULL && N % 16 == 0, "lagged passes are 16, 32 or 64 px");
  if (p.wy != N || p.wx != N || p.nw != 0 || p.n_tiles == 0 || p.H < N || p.W < N || !p.lag) return hipErrorInvalidValue;
  const bool nz = p.signal_threshold >= 0.0f;
  switch (dtype) {
    case 0: return nz ? launch_lag_t<uint8_t, N, true>(p, s) : launch_lag_t<uint8_t, N, false>(p, s);
    case 1: return nz ? launch_lag_t<float, N, true>(p, s) : launch_lag_t<float, N, false>(p, s);
    case 2: return nz ? launch_lag_t<double, N, true>(p, s) : launch_lag_t<double, N, false>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lspiv
