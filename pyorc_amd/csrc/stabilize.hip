// Frame stabilisation: what stands between a camera that moves (handheld, drone, a pole in the wind) and the fixed-camera chain
// normalize -> project -> get_piv.  The vectors come from the masked per-pair PIV kernels under a static mask of the banks, unchanged;
// this file holds the three kernels behind them (include/lspiv.h):
//
//   stabilize_fit_kernel    one block per pair: the three rounds of the robust least-squares fit in ONE launch.  Twelve float64 sums per
//                           round, each lane over the windows tid, tid + 256, ... in that order, then a fixed LDS tree: the reduction order
//                           depends on the grid alone.  Lane 0 solves the normal equations in closed form (no arrays: no scratch) and
//                           hands the coefficients to the block for the next round's selection.
//   stabilize_chain_kernel  one wave: the pairwise transforms are staged 64 at a time into LDS by all lanes, lane 0 multiplies them onto
//                           the pose sequentially.  Stream-ordered behind the fit: the chain needs no host round trip.
//   warp_affine_kernel<T>   the hot path.  One wave = 64 destination pixels of one row = one block of the fixed-point walk (x1 = lane).
//                           Camera shake is close to the identity, so the 64 sources of a wave are 64 consecutive pixels of a source row
//                           (give or take a row change along the way): each of the four neighbour loads of a wave is one or two cache
//                           lines, fully used, and the second row's lines are the first row's of the wave below -- L1 / L2 hits.  Direct
//                           neighbour loads, no LDS staging: a wave-private staged chunk would save vector-memory instructions (4 per
//                           pixel here), not HBM bytes, at the price of a row-change case analysis per wave; the rates of DESIGN.md
//                           section 3.4j are those of this form.
//
// The arithmetic is the float64 numpy reference's (tests/stabilize_ref.py) operation for operation where bits are promised (chain, walk,
// blend): contraction is off for the whole file (the pragma below), so every product and every sum written here is one correctly rounded
// operation and the object code holds no fused multiply-add.  (__dmul_rn / __dadd_rn would NOT do: they are inline functions of a
// header compiled under the default contraction, and the backend fuses them like any other pair.)
#include "stabilize.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace lspiv {

namespace {

constexpr int kFitBlock = 256;
constexpr int kFitSums = 12;
constexpr double kSingularRtol = 1e-9;   // tests/stabilize_ref.py, SINGULAR_RTOL

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for +-inf and NaN

// The closed forms of tests/stabilize_ref.py, _solve: (a, b, c, d, e, f) of u = a x + b y + c, v = d x + e y + f.  false: too few vectors
// or a singular normal matrix (the determinant against kSingularRtol times the product of the diagonal).
__device__ __forceinline__ bool solve_model(int model, int min_vectors, double N, double Sx, double Sy, double Sxx, double Sxy, double Syy,
                                            double Su, double Sv, double Sxu, double Syu, double Sxv, double Syv, double (&co)[6]) {
  if (!(N >= (double)(min_vectors > 1 ? min_vectors : 1))) return false;
  if (model == 0) {
    co[0] = 0.0; co[1] = 0.0; co[2] = Su / N; co[3] = 0.0; co[4] = 0.0; co[5] = Sv / N;
    return true;
  }
  if (model == 1) {   // u = a x - b y + c, v = b x + a y + d
    const double S2 = Sxx + Syy;
    const double D = N * S2 - Sx * Sx - Sy * Sy;
    if (!(D > kSingularRtol * (N * S2))) return false;
    const double a = (N * (Sxu + Syv) - Sx * Su - Sy * Sv) / D;
    const double b = (N * (Sxv - Syu) - Sx * Sv + Sy * Su) / D;
    co[0] = a; co[1] = -b; co[2] = (Su - a * Sx + b * Sy) / N;
    co[3] = b; co[4] = a;  co[5] = (Sv - b * Sx - a * Sy) / N;
    return true;
  }
  // the adjugate of the symmetric normal matrix [[Sxx Sxy Sx] [Sxy Syy Sy] [Sx Sy N]]
  const double c00 = Syy * N - Sy * Sy, c01 = Sx * Sy - Sxy * N, c02 = Sxy * Sy - Syy * Sx;
  const double c11 = Sxx * N - Sx * Sx, c12 = Sxy * Sx - Sxx * Sy, c22 = Sxx * Syy - Sxy * Sxy;
  const double det = Sxx * c00 + Sxy * c01 + Sx * c02;
  if (!(det > kSingularRtol * (N * Sxx * Syy))) return false;
  co[0] = (c00 * Sxu + c01 * Syu + c02 * Su) / det; co[1] = (c01 * Sxu + c11 * Syu + c12 * Su) / det; co[2] = (c02 * Sxu + c12 * Syu + c22 * Su) / det;
  co[3] = (c00 * Sxv + c01 * Syv + c02 * Sv) / det; co[4] = (c01 * Sxv + c11 * Syv + c12 * Sv) / det; co[5] = (c02 * Sxv + c12 * Syv + c22 * Sv) / det;
  return true;
}

__global__ __launch_bounds__(kFitBlock) void stabilize_fit_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  StabilizeFitParams p, double* __restrict__ P, int32_t* __restrict__ n_used) {
  __shared__ double red[kFitSums][kFitBlock];
  __shared__ double coef[8];   // the round's six coefficients, [6] = 1 solved / 0 not, [7] = the round's vector count
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x;
  const int n_win = p.rows * p.cols;
  const float* up = u + pair * n_win;
  const float* vp = v + pair * n_win;
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0, e = 0.0, f = 0.0, count = 0.0;
  bool solved = true;
  for (int rnd = 0; rnd < 3 && solved; ++rnd) {
    const double lim = rnd == 1 ? p.reject0 : p.reject1, lim2 = lim * lim;
    double s[kFitSums];
#pragma unroll
    for (int k = 0; k < kFitSums; ++k) s[k] = 0.0;
    for (int i = tid; i < n_win; i += kFitBlock) {
      const int r = i / p.cols, cc = i - r * p.cols;
      const double uu = (double)up[i], vv = (double)vp[i];
      const double x = p.x0 + (double)cc * p.dx, y = p.y0 + (double)r * p.dy;   // half-integers: exact
      bool sel = finite_d(uu) && finite_d(vv);
      if (rnd > 0) {   // within the round's limit of the previous round's prediction (a NaN residual is not)
        const double du = uu - ((a * x + b * y) + c), dv = vv - ((d * x + e * y) + f);
        sel = sel && (du * du + dv * dv <= lim2);
      }
      const double w = sel ? 1.0 : 0.0, xs = sel ? x : 0.0, ys = sel ? y : 0.0, us = sel ? uu : 0.0, vs = sel ? vv : 0.0;
      s[0] += w;        s[1] += xs;       s[2] += ys;
      s[3] += xs * xs;  s[4] += xs * ys;  s[5] += ys * ys;
      s[6] += us;       s[7] += vs;
      s[8] += xs * us;  s[9] += ys * us;  s[10] += xs * vs;  s[11] += ys * vs;
    }
#pragma unroll
    for (int k = 0; k < kFitSums; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int h = kFitBlock / 2; h > 0; h >>= 1) {
      if (tid < h) {
#pragma unroll
        for (int k = 0; k < kFitSums; ++k) red[k][tid] += red[k][tid + h];
      }
      __syncthreads();
    }
    if (tid == 0) {
      double co[6];
      const bool ok = solve_model(p.model, p.min_vectors, red[0][0], red[1][0], red[2][0], red[3][0], red[4][0], red[5][0], red[6][0],
                                  red[7][0], red[8][0], red[9][0], red[10][0], red[11][0], co);
      coef[0] = ok ? co[0] : 0.0; coef[1] = ok ? co[1] : 0.0; coef[2] = ok ? co[2] : 0.0;
      coef[3] = ok ? co[3] : 0.0; coef[4] = ok ? co[4] : 0.0; coef[5] = ok ? co[5] : 0.0;
      coef[6] = ok ? 1.0 : 0.0;
      coef[7] = red[0][0];
    }
    __syncthreads();
    a = coef[0]; b = coef[1]; c = coef[2]; d = coef[3]; e = coef[4]; f = coef[5];
    solved = coef[6] != 0.0;
    count = coef[7];
    __syncthreads();   // coef and red are rewritten by the next round
  }
  if (tid == 0) {
    double* out = P + pair * 6;
    if (solved) {   // back from frame-centred coordinates
      out[0] = 1.0 + a; out[1] = b;       out[2] = (c - a * p.cx) - b * p.cy;
      out[3] = d;       out[4] = 1.0 + e; out[5] = (f - d * p.cx) - e * p.cy;
      n_used[pair] = (int32_t)count;
    } else {
      out[0] = 1.0; out[1] = 0.0; out[2] = 0.0;
      out[3] = 0.0; out[4] = 1.0; out[5] = 0.0;
      n_used[pair] = 0;
    }
  }
}

// (p0 c0 + p1 c1) + p2 c2, every product and sum rounded on its own (contraction is off)
__device__ __forceinline__ double dot3_rn(double p0, double p1, double p2, double c0, double c1, double c2) {
  return (p0 * c0 + p1 * c1) + p2 * c2;
}

__global__ __launch_bounds__(64) void stabilize_chain_kernel(const double* __restrict__ P, int64_t pairs, const double* __restrict__ carry_in,
                                                             double* __restrict__ A, double* __restrict__ carry_out) {
  __shared__ double stage[64 * 6];
  const int lane = threadIdx.x;
  // the pose [C; 0 0 1] lives in lane 0's registers
  double c00 = 1.0, c01 = 0.0, c02 = 0.0, c10 = 0.0, c11 = 1.0, c12 = 0.0;
  const double c20 = 0.0, c21 = 0.0, c22 = 1.0;
  if (carry_in != nullptr) { c00 = carry_in[0]; c01 = carry_in[1]; c02 = carry_in[2]; c10 = carry_in[3]; c11 = carry_in[4]; c12 = carry_in[5]; }
  if (lane == 0) { A[0] = c00; A[1] = c01; A[2] = c02; A[3] = c10; A[4] = c11; A[5] = c12; }
  for (int64_t base = 0; base < pairs; base += 64) {
    const int n = (int)(pairs - base < 64 ? pairs - base : 64);
    for (int i = lane; i < n * 6; i += 64) stage[i] = P[base * 6 + i];
    __syncthreads();
    if (lane == 0) {
      for (int k = 0; k < n; ++k) {
        const double p00 = stage[k * 6 + 0], p01 = stage[k * 6 + 1], p02 = stage[k * 6 + 2];
        const double p10 = stage[k * 6 + 3], p11 = stage[k * 6 + 4], p12 = stage[k * 6 + 5];
        const double n00 = dot3_rn(p00, p01, p02, c00, c10, c20), n01 = dot3_rn(p00, p01, p02, c01, c11, c21), n02 = dot3_rn(p00, p01, p02, c02, c12, c22);
        const double n10 = dot3_rn(p10, p11, p12, c00, c10, c20), n11 = dot3_rn(p10, p11, p12, c01, c11, c21), n12 = dot3_rn(p10, p11, p12, c02, c12, c22);
        // (the third row of [P; 0 0 1] [C; 0 0 1] is 0 0 1 again for finite entries; it is kept literal)
        c00 = n00; c01 = n01; c02 = n02; c10 = n10; c11 = n11; c12 = n12;
        double* a = A + (base + k + 1) * 6;
        a[0] = c00; a[1] = c01; a[2] = c02; a[3] = c10; a[4] = c11; a[5] = c12;
      }
    }
    __syncthreads();   // the stage is refilled
  }
  if (lane == 0 && carry_out != nullptr) {
    carry_out[0] = c00; carry_out[1] = c01; carry_out[2] = c02; carry_out[3] = c10; carry_out[4] = c11; carry_out[5] = c12;
  }
}

// the walk's fixed-point coordinate: NaN -> 0, clipped to the int32 range, round half to even
__device__ __forceinline__ int fixed_coord(double f) {
  f = f != f ? 0.0 : f;
  f = fmin(fmax(f, -2147483648.0), 2147483647.0);
  return (int)rint(f);
}

constexpr int kWarpRows = 4;   // waves (rows) per block

template <typename T>
__global__ __launch_bounds__(64 * kWarpRows) void warp_affine_kernel(const T* __restrict__ frames, int64_t n_frames, int H, int W,
                                                                      const double* __restrict__ A, T* __restrict__ out) {
  const int x1 = threadIdx.x, xb = blockIdx.x * 64, x = xb + x1;
  const int y = blockIdx.y * kWarpRows + threadIdx.y;
  if (x >= W || y >= H) return;
  const int64_t frame_elems = (int64_t)H * W;
  for (int64_t t = blockIdx.z; t < n_frames; t += gridDim.z) {
    const double* a = A + t * 6;   // uniform over the block: scalar loads
    const double dxb = (double)xb, dy = (double)y, dx1 = (double)x1;
    const double X0 = (a[0] * dxb + a[1] * dy) + a[2];
    const double Y0 = (a[3] * dxb + a[4] * dy) + a[5];
    const int X = fixed_coord((X0 + a[0] * dx1) * 32.0);
    const int Y = fixed_coord((Y0 + a[3] * dx1) * 32.0);
    const int ix = X >> 5, iy = Y >> 5, fx = X & 31, fy = Y & 31;
    // a neighbour outside the frame counts as 0 and is never read (ix + 1, iy + 1 cannot overflow: |X >> 5| <= 2^26)
    const bool xl = ix >= 0 && ix < W, xr = ix + 1 >= 0 && ix + 1 < W, yt = iy >= 0 && iy < H, yb = iy + 1 >= 0 && iy + 1 < H;
    const T* img = frames + t * frame_elems;
    const int64_t base = (int64_t)iy * W + ix;
    // (one load per neighbour: joining a row's two into one 2-pixel load, as project.hip's remap does, measured 1.38 against 1.21 ms per
    // 201 1080p uint8 frames and no change for float32 -- the kernel is bound by its arithmetic, not by its loads)
    const T p00 = (xl && yt) ? img[base] : (T)0, p01 = (xr && yt) ? img[base + 1] : (T)0;
    const T p10 = (xl && yb) ? img[base + W] : (T)0, p11 = (xr && yb) ? img[base + W + 1] : (T)0;
    T* dst = out + t * frame_elems + (int64_t)y * W + x;
    if constexpr (sizeof(T) == 1) {
      const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
      const int acc = (int)p00 * w00 + (int)p01 * w01 + (int)p10 * w10 + (int)p11 * w11;
      *dst = (T)((acc + (1 << 14)) >> 15);
    } else {
      const float wa = (float)fx / 32.0f, wb = (float)fy / 32.0f;
      const float w00 = (1.0f - wa) * (1.0f - wb), w01 = wa * (1.0f - wb), w10 = (1.0f - wa) * wb, w11 = wa * wb;
      *dst = ((p00 * w00 + p01 * w01) + p10 * w10) + p11 * w11;   // left to right, no contraction (a weight of 0 still meets its sample: 0 * NaN)
    }
  }
}

}  // namespace

hipError_t launch_stabilize_fit(const float* u, const float* v, int64_t pairs, const StabilizeFitParams& p, double* P, int32_t* n_used,
                                hipStream_t s) {
  if (pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(stabilize_fit_kernel, dim3((unsigned)pairs), dim3(kFitBlock), 0, s, u, v, p, P, n_used);
  return hipGetLastError();
}

hipError_t launch_stabilize_chain(const double* P, int64_t pairs, const double* carry_in, double* A, double* carry_out, hipStream_t s) {
  hipLaunchKernelGGL(stabilize_chain_kernel, dim3(1), dim3(64), 0, s, P, pairs, carry_in, A, carry_out);
  return hipGetLastError();
}

hipError_t launch_warp_affine(const void* frames, int dtype, int64_t T, int H, int W, const double* A, void* out, hipStream_t s) {
  if (T == 0) return hipSuccess;
  const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + kWarpRows - 1) / kWarpRows), (unsigned)std::min<int64_t>(T, 65535));
  const dim3 block(64, kWarpRows);
  if (dtype == 0)
    hipLaunchKernelGGL(warp_affine_kernel<uint8_t>, grid, block, 0, s, (const uint8_t*)frames, T, H, W, A, (uint8_t*)out);
  else
    hipLaunchKernelGGL(warp_affine_kernel<float>, grid, block, 0, s, (const float*)frames, T, H, W, A, (float*)out);
  return hipGetLastError();
}

}  // namespace lspiv
