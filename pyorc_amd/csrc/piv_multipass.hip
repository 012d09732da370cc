// Multi-pass PIV (gfx950): what runs BETWEEN the passes of a chain.
//
// A coarse pass predicts the displacement; the next, finer pass cuts its window of frame t+1 at an integer offset from that
// prediction (the shifted kernels, piv_fft_impl.h) and measures the residual.  Small kernels, one thread per (pair, window):
//   predict_shift_kernel   (u, v) of pass k on its grid -> int16 offsets (dy, dx) on the grid of pass k + 1.  After the first step
//                          (rint of every vector) it is exact integer arithmetic, so that a float64 reference on the host gives the
//                          very same integers: median of the rounded vectors over the 3 x 3 neighbourhood, bilinear interpolation
//                          between the coarse window centres with integer weights, one rounding division, the frame clamp.
//   clamp_shift_kernel     the offset field of a shifted ensemble handle -> its clamped values (window_shift), in place.
//   add_shift_kernel       u += clamped dx, v += clamped dy after the rescue pass: the kernels and the rescue pass write the residual.
// Window deformation passes (section 2f) run on the final grid after the chain:
//   predict_deform_kernel  (u, v) of a pass -> int32 nodes {v, u} in 1 / 128 px on the SAME grid: rint(64 x), then twice the 3 x 3 median
//                          (the code of predict_shift_kernel's median on the finer units).
//   deform_warp_kernel     frame t+1 of every pair of a batch sampled at the dense field of the pair's nodes (common.h, deform_sample)
//                          -> a float32 workspace the mixed-type kernels (piv_deform_impl.h) and the rescue pass cut window B from.
//   add_nodes_kernel       u += nodes.u / 128, v += nodes.v / 128 after the rescue pass.
// All of it in the kernels' native orientation (u = column shift, v = row shift, rows downward); the "v_sign" option is applied to
// the final result only.
#include <climits>

#include "common.h"
#include "piv_predict.h"

namespace lspiv {

namespace {

using namespace predict;

constexpr int MBLOCK = 256;

// per axis: the coarse interval [i0, i0 + 1] a fine centre falls into and its integer weights (w0, w1), w0 + w1 = s; constant
// extrapolation outside the outermost coarse centres; a one-entry axis has i0 = 0, w1 = 0
struct AxisW { int i0, i1, w0, w1; };
__device__ __forceinline__ AxisW axis_weights(int cf, int half_c, int s, int count) {
  AxisW a;
  const int d = cf - half_c;                                   // cf - cc[0]
  int i0 = d >= 0 ? d / s : -((-d + s - 1) / s);               // floor
  i0 = min(max(i0, 0), max(count - 2, 0));
  a.i0 = i0;
  a.i1 = min(i0 + 1, count - 1);
  a.w1 = count > 1 ? min(max(cf - (i0 * s + half_c), 0), s) : 0;
  a.w0 = s - a.w1;
  return a;
}

__global__ __launch_bounds__(MBLOCK) void predict_shift_kernel(const float* u, const float* v, uint32_t n_pairs, int H, int W, PassGrid cg,
                                                               PassGrid fg, int16_t* shift) {
  const uint32_t n_fine = (uint32_t)fg.n_rows * (uint32_t)fg.n_cols;
  const uint64_t g = (uint64_t)blockIdx.x * MBLOCK + threadIdx.x;
  if (g >= (uint64_t)n_pairs * n_fine) return;
  const uint32_t pair = (uint32_t)(g / n_fine), win = (uint32_t)(g - (uint64_t)pair * n_fine);
  const int r = (int)(win / (uint32_t)fg.n_cols), c = (int)(win - (uint32_t)r * (uint32_t)fg.n_cols);
  const int y0 = r * fg.sy, x0 = c * fg.sx;
  const AxisW ay = axis_weights(y0 + fg.wy / 2, cg.wy / 2, cg.sy, cg.n_rows);
  const AxisW ax = axis_weights(x0 + fg.wx / 2, cg.wx / 2, cg.sx, cg.n_cols);
  const size_t base = (size_t)pair * cg.n_rows * cg.n_cols;
  const float* pu = u + base;
  const float* pv = v + base;
  int64_t num_u = 0, num_v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int iy = e & 2 ? ay.i1 : ay.i0, ix = e & 1 ? ax.i1 : ax.i0;
    const int64_t w = (int64_t)(e & 2 ? ay.w1 : ay.w0) * (int64_t)(e & 1 ? ax.w1 : ax.w0);
    int mu = 0, mv = 0;
    if (w != 0) median2(pu, pv, cg.n_rows, cg.n_cols, iy, ix, mu, mv);
    num_u += w * mu;
    num_v += w * mv;
  }
  const int64_t den = 2 * (int64_t)cg.sy * (int64_t)cg.sx;           // the medians carry a factor 2
  const int64_t dx = floor_div(2 * num_u + den, 2 * den);           // round half up
  const int64_t dy = floor_div(2 * num_v + den, 2 * den);
  const int64_t cy = min(max(dy, (int64_t)-y0), (int64_t)(H - fg.wy - y0));   // the frame clamp of window_shift
  const int64_t cx = min(max(dx, (int64_t)-x0), (int64_t)(W - fg.wx - x0));
  shift[2 * g] = (int16_t)cy;
  shift[2 * g + 1] = (int16_t)cx;
}

__global__ __launch_bounds__(MBLOCK) void add_shift_kernel(PivParams p) {
  const uint32_t g = blockIdx.x * MBLOCK + threadIdx.x;
  if (g >= p.n_tiles) return;
  const uint32_t pair = p.div_nwin.div(g), win = g - pair * p.n_win;
  const uint32_t wrow = p.div_ncols.div(win), wcol = win - wrow * (uint32_t)p.n_cols;
  const WinShift ws = window_shift(p, g, wrow, wcol);
  if (ws.dx != 0) p.u[g] = p.u[g] + (float)ws.dx;   // (a zero offset leaves the residual's bits, the sign of a zero included)
  if (ws.dy != 0) p.v[g] = p.v[g] + (float)ws.dy;
}

// one thread per (pair, window): nodes[g] = {twice the median of rint(64 v), of rint(64 u)} over the valid 3 x 3 neighbours, 1 / 128 px
__global__ __launch_bounds__(MBLOCK) void predict_deform_kernel(const float* u, const float* v, uint32_t n_pairs, int n_rows, int n_cols,
                                                                int32_t* nodes) {
  const uint32_t n_win = (uint32_t)n_rows * (uint32_t)n_cols;
  const uint64_t g = (uint64_t)blockIdx.x * MBLOCK + threadIdx.x;
  if (g >= (uint64_t)n_pairs * n_win) return;
  const uint32_t pair = (uint32_t)(g / n_win), win = (uint32_t)(g - (uint64_t)pair * n_win);
  const int r = (int)(win / (uint32_t)n_cols), c = (int)(win - (uint32_t)r * (uint32_t)n_cols);
  const size_t base = (size_t)pair * n_win;
  int mu = 0, mv = 0;
  median2<true>(u + base, v + base, n_rows, n_cols, r, c, mu, mv);
  nodes[2 * g] = mv;
  nodes[2 * g + 1] = mu;
}

// one thread per pixel of the warped frames: block = 64 pixels of 4 rows (the lanes of a wave run along x: the field is smooth, so
// they read near-contiguous addresses, and the two node columns of an interval are the same words for most lanes -- L1 / L2 hits on a
// pair's few KB of nodes), blockIdx.z = the pair.  p.frames = frame 0 of the batch; pair k reads frame k + 1
constexpr int WARP_BX = 64, WARP_BY = 4;
template <typename T>
__global__ __launch_bounds__(WARP_BX * WARP_BY) void deform_warp_kernel(PivParams p, float* warped) {
  const int x = (int)(blockIdx.x * WARP_BX + threadIdx.x), y = (int)(blockIdx.y * WARP_BY + threadIdx.y);
  if (x >= p.W || y >= p.H) return;
  const uint32_t pair = blockIdx.z;
  const T* I = static_cast<const T*>(p.frames) + ((int64_t)pair + 1) * p.frame_elems;
  warped[(int64_t)pair * p.frame_elems + (int64_t)y * p.W + x] = deform_sample<T>(p, p.nodes + 2 * (size_t)pair * p.n_win, I, y, x);
}

__global__ __launch_bounds__(MBLOCK) void add_nodes_kernel(PivParams p) {
  const uint32_t g = blockIdx.x * MBLOCK + threadIdx.x;
  if (g >= p.n_tiles) return;
  p.v[g] = (float)p.nodes[2 * (size_t)g] * (1.0f / 128.0f) + p.v[g];       // (|node| < 2^23: the conversion and the scaling are exact)
  p.u[g] = (float)p.nodes[2 * (size_t)g + 1] * (1.0f / 128.0f) + p.u[g];
}

// shifted ensemble pass: the offset field of a handle (n_win x {dy, dx}, p.n_tiles = p.n_win) replaced by its clamped values -- through
// window_shift, so that what lspiv_ensemble_get_shift hands out is what the kernels use.  In place: a thread reads and writes its own entry.
__global__ __launch_bounds__(MBLOCK) void clamp_shift_kernel(PivParams p, int16_t* out) {
  const uint32_t g = blockIdx.x * MBLOCK + threadIdx.x;
  if (g >= p.n_win) return;
  const uint32_t wrow = p.div_ncols.div(g), wcol = g - wrow * (uint32_t)p.n_cols;
  const WinShift ws = window_shift(p, g, wrow, wcol);
  out[2 * (size_t)g] = (int16_t)ws.dy;
  out[2 * (size_t)g + 1] = (int16_t)ws.dx;
}

}  // namespace

hipError_t launch_clamp_shift(const PivParams& p, int16_t* out, hipStream_t s) {
  if (!p.shift || !out || p.n_win == 0) return hipSuccess;
  hipLaunchKernelGGL(clamp_shift_kernel, dim3((p.n_win + MBLOCK - 1) / MBLOCK), dim3(MBLOCK), 0, s, p, out);
  return hipGetLastError();
}

hipError_t launch_predict_shift(const float* u, const float* v, uint32_t n_pairs, int H, int W, const PassGrid& coarse, const PassGrid& fine,
                                int16_t* shift, hipStream_t s) {
  const uint64_t n = (uint64_t)n_pairs * (uint64_t)fine.n_rows * (uint64_t)fine.n_cols;
  if (n == 0) return hipSuccess;
  if (n >= (uint64_t)1 << 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predict_shift_kernel, dim3((uint32_t)((n + MBLOCK - 1) / MBLOCK)), dim3(MBLOCK), 0, s, u, v, n_pairs, H, W, coarse, fine, shift);
  return hipGetLastError();
}

hipError_t launch_predict_deform(const float* u, const float* v, uint32_t n_pairs, int n_rows, int n_cols, int32_t* nodes, hipStream_t s) {
  const uint64_t n = (uint64_t)n_pairs * (uint64_t)n_rows * (uint64_t)n_cols;
  if (n == 0) return hipSuccess;
  if (n >= (uint64_t)1 << 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predict_deform_kernel, dim3((uint32_t)((n + MBLOCK - 1) / MBLOCK)), dim3(MBLOCK), 0, s, u, v, n_pairs, n_rows, n_cols, nodes);
  return hipGetLastError();
}

hipError_t launch_deform_warp(const PivParams& p, int dtype, float* warped, hipStream_t s) {
  if (!p.nodes || !warped || p.H < 2 || p.W < 2 || p.n_pairs == 0 || p.n_pairs > 65535) return hipErrorInvalidValue;
  const dim3 grid((p.W + WARP_BX - 1) / WARP_BX, (p.H + WARP_BY - 1) / WARP_BY, p.n_pairs), block(WARP_BX, WARP_BY);
  if (grid.y > 65535) return hipErrorInvalidValue;
  switch (dtype) {
    case 0: hipLaunchKernelGGL(deform_warp_kernel<uint8_t>, grid, block, 0, s, p, warped); break;
    case 1: hipLaunchKernelGGL(deform_warp_kernel<float>, grid, block, 0, s, p, warped); break;
    case 2: hipLaunchKernelGGL(deform_warp_kernel<double>, grid, block, 0, s, p, warped); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_add_nodes(const PivParams& p, hipStream_t s) {
  if (!p.nodes || p.n_tiles == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(add_nodes_kernel, dim3((p.n_tiles + MBLOCK - 1) / MBLOCK), dim3(MBLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_add_shift(const PivParams& p, hipStream_t s) {
  if (!p.shift || p.n_tiles == 0) return hipSuccess;   // all-zero offsets: nothing to add
  hipLaunchKernelGGL(add_shift_kernel, dim3((p.n_tiles + MBLOCK - 1) / MBLOCK), dim3(MBLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace lspiv
