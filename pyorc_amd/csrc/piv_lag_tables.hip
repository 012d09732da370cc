// Per-window frame lag (gfx950): what runs AROUND the lag kernels of piv_lag_impl.h.  Small kernels, one
// thread per (pair, window), in the kernels' native orientation (u = column shift, v = row shift, rows downward):
//   lag_fill_kernel     the table of a uniform lag, of a per-window lag or of a caller's table, every entry clipped to 1 .. 16 and to the
//                       end of the stack: pair t of a launch that may read n_frames frames gets at most n_frames - 1 - t.  The PIV
//                       kernel and the rescue pass read the table only after this kernel or the predictor wrote it, so no table can make
//                       them read past the stack.
//   lag_predict_kernel  (u, v) of a lag-1 pass -> (k, dy, dx) per window: rint(64 x) of every vector, twice the 3 x 3 median (the
//                       predictors' median2, piv_predict.h) in 1 / 128 px, k = the largest lag that keeps the larger component at or
//                       below the target, the offset = the median times k rounded half up, the frame clamp of window_shift.  Exact
//                       integers after the first rounding (everything fits int32; the divisions are done on int64 for the floor).
//   lag_divide_kernel   after the rescue pass: u = (residual + clamped dx) / k, v likewise -- the float32 sum of launch_add_shift (a zero
//                       offset leaves the residual's bits), then ONE correctly rounded float32 division by float(k); k = 1 leaves the
//                       bits, a NaN stays NaN.  It also hands out the clamped offsets it added.
#include "common.h"
#include "piv_predict.h"

namespace lspiv {

namespace {

using namespace predict;

constexpr int LBLOCK = 256;

// the largest lag pair t may use: the frames left after it, at most kMaxLag; at least 1 (t <= n_frames - 2 for every pair of a launch)
__device__ __forceinline__ int lag_limit(int64_t n_frames, uint32_t pair) {
  return (int)min((int64_t)kMaxLag, max((int64_t)1, n_frames - 1 - (int64_t)pair));
}

__global__ __launch_bounds__(LBLOCK) void lag_fill_kernel(int form, int k, const uint8_t* src, uint32_t n_pairs, uint32_t n_win, int64_t n_frames,
                                                          uint8_t* lag) {
  const uint64_t g = (uint64_t)blockIdx.x * LBLOCK + threadIdx.x;
  if (g >= (uint64_t)n_pairs * n_win) return;
  const uint32_t pair = (uint32_t)(g / n_win), win = (uint32_t)(g - (uint64_t)pair * n_win);
  const int want = form == 0 ? k : form == 1 ? (int)src[win] : (int)src[g];
  lag[g] = (uint8_t)min(max(want, 1), lag_limit(n_frames, pair));
}

__global__ __launch_bounds__(LBLOCK) void lag_predict_kernel(const float* u, const float* v, uint32_t n_pairs, int64_t n_frames, int H, int W,
                                                             PassGrid pg, int k_max, int t128, uint8_t* lag, int16_t* shift) {
  const uint32_t n_win = (uint32_t)pg.n_rows * (uint32_t)pg.n_cols;
  const uint64_t g = (uint64_t)blockIdx.x * LBLOCK + threadIdx.x;
  if (g >= (uint64_t)n_pairs * n_win) return;
  const uint32_t pair = (uint32_t)(g / n_win), win = (uint32_t)(g - (uint64_t)pair * n_win);
  const int r = (int)(win / (uint32_t)pg.n_cols), c = (int)(win - (uint32_t)r * (uint32_t)pg.n_cols);
  const size_t base = (size_t)pair * n_win;
  int m2u = 0, m2v = 0;
  median2<true>(u + base, v + base, pg.n_rows, pg.n_cols, r, c, m2u, m2v);   // 1 / 128 px, |m2| <= 2 * 32767 * 64
  const int mag = max(abs(m2u), abs(m2v));
  int k = min(max(t128 / max(mag, 1), 1), k_max);                            // (both operands positive: the quotient is the floor)
  k = min(k, lag_limit(n_frames, pair));
  const int64_t dx = floor_div((int64_t)k * m2u + 64, 128);                  // round half up
  const int64_t dy = floor_div((int64_t)k * m2v + 64, 128);
  const int y0 = r * pg.sy, x0 = c * pg.sx;
  const int64_t cy = min(max(dy, (int64_t)-y0), (int64_t)(H - pg.wy - y0));   // the frame clamp of window_shift
  const int64_t cx = min(max(dx, (int64_t)-x0), (int64_t)(W - pg.wx - x0));
  lag[g] = (uint8_t)k;
  shift[2 * g] = (int16_t)cy;
  shift[2 * g + 1] = (int16_t)cx;
}

__global__ __launch_bounds__(LBLOCK) void lag_divide_kernel(PivParams p, int16_t* shift_out) {
  const uint32_t g = blockIdx.x * LBLOCK + threadIdx.x;
  if (g >= p.n_tiles) return;
  const uint32_t pair = p.div_nwin.div(g), win = g - pair * p.n_win;
  const uint32_t wrow = p.div_ncols.div(win), wcol = win - wrow * (uint32_t)p.n_cols;
  const WinShift ws = window_shift(p, g, wrow, wcol);
  float fu = p.u[g], fv = p.v[g];
  if (ws.dx != 0) fu = fu + (float)ws.dx;   // (launch_add_shift's step: a zero offset leaves the residual's bits)
  if (ws.dy != 0) fv = fv + (float)ws.dy;
  const float k = (float)p.lag[g];
  p.u[g] = __fdiv_rn(fu, k);
  p.v[g] = __fdiv_rn(fv, k);
  if (shift_out) {   // what the kernel and the rescue pass used (shift_out may be p.shift itself: a thread reads and writes its own entry)
    shift_out[2 * (size_t)g] = (int16_t)ws.dy;
    shift_out[2 * (size_t)g + 1] = (int16_t)ws.dx;
  }
}

}  // namespace

hipError_t launch_lag_fill(int form, int k, const uint8_t* src, uint32_t n_pairs, uint32_t n_win, int64_t n_frames, uint8_t* lag, hipStream_t s) {
  const uint64_t n = (uint64_t)n_pairs * n_win;
  if (n == 0) return hipSuccess;
  if (n >= (uint64_t)1 << 31 || !lag || form < 0 || form > 2 || (form != 0 && !src) || n_frames < (int64_t)n_pairs + 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lag_fill_kernel, dim3((uint32_t)((n + LBLOCK - 1) / LBLOCK)), dim3(LBLOCK), 0, s, form, k, src, n_pairs, n_win, n_frames, lag);
  return hipGetLastError();
}

hipError_t launch_lag_predict(const float* u, const float* v, uint32_t n_pairs, int64_t n_frames, int H, int W, const PassGrid& g, int k_max,
                              int t128, uint8_t* lag, int16_t* shift, hipStream_t s) {
  const uint64_t n = (uint64_t)n_pairs * (uint64_t)g.n_rows * (uint64_t)g.n_cols;
  if (n == 0) return hipSuccess;
  if (n >= (uint64_t)1 << 31 || k_max < 1 || k_max > kMaxLag || t128 < 1 || n_frames < (int64_t)n_pairs + 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lag_predict_kernel, dim3((uint32_t)((n + LBLOCK - 1) / LBLOCK)), dim3(LBLOCK), 0, s, u, v, n_pairs, n_frames, H, W, g, k_max,
                     t128, lag, shift);
  return hipGetLastError();
}

hipError_t launch_lag_divide(const PivParams& p, int16_t* shift_out, hipStream_t s) {
  if (!p.lag || p.n_tiles == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lag_divide_kernel, dim3((p.n_tiles + LBLOCK - 1) / LBLOCK), dim3(LBLOCK), 0, s, p, shift_out);
  return hipGetLastError();
}

}  // namespace lspiv
