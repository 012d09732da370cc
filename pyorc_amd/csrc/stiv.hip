// Space-time image velocimetry (STIV; Fujita et al.): the brightness along a short search line laid along the flow, sampled in every
// frame and stacked into a space-time image (STI), carries the speed along the line as the orientation of its streaks.  Two kernels
// (include/lspiv.h):
//
//   sti_gather_kernel<T>       the hot path.  The grid runs over blocks of 256 sample points x groups of kGatherFrames frames; the
//                              points are numbered line after line, so the lanes of a wave are consecutive samples of one line (two
//                              lines where a line ends inside the wave): the four neighbour loads of a wave land on neighbouring
//                              addresses of two frame rows, and its store is one row segment of sti[s, t, :].  A lane reads its table
//                              entry (element offset of the upper left neighbour, float32 fractions -- prepared once per call by the
//                              host) once and keeps it over its frames; the 4 x kGatherFrames loads of a group are issued before the
//                              first blend, because the kernel is a request-pattern problem (a few cache lines per line and frame, far
//                              apart), not a bandwidth one.
//   sti_orientation_kernel<k>  one block per (line, window).  Lanes over the columns (samples along the line) in strips of 256; the rows
//                              (frames) stream through a register ring of 2k + 3 horizontally filtered rows per lane.  A lane reads the
//                              2k + 3 samples of its stencil row itself: the neighbours' are the same cache lines (L1 hits after the
//                              first lane's miss), so neither LDS staging with a barrier per row nor a cross-lane exchange of float64
//                              pairs is needed and the waves of a block run free of each other (DESIGN.md section 3.4k says what was
//                              and what was not measured).  The column means of the detrending are summed with t ascending by one lane
//                              per column and handed over in LDS once per strip.  Three float64 sums per lane in row order, one fixed
//                              LDS tree, the closed form in lane 0: the bits depend on the shape alone.
//
// The blend is tests/stiv_ref.py's operation for operation (bits are promised): contraction is off for the whole file, as in
// stabilize.hip, so every product and sum written here is one correctly rounded operation.
#include "stiv.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace lspiv {

namespace {

constexpr int kGatherBlock = 256;
constexpr int kGatherFrames = 4;   // frames per lane and trip: 16 loads in flight
constexpr int kOriBlock = 256;

template <typename T>
__global__ __launch_bounds__(kGatherBlock) void sti_gather_kernel(const T* __restrict__ frames, int64_t n_frames, int64_t frame_elems, int W,
                                                                   StiTable table, int64_t n_points, int L, float* __restrict__ sti,
                                                                   int64_t t_offset, int64_t T_total) {
  const int64_t p = (int64_t)blockIdx.x * kGatherBlock + threadIdx.x;
  if (p >= n_points) return;
  const int64_t line = p / L;
  const int i = (int)(p - line * L);
  // (the entry point has checked every point; the clamp keeps the four loads inside the frame whatever the table holds)
  const int64_t o = std::min<int64_t>(std::max<int64_t>(table.offset[p], 0), frame_elems - W - 2);
  const float fx = table.fx[p], fy = table.fy[p];
  float* dst = sti + ((line * T_total + t_offset) * L + i);
  for (int64_t t0 = (int64_t)blockIdx.y * kGatherFrames; t0 < n_frames; t0 += (int64_t)gridDim.y * kGatherFrames) {
    T a[kGatherFrames], b[kGatherFrames], c[kGatherFrames], d[kGatherFrames];
#pragma unroll
    for (int k = 0; k < kGatherFrames; ++k) {   // a trip's last frames may repeat frame n_frames - 1: loaded, not stored
      const T* img = frames + std::min<int64_t>(t0 + k, n_frames - 1) * frame_elems + o;
      a[k] = img[0]; b[k] = img[1]; c[k] = img[W]; d[k] = img[W + 1];
    }
#pragma unroll
    for (int k = 0; k < kGatherFrames; ++k) {
      const float fa = (float)a[k], fb = (float)b[k], fc = (float)c[k], fd = (float)d[k];
      const float top = fa + fx * (fb - fa);
      const float bot = fc + fx * (fd - fc);
      if (t0 + k < n_frames) dst[(t0 + k) * L] = top + fy * (bot - top);
    }
  }
}

// The integer taps of smooth = K (include/lspiv.h): b = the binomial row of order 2K + 2, dx = [-1, 0, 1] * the binomial row of order 2K,
// both 2K + 3 long; Gx = dx(i) (x) b(t), Gt = b(i) (x) dx(t), applied as correlations (tap j meets sample i + j - (K + 1)).
constexpr double binomial(int m, int j) {
  if (j < 0 || j > m) return 0.0;
  double c = 1.0;
  for (int q = 0; q < j; ++q) c = c * (double)(m - q) / (double)(q + 1);
  return c;
}
template <int K>
struct StiTaps {
  static constexpr int N = 2 * K + 3;
  static constexpr double b(int j) { return binomial(2 * K + 2, j); }
  static constexpr double dx(int j) { return binomial(2 * K, j - 2) - binomial(2 * K, j); }
};

template <int K>
__global__ __launch_bounds__(kOriBlock) void sti_orientation_kernel(const float* __restrict__ sti, int64_t T, int L, int64_t Tw, int64_t stride,
                                                                    int64_t n_win, int detrend, double* __restrict__ tensor,
                                                                    double* __restrict__ slope, double* __restrict__ coherency) {
  using Taps = StiTaps<K>;
  constexpr int R = K + 1, N = Taps::N;
  __shared__ double mean[kOriBlock + 2 * (kStiMaxSmooth + 1)];
  __shared__ double red[3][kOriBlock];
  const int tid = threadIdx.x;
  const int64_t line = blockIdx.x / n_win, win = blockIdx.x - line * n_win;
  const float* img = sti + (line * T + win * stride) * L;
  const int n_out = L - 2 * R;   // columns whose whole stencil lies inside the line
  double jxx = 0.0, jtt = 0.0, jxt = 0.0;
  for (int c0 = 0; c0 < n_out; c0 += kOriBlock) {
    // the means of the strip's columns c0 .. c0 + kOriBlock + 2R - 1 (0 without detrending: x - 0 is x)
    const int n_cols = std::min(kOriBlock + 2 * R, L - c0);
    for (int j = tid; j < n_cols; j += kOriBlock) {
      double m = 0.0;
      if (detrend) {
        const float* col = img + c0 + j;
        double sum = 0.0;
#pragma unroll 8
        for (int64_t t = 0; t < Tw; ++t) sum += (double)col[t * L];
        m = sum / (double)Tw;
      }
      mean[j] = m;
    }
    __syncthreads();
    if (c0 + tid < n_out) {
      double m[N], hx[N], hb[N];   // the ring: entry a is the filtered row q - 2R + a
#pragma unroll
      for (int j = 0; j < N; ++j) { m[j] = mean[tid + j]; hx[j] = 0.0; hb[j] = 0.0; }
      const float* col = img + c0 + tid;
      for (int64_t q = 0; q < Tw; ++q) {
        double g[N];
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = (double)col[q * L + j] - m[j];
        double x = Taps::dx(0) * g[0], b = Taps::b(0) * g[0];
#pragma unroll
        for (int j = 1; j < N; ++j) { x += Taps::dx(j) * g[j]; b += Taps::b(j) * g[j]; }
#pragma unroll
        for (int a = 0; a < N - 1; ++a) { hx[a] = hx[a + 1]; hb[a] = hb[a + 1]; }
        hx[N - 1] = x; hb[N - 1] = b;
        if (q >= 2 * R) {
          double gx = Taps::b(0) * hx[0], gt = Taps::dx(0) * hb[0];
#pragma unroll
          for (int a = 1; a < N; ++a) { gx += Taps::b(a) * hx[a]; gt += Taps::dx(a) * hb[a]; }
          jxx += gx * gx; jtt += gt * gt; jxt += gx * gt;
        }
      }
    }
    __syncthreads();   // the means are rewritten by the next strip
  }
  red[0][tid] = jxx; red[1][tid] = jtt; red[2][tid] = jxt;
  __syncthreads();
  for (int h = kOriBlock / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double Jxx = red[0][0], Jtt = red[1][0], Jxt = red[2][0];
    const double d = Jxx - Jtt, r = sqrt(d * d + 4.0 * Jxt * Jxt);
    double* ten = tensor + (int64_t)blockIdx.x * 3;
    ten[0] = Jxx; ten[1] = Jtt; ten[2] = Jxt;
    slope[blockIdx.x] = (-2.0 * Jxt) / (d + r);   // the half-angle form; 0 / 0 = NaN for a constant window
    coherency[blockIdx.x] = r / (Jxx + Jtt);
  }
}

}  // namespace

hipError_t launch_sti_gather(const void* frames, int dtype, int64_t T, int H, int W, const StiTable& table, int64_t S, int L, float* sti,
                             int64_t t_offset, int64_t T_total, hipStream_t s) {
  if (T == 0 || S == 0) return hipSuccess;
  const int64_t n_points = S * L, frame_elems = (int64_t)H * W;
  const dim3 grid((unsigned)((n_points + kGatherBlock - 1) / kGatherBlock),
                  (unsigned)std::min<int64_t>((T + kGatherFrames - 1) / kGatherFrames, 65535));
  if (dtype == 0)
    hipLaunchKernelGGL(sti_gather_kernel<uint8_t>, grid, dim3(kGatherBlock), 0, s, (const uint8_t*)frames, T, frame_elems, W, table, n_points, L,
                       sti, t_offset, T_total);
  else
    hipLaunchKernelGGL(sti_gather_kernel<float>, grid, dim3(kGatherBlock), 0, s, (const float*)frames, T, frame_elems, W, table, n_points, L, sti,
                       t_offset, T_total);
  return hipGetLastError();
}

hipError_t launch_sti_orientation(const float* sti, int64_t S, int64_t T, int L, int64_t Tw, int64_t stride, int64_t K, int smooth, bool detrend,
                                  double* tensor, double* slope, double* coherency, hipStream_t s) {
  if (S == 0 || K == 0) return hipSuccess;
  const dim3 grid((unsigned)(S * K)), block(kOriBlock);
  const int dt = detrend ? 1 : 0;
  switch (smooth) {
    case 0: hipLaunchKernelGGL(sti_orientation_kernel<0>, grid, block, 0, s, sti, T, L, Tw, stride, K, dt, tensor, slope, coherency); break;
    case 1: hipLaunchKernelGGL(sti_orientation_kernel<1>, grid, block, 0, s, sti, T, L, Tw, stride, K, dt, tensor, slope, coherency); break;
    case 2: hipLaunchKernelGGL(sti_orientation_kernel<2>, grid, block, 0, s, sti, T, L, Tw, stride, K, dt, tensor, slope, coherency); break;
    case 3: hipLaunchKernelGGL(sti_orientation_kernel<3>, grid, block, 0, s, sti, T, L, Tw, stride, K, dt, tensor, slope, coherency); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace lspiv
