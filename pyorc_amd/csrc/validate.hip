// Vector validation on the device-resident result block: the normalised median test (Westerweel & Scarano 2005) over the 3 x 3
// neighbourhood of every vector of (T, R, C), with the runner-up vector of the second correlation peak as the first substitute for a
// rejected one (include/lspiv.h, lspiv_validate_dev).
//
// One lane per vector, lanes along x, one launch per Jacobi iteration.  The rule is built from selections and single correctly rounded
// float32 operations only -- no expression of the shape a * b + c exists, and contraction is switched off for the file all the same --,
// so the result is the float32 numpy restatement's (tests/validate_ref.py) value for value.  HBM streaming: 8 bytes in and 9 out per
// vector; the eight neighbours are L1 / L2 hits of the rows the adjacent lanes and blocks stream.
#include "validate.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace lspiv {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_MAX; }   // false for +-inf and NaN

__device__ __forceinline__ void cex(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo; b = hi;
}

// eight values ascending: the 19 compare-exchanges of the classic network, in registers (no NaN comes in: a missing neighbour is +inf)
__device__ __forceinline__ void sort8(float (&x)[8]) {
  cex(x[0], x[1]); cex(x[2], x[3]); cex(x[4], x[5]); cex(x[6], x[7]);
  cex(x[0], x[2]); cex(x[1], x[3]); cex(x[4], x[6]); cex(x[5], x[7]);
  cex(x[1], x[2]); cex(x[5], x[6]); cex(x[0], x[4]); cex(x[3], x[7]);
  cex(x[1], x[5]); cex(x[2], x[6]);
  cex(x[1], x[4]); cex(x[3], x[6]);
  cex(x[2], x[4]); cex(x[3], x[5]);
  cex(x[3], x[4]);
}

// x[k] for a run-time k by a select chain over the compile-time positions (a run-time index would put the array into scratch)
__device__ __forceinline__ float pick8(const float (&x)[8], int k) {
  float r = x[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) r = k == j ? x[j] : r;
  return r;
}

// median of the first n (1 .. 8) of eight sorted values: the middle one, or 0.5f * (the two middle ones): one add, one multiply
__device__ __forceinline__ float median8(const float (&x)[8], int n) {
  const float lo = pick8(x, (n - 1) >> 1), hi = pick8(x, n >> 1);
  return (n & 1) ? lo : 0.5f * (lo + hi);
}

__global__ __launch_bounds__(kBlock) void validate_kernel(const float* __restrict__ u_in, const float* __restrict__ v_in,
                                                          const float* __restrict__ peak2, int64_t N, int R, int C, ValidateParams p,
                                                          int first, float* __restrict__ u_out, float* __restrict__ v_out,
                                                          uint8_t* __restrict__ flag) {
  const int64_t n_cell = (int64_t)R * C;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
    const int64_t cell = i % n_cell;
    const int r = (int)(cell / C), c = (int)(cell - (int64_t)r * C);
    float u0 = u_in[i], v0 = v_in[i];
    uint8_t fl = first ? (uint8_t)0 : flag[i];
    // the up to eight neighbours of the same time step, inside the grid (no wrap across row ends or time steps), finite in u AND v
    float un[8], vn[8];
    int n = 0, k = 0;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
      for (int dc = -1; dc <= 1; ++dc) {
        if (dr == 0 && dc == 0) continue;
        const bool in = r + dr >= 0 && r + dr < R && c + dc >= 0 && c + dc < C;
        const int64_t j = in ? i + (int64_t)dr * C + dc : i;
        const float a = u_in[j], b = v_in[j];
        const bool ok = in && finite(a) && finite(b);
        un[k] = ok ? a : INFINITY;
        vn[k] = ok ? b : INFINITY;
        n += ok;
        ++k;
      }
    if (finite(u0) && finite(v0) && n >= p.min_neighbours) {   // judged; anything else keeps value and flag
      float su[8], sv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { su[q] = un[q]; sv[q] = vn[q]; }
      sort8(su); sort8(sv);
      const float um = median8(su, n), vm = median8(sv, n);
#pragma unroll
      for (int q = 0; q < 8; ++q) {   // a missing neighbour (the only +inf: the others are finite) stays +inf, whatever the median
        su[q] = un[q] == INFINITY ? INFINITY : fabsf(un[q] - um);
        sv[q] = vn[q] == INFINITY ? INFINITY : fabsf(vn[q] - vm);
      }
      sort8(su); sort8(sv);
      const float lu = p.threshold * (median8(su, n) + p.epsilon), lv = p.threshold * (median8(sv, n) + p.epsilon);
      if (fabsf(u0 - um) > lu || fabsf(v0 - vm) > lv) {
        bool substituted = false;
        if (peak2 != nullptr && fl == 0) {   // the runner-up of a vector that is still the primary one, tested against the same limits
          const float u2 = peak2[4 * i], v2 = peak2[4 * i + 1];
          if (finite(u2) && finite(v2) && !(fabsf(u2 - um) > lu || fabsf(v2 - vm) > lv)) {
            u0 = u2; v0 = v2; fl = 2;
            substituted = true;
          }
        }
        if (!substituted) {
          if (p.replace == 0) { u0 = NAN; v0 = NAN; fl = 1; }
          else { u0 = um; v0 = vm; fl = 3; }
        }
      }
    }
    u_out[i] = u0;
    v_out[i] = v0;
    flag[i] = fl;
  }
}

}  // namespace

hipError_t launch_validate(const float* u_in, const float* v_in, const float* peak2, int64_t T, int R, int C, const ValidateParams& p,
                           bool first, float* u_out, float* v_out, uint8_t* flag, hipStream_t s) {
  const int64_t N = T * R * C;
  if (N == 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((N + kBlock - 1) / kBlock, 256 * 32);
  hipLaunchKernelGGL(validate_kernel, dim3(grid), dim3(kBlock), 0, s, u_in, v_in, peak2, N, R, C, p, first ? 1 : 0, u_out, v_out, flag);
  return hipGetLastError();
}

}  // namespace lspiv
