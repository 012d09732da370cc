// What the integer predictors share (piv_multipass.hip: the offsets of a multi-pass chain and the nodes of a deformation pass;
// piv_lag_tables.hip: the lags of INTEGRATION.md section 2k): the rounding of a float32 vector to integers and twice the median over the
// valid 3 x 3 neighbours.  After the rounding everything is exact integer arithmetic, so that a float64 reference on the host gives the
// very same integers.  Device code only; included into the anonymous namespace's translation units.
#pragma once
#include <climits>

#include "common.h"

namespace lspiv {
namespace predict {

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// finite: the exponent field is not all ones (on the bits: no floating-point compare a fast-math flag could fold)
__device__ __forceinline__ bool is_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
// q = rint (half to even, in float32) clamped to the range of the int16 offsets, [-32768, 32767]: a frame side is at most 32767, so no
// displacement a frame can hold is touched, the conversion to int is defined for every finite input, and sums of two q cannot overflow
__device__ __forceinline__ int round_q(float x) { return (int)fminf(fmaxf(rintf(x), -32768.0f), 32767.0f); }
// deformation nodes: q = rint(64 x) (the product is exact in float32, or infinite), clamped to +-32767 * 64
__device__ __forceinline__ int round_q64(float x) {
  constexpr float lim = 32767.0f * (float)kDeformQ;
  return (int)fminf(fmaxf(rintf((float)kDeformQ * x), -lim), lim);
}

// twice the median of the rounded vectors over the valid ones of the 3 x 3 neighbourhood of coarse window (r, c), clipped at the
// grid's edges, centre included: odd count 2 * middle, even count the sum of the two middle values, none 0.  The nine values of a
// component live in registers: an odd-even transposition sort with constant indices, invalid entries sorted to the end.
// Q64: the vectors are rounded to 1 / 64 px (round_q64) instead of whole pixels.
template <bool Q64 = false>
__device__ __forceinline__ void median2(const float* u, const float* v, int n_rows, int n_cols, int r, int c, int& mu, int& mv) {
  int qu[9], qv[9];
  int k = 0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const int rr = r + e / 3 - 1, cc = c + e % 3 - 1;
    const bool in = (unsigned)rr < (unsigned)n_rows && (unsigned)cc < (unsigned)n_cols;
    const size_t i = (size_t)(in ? rr : r) * n_cols + (in ? cc : c);
    const float fu = u[i], fv = v[i];
    const bool ok = in && is_finite(fu) && is_finite(fv);
    qu[e] = ok ? (Q64 ? round_q64(fu) : round_q(fu)) : INT_MAX;       // (INT_MAX, the invalid entries' sort key, is outside the range of q)
    qv[e] = ok ? (Q64 ? round_q64(fv) : round_q(fv)) : INT_MAX;
    k += ok ? 1 : 0;
  }
#pragma unroll
  for (int round = 0; round < 9; ++round) {
#pragma unroll
    for (int i = round & 1; i + 1 < 9; i += 2) {
      const int a = qu[i], b = qu[i + 1];
      qu[i] = min(a, b); qu[i + 1] = max(a, b);
      const int a2 = qv[i], b2 = qv[i + 1];
      qv[i] = min(a2, b2); qv[i + 1] = max(a2, b2);
    }
  }
  const int lo = (k - 1) >> 1, hi = k >> 1;   // the same entry for an odd count
  int ul = 0, uh = 0, vl = 0, vh = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    ul = i == lo ? qu[i] : ul; uh = i == hi ? qu[i] : uh;
    vl = i == lo ? qv[i] : vl; vh = i == hi ? qv[i] : vh;
  }
  mu = k > 0 ? ul + uh : 0;
  mv = k > 0 ? vl + vh : 0;
}

}  // namespace predict
}  // namespace lspiv
