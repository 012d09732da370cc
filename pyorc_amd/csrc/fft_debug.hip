// Test hook: the register FFTs of fft_regs.h, one transform per thread, so the parity suite can hold every length the
// PIV kernels instantiate (8, 16, 32, 64 and the prime-factor lengths P * 2^m) against numpy.fft directly.
// FORM 0 is the transform the kernels use (fft_n); 1 and 2 are the un-folded and the folded twiddle path of 16 / 32 / 64 by name,
// whichever of them the length has adopted, and 4 is the conjugate-pair split-radix form, so that one library can hold them against each
// other (3 is not a form: the values are one bit each).
#include "piv_fft_impl.h"

namespace lspiv {

template <bool INV, int FORM> __device__ __forceinline__ void fft_form(float (&r)[16], float (&i)[16]) { fft16<INV, false, FORM == 2, FORM == 4>(r, i); }
template <bool INV, int FORM> __device__ __forceinline__ void fft_form(float (&r)[32], float (&i)[32]) { fft32<INV, false, FORM == 2, FORM == 4>(r, i); }
template <bool INV, int FORM> __device__ __forceinline__ void fft_form(float (&r)[64], float (&i)[64]) { fft64<INV, false, FORM == 2, FORM == 4>(r, i); }

template <int N, bool INV, int FORM = 0>
__global__ void fft_debug_kernel(const float* in, float* out, int count) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  float r[N], i[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { r[j] = in[(size_t)t * 2 * N + 2 * j]; i[j] = in[(size_t)t * 2 * N + 2 * j + 1]; }
  if constexpr (FORM == 0) fft_n<INV>(r, i); else fft_form<INV, FORM>(r, i);
#pragma unroll
  for (int j = 0; j < N; ++j) { out[(size_t)t * 2 * N + 2 * j] = r[j]; out[(size_t)t * 2 * N + 2 * j + 1] = i[j]; }
}

template <int N, int FORM = 0>
static hipError_t launch_one(bool inverse, const float* in, float* out, int count, hipStream_t s) {
  const dim3 grid((count + 63) / 64), block(64);
  if (inverse) hipLaunchKernelGGL((fft_debug_kernel<N, true, FORM>), grid, block, 0, s, in, out, count);
  else hipLaunchKernelGGL((fft_debug_kernel<N, false, FORM>), grid, block, 0, s, in, out, count);
  return hipGetLastError();
}

hipError_t launch_fft_debug(int n, bool inverse, const float* in, float* out, int count, hipStream_t s) {
  switch (n) {
    case 8: return launch_one<8>(inverse, in, out, count, s);
    case 16: return launch_one<16>(inverse, in, out, count, s);
    case 32: return launch_one<32>(inverse, in, out, count, s);
    case 64: return launch_one<64>(inverse, in, out, count, s);
#define LSPIV_PFA_CASE(m) case m: return launch_one<m>(inverse, in, out, count, s);
    LSPIV_PFA_SIZES(LSPIV_PFA_CASE)
#undef LSPIV_PFA_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_fft_debug_form(int n, int form, bool inverse, const float* in, float* out, int count, hipStream_t s) {
  if (form == 0) return launch_fft_debug(n, inverse, in, out, count, s);
  if (form != 1 && form != 2 && form != 4) return hipErrorInvalidValue;
  switch (n) {
    case 16: return form == 1 ? launch_one<16, 1>(inverse, in, out, count, s) : form == 2 ? launch_one<16, 2>(inverse, in, out, count, s) : launch_one<16, 4>(inverse, in, out, count, s);
    case 32: return form == 1 ? launch_one<32, 1>(inverse, in, out, count, s) : form == 2 ? launch_one<32, 2>(inverse, in, out, count, s) : launch_one<32, 4>(inverse, in, out, count, s);
    case 64: return form == 1 ? launch_one<64, 1>(inverse, in, out, count, s) : form == 2 ? launch_one<64, 2>(inverse, in, out, count, s) : launch_one<64, 4>(inverse, in, out, count, s);
    default: return hipErrorInvalidValue;
  }
}

// Test hook: the 32-lane reductions of common.h on whole waves, one wave of 64 lanes per block.  OP 0 = half_sum (float bits), 1 =
// half_sum_i, 2 = half_min_i, 3 = half_max_i; FORM 0 = the ds_swizzle form, 1 = the v_permlane16_swap form, 2 / 3 = the paired form
// (half_reduce2_i, integers only) on x = the lane's value and y = the value of the same lane of the wave's OTHER half: 2 stores the
// result for x, 3 the one for y -- which is what the other half's lanes get for their x
template <int OP, int FORM>
__global__ __launch_bounds__(64) void half_reduce_debug_kernel(const uint32_t* in, uint32_t* out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;   // the grid is `count` blocks of 64 lanes over count * 64 values
  const uint32_t x = in[t];
  uint32_t r;
  if constexpr (FORM >= 2) {
    static_assert(OP >= 1 && OP <= 3, "the paired form is for integers");
    int a = (int)x, b = (int)in[t ^ 32];
    half_reduce2_i<OP == 1 ? RedOp::kSum : OP == 2 ? RedOp::kMin : RedOp::kMax>(a, b);
    r = (uint32_t)(FORM == 2 ? a : b);
  } else {
    constexpr bool S16 = FORM == 1;
    if constexpr (OP == 0) r = __builtin_bit_cast(uint32_t, half_sum<S16>(__builtin_bit_cast(float, x)));
    else if constexpr (OP == 1) r = (uint32_t)half_sum_i<S16>((int)x);
    else if constexpr (OP == 2) r = (uint32_t)half_min_i<S16>((int)x);
    else r = (uint32_t)half_max_i<S16>((int)x);
  }
  out[t] = r;
}
template <int OP>
static hipError_t launch_half_reduce(int form, const uint32_t* in, uint32_t* out, int count, hipStream_t s) {
  if (form == 0) hipLaunchKernelGGL((half_reduce_debug_kernel<OP, 0>), dim3(count), dim3(64), 0, s, in, out);
  else if (form == 1) hipLaunchKernelGGL((half_reduce_debug_kernel<OP, 1>), dim3(count), dim3(64), 0, s, in, out);
  else if constexpr (OP >= 1) {
    if (form == 2) hipLaunchKernelGGL((half_reduce_debug_kernel<OP, 2>), dim3(count), dim3(64), 0, s, in, out);
    else hipLaunchKernelGGL((half_reduce_debug_kernel<OP, 3>), dim3(count), dim3(64), 0, s, in, out);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_half_reduce_debug(int op, int form, const uint32_t* in, uint32_t* out, int count, hipStream_t s) {
  if (form < 0 || form > 3) return hipErrorInvalidValue;
  switch (op) {
    case 0: return launch_half_reduce<0>(form, in, out, count, s);
    case 1: return launch_half_reduce<1>(form, in, out, count, s);
    case 2: return launch_half_reduce<2>(form, in, out, count, s);
    case 3: return launch_half_reduce<3>(form, in, out, count, s);
    default: return hipErrorInvalidValue;
  }
}

// Test hook: the first-match search of the 32 x 32 peak search on whole waves, one wave per block.  in = one flag per lane (non-zero =
// the lane matches); out = what every lane of the group gets: the smallest SHIFTED index (lane + 16) & 31 among the group's matching
// lanes, 1 << 12 where the group has none.  FORM 0 = the DPP arg-min (half_min_i in its v_permlane16_swap form), 1 = one ballot and a bit
// scan per group (first_shifted), 2 = the paired DPP chain (half_reduce2_i) on the lane's flag and that of the same lane of the other half
template <int FORM>
__global__ __launch_bounds__(64) void first_match_debug_kernel(const uint32_t* in, uint32_t* out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool match = in[t] != 0u;
  const int sh = (int)((threadIdx.x + 16u) & 31u);
  int r;
  if constexpr (FORM == 0) {
    r = half_min_i<true>(match ? sh : kNoMatch);
  } else if constexpr (FORM == 1) {
    r = group_pick(first_shifted(__builtin_amdgcn_ballot_w64(match)), (threadIdx.x & 32u) != 0u);
  } else {
    int b = in[t ^ 32] != 0u ? sh : kNoMatch;
    r = match ? sh : kNoMatch;
    half_reduce2_i<RedOp::kMin>(r, b);
  }
  out[t] = (uint32_t)r;
}
hipError_t launch_first_match_debug(int form, const uint32_t* in, uint32_t* out, int count, hipStream_t s) {
  if (form == 0) hipLaunchKernelGGL((first_match_debug_kernel<0>), dim3(count), dim3(64), 0, s, in, out);
  else if (form == 1) hipLaunchKernelGGL((first_match_debug_kernel<1>), dim3(count), dim3(64), 0, s, in, out);
  else if (form == 2) hipLaunchKernelGGL((first_match_debug_kernel<2>), dim3(count), dim3(64), 0, s, in, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lspiv
