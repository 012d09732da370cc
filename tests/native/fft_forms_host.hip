// Stand-alone program for tests/test_fft_splitradix_host.py: the register FFTs of pyorc_amd/csrc/fft_regs.h instantiated for the HOST
// (they are __host__ __device__), one transform per row of a file, and -- for the compile-only check of the instruction counts --
// one kernel per length and direction that holds nothing but loads, the split-radix transform and stores.
//
//   fft_forms_host <n: 16|32|64> <inverse: 0|1> <form: 1 un-folded | 2 folded | 4 split radix> <in> <out>
//
// in / out: rows of n interleaved (re, im) float32 pairs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fft_regs.h"

using namespace lspiv;

template <bool INV, int FORM, bool CLAMP = false>
__host__ __device__ __forceinline__ void form_fft(float (&r)[16], float (&i)[16]) { fft16<INV, CLAMP, FORM == 2, FORM == 4>(r, i); }
template <bool INV, int FORM, bool CLAMP = false>
__host__ __device__ __forceinline__ void form_fft(float (&r)[32], float (&i)[32]) { fft32<INV, CLAMP, FORM == 2, FORM == 4>(r, i); }
template <bool INV, int FORM, bool CLAMP = false>
__host__ __device__ __forceinline__ void form_fft(float (&r)[64], float (&i)[64]) { fft64<INV, CLAMP, FORM == 2, FORM == 4>(r, i); }

// compile-only: `hipcc -S --cuda-device-only` of this file, the float32 arithmetic of each kernel is the transform's
template <int N, bool INV, bool CLAMP>
__global__ void sr_count_kernel(const float* in, float* out) {
  const size_t t = blockIdx.x * blockDim.x + threadIdx.x;
  float r[N], i[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { r[j] = in[t * 2 * N + 2 * j]; i[j] = in[t * 2 * N + 2 * j + 1]; }
  form_fft<INV, 4, CLAMP>(r, i);
#pragma unroll
  for (int j = 0; j < N; ++j) { out[t * 2 * N + 2 * j] = r[j]; out[t * 2 * N + 2 * j + 1] = i[j]; }
}
template __global__ void sr_count_kernel<16, false, false>(const float*, float*);
template __global__ void sr_count_kernel<32, false, false>(const float*, float*);
template __global__ void sr_count_kernel<64, false, false>(const float*, float*);
template __global__ void sr_count_kernel<16, true, false>(const float*, float*);
template __global__ void sr_count_kernel<32, true, false>(const float*, float*);
template __global__ void sr_count_kernel<64, true, false>(const float*, float*);
template __global__ void sr_count_kernel<16, true, true>(const float*, float*);
template __global__ void sr_count_kernel<32, true, true>(const float*, float*);
template __global__ void sr_count_kernel<64, true, true>(const float*, float*);

template <int N, bool INV, int FORM>
static void run_rows(const std::vector<float>& in, std::vector<float>& out) {
  const size_t rows = in.size() / (2 * N);
  for (size_t t = 0; t < rows; ++t) {
    float r[N], i[N];
    for (int j = 0; j < N; ++j) { r[j] = in[t * 2 * N + 2 * j]; i[j] = in[t * 2 * N + 2 * j + 1]; }
    form_fft<INV, FORM>(r, i);
    for (int j = 0; j < N; ++j) { out[t * 2 * N + 2 * j] = r[j]; out[t * 2 * N + 2 * j + 1] = i[j]; }
  }
}

template <int N, bool INV>
static bool run_form(int form, const std::vector<float>& in, std::vector<float>& out) {
  if (form == 1) run_rows<N, INV, 1>(in, out);
  else if (form == 2) run_rows<N, INV, 2>(in, out);
  else if (form == 4) run_rows<N, INV, 4>(in, out);
  else return false;
  return true;
}

template <int N>
static bool run_n(bool inv, int form, const std::vector<float>& in, std::vector<float>& out) {
  return inv ? run_form<N, true>(form, in, out) : run_form<N, false>(form, in, out);
}

int main(int argc, char** argv) {
  if (argc != 6) { std::fprintf(stderr, "usage: %s n inverse form in out\n", argv[0]); return 2; }
  const int n = std::atoi(argv[1]), form = std::atoi(argv[3]);
  const bool inv = std::atoi(argv[2]) != 0;
  if (n != 16 && n != 32 && n != 64) { std::fprintf(stderr, "n = 16, 32 or 64\n"); return 2; }
  std::FILE* f = std::fopen(argv[4], "rb");
  if (!f) { std::perror(argv[4]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes <= 0 || bytes % (long)(2 * n * sizeof(float))) { std::fprintf(stderr, "%s: not whole rows of %d pairs\n", argv[4], n); return 1; }
  std::vector<float> in(bytes / sizeof(float)), out(bytes / sizeof(float));
  if (std::fread(in.data(), 1, bytes, f) != (size_t)bytes) { std::fprintf(stderr, "short read\n"); return 1; }
  std::fclose(f);
  const bool ok = n == 16 ? run_n<16>(inv, form, in, out) : n == 32 ? run_n<32>(inv, form, in, out) : run_n<64>(inv, form, in, out);
  if (!ok) { std::fprintf(stderr, "form = 1, 2 or 4\n"); return 2; }
  f = std::fopen(argv[5], "wb");
  if (!f) { std::perror(argv[5]); return 1; }
  if (std::fwrite(out.data(), 1, bytes, f) != (size_t)bytes) { std::fprintf(stderr, "short write\n"); return 1; }
  std::fclose(f);
  return 0;
}
