// Pyramidal Lucas-Kanade point tracking (Lucas & Kanade 1981; the pyramidal forward-additive form of Bouguet 2001): the displacement of
// a small window around a point between two frames, refined from the coarsest level of a Gaussian pyramid down to the frame itself.
// Two kernels (include/lspiv.h):
//
//   pyr_down_kernel<T>    one thread per sample of the next level: the five taps [1, 4, 6, 4, 1] along x on each of the five (reflected)
//                         source rows, then along y, times 2^-8.  25 loads per sample, neighbours' loads on the same cache lines.
//   lk_track_kernel<T, w> one WAVE per (point, pair) through all levels; kWaves waves per block that never meet (no block barrier: their
//                         iteration counts differ).  Sample k of the w x w window lives on lane k mod 64, at most 16 per lane.  Per level:
//                         the (w + 2)^2 template patch is sampled into the wave's own LDS patch -- the one exchange of the kernel -- from
//                         which each lane takes its samples' I and the central differences Ix, Iy (into registers up to w = kRegWindow,
//                         from the patch again in every iteration above: lk_level); the 2 x 2 normal matrix once; then per iteration the four neighbours of every J sample straight from the level (clamped indices: the
//                         level is edge replicated, nothing outside it is read), the mismatch vector b, the solve.  The float64 sums: a
//                         lane adds its samples with k ascending, then a butterfly over the lanes (32, 16, .. 1) -- every lane ends with
//                         the bits of the halving tree, since a + b = b + a -- and the total goes through readfirstlane, so that the
//                         solve, the position and every decision are wave-uniform values and branches.
//
// The arithmetic is tests/track_ref.py's operation for operation: contraction is off for the whole file, as in stiv.hip, so every
// product, sum and difference written here is one correctly rounded operation; float32 x float32 products are formed in float64, where
// they are exact.  Only the order of the float64 sums is this file's own (track_ref.py: order="lanes").
#include "track.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace lspiv {

namespace {

constexpr int kPyrBlock = 256;
constexpr int kWaves = 4;   // waves (points) per block of lk_track_kernel
constexpr int kLoadGroup = 4;   // samples per lane and trip of the loops that are not unrolled whole: 16 loads in flight
#ifndef LSPIV_TRACK_REG_WINDOW
#define LSPIV_TRACK_REG_WINDOW 17   // (a build flag for A/B measurements: tools/build_variant.sh)
#endif
constexpr int kRegWindow = LSPIV_TRACK_REG_WINDOW;   // the largest window whose template stays in registers (17: 5 samples per lane)

__device__ inline int reflect(int i, int n) {   // -1 -> 1, n -> n - 2
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

template <typename T>
__global__ __launch_bounds__(kPyrBlock) void pyr_down_kernel(const T* __restrict__ src, int64_t n_frames, int H, int W, int Ho, int Wo,
                                                             float* __restrict__ dst) {
  const int64_t per_frame = (int64_t)Ho * Wo;
  const int64_t o = (int64_t)blockIdx.x * kPyrBlock + threadIdx.x;
  if (o >= n_frames * per_frame) return;
  const int64_t t = o / per_frame;
  const int rem = (int)(o - t * per_frame);
  const int y = rem / Wo, x = rem - y * Wo;
  const T* img = src + t * (int64_t)H * W;
  int cx[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) cx[j] = reflect(2 * x + j - 2, W);
  float h[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const T* row = img + (int64_t)reflect(2 * y + i - 2, H) * W;
    const float a0 = (float)row[cx[0]], a1 = (float)row[cx[1]], a2 = (float)row[cx[2]], a3 = (float)row[cx[3]], a4 = (float)row[cx[4]];
    h[i] = ((a0 + a4) + 4.0f * (a1 + a3)) + 6.0f * a2;
  }
  dst[o] = (((h[0] + h[4]) + 4.0f * (h[1] + h[3])) + 6.0f * h[2]) * 0.00390625f;
}

// ---- the tracker ------------------------------------------------------------------------------------------------------------------------
__device__ inline double uniform(double v) {   // the first lane's value as a wave-uniform one
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return uniform(v);
}
// the wave's LDS patch changes hands between its lanes: no lane's access moves across this point
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ix = floor(q) as an int that index arithmetic cannot overflow (a position far outside samples the replicated edge), f = float32(q - floor(q))
__device__ inline void split(double q, int* i, float* f) {
  const double fl = floor(q);
  *f = (float)(q - fl);
  *i = (int)fmin(fmax(fl, -1073741824.0), 1073741824.0);   // (NaN: fmax gives the bound; f is NaN and the sums say so)
}

// A template value as the iteration loop sees it: opaque, so that what is derived from it (the float64 form of a gradient, a sample's row
// and column) is formed where it is used, not once per level and kept in registers of its own -- that cost 6 VGPRs per sample.
template <typename V>
__device__ inline V here(V v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <typename S>
__device__ inline float bilinear(const S* __restrict__ img, int Wl, int Hl, int x, int y, float fx, float fy) {
  const int xa = std::min(std::max(x, 0), Wl - 1), xb = std::min(std::max(x + 1, 0), Wl - 1);
  const int ya = std::min(std::max(y, 0), Hl - 1) * Wl, yb = std::min(std::max(y + 1, 0), Hl - 1) * Wl;
  // (unsigned element offsets, below 2^30: the loads take the level's base from scalar registers and a 32-bit offset per lane)
  const float a = (float)img[(unsigned)(ya + xa)], b = (float)img[(unsigned)(ya + xb)], c = (float)img[(unsigned)(yb + xa)],
              d = (float)img[(unsigned)(yb + xb)];
  const float top = a + fx * (b - a);
  const float bot = c + fx * (d - c);
  return top + fy * (bot - top);
}

struct LkPoint {
  double dx, dy, lam, err;
  int n_iter, status;
};

// One level: the template around (px, py) in imgI, the iterations against imgJ from st->dx, st->dy on.  false: the point is lost
// (st->status says how).  last: level 0 -- lam, status 1 and err are its.
// The template of a lane's samples: windows up to kRegWindow keep I, Ix, Iy in registers (3 x 5 at most); larger ones (up to 16 samples
// per lane) read the patch again in every iteration and form the differences anew -- the same operations on the same values, so the
// same bits -- which keeps every variant at the register count of the small ones.
template <int WIN, typename S>
__device__ inline bool lk_level(const S* __restrict__ imgI, const S* __restrict__ imgJ, int Wl, int Hl, double px, double py, float* patch,
                                int lane, int max_iter, double eps2, double min_eig, bool last, LkPoint* st) {
  constexpr int R = (WIN - 1) / 2, PW = WIN + 2, NP = PW * PW, NW = WIN * WIN, NSP = (NP + 63) / 64, NS = (NW + 63) / 64;
  constexpr bool kRegs = WIN <= kRegWindow;
  constexpr int NR = kRegs ? NS : 1, kUnroll = kRegs ? NS : kLoadGroup;
  int ix, iy;
  float fx, fy;
  split(px, &ix, &fx);
  split(py, &iy, &fy);
  lane = here(lane) & 63;   // (the samples' rows and columns are formed per level: kept over the level loop they were 36 spilled registers)
  wave_sync();   // the last level's reads of the patch are done
#pragma unroll kLoadGroup
  for (int s = 0; s < NSP; ++s) {
    const int k = lane + 64 * s;
    if (k < NP) {
      const int pi = k / PW, pj = k - pi * PW;
      patch[k] = bilinear(imgI, Wl, Hl, ix + pj - R - 1, iy + pi - R - 1, fx, fy);
    }
  }
  wave_sync();
  // sample s of this lane: its row and column in the window (lanes past the window: its last sample, weight 0), and its template
  struct Tmpl { float I, Ix, Iy; };
  const auto from_patch = [&](int ln, int s, int* i, int* j) {
    const int k = ln + 64 * s;
    const bool in = k < NW;
    const int kk = in ? k : NW - 1;
    *i = kk / WIN; *j = kk - *i * WIN;
    const float* c = patch + (*i + 1) * PW + (*j + 1);
    const float v = c[0], x = 0.5f * (c[1] - c[-1]), y = 0.5f * (c[PW] - c[-PW]);
    return Tmpl{in ? v : 0.0f, in ? x : 0.0f, in ? y : 0.0f};
  };
  float I[NR], Ix[NR], Iy[NR];
  double gxx = 0.0, gyy = 0.0, gxy = 0.0;
#pragma unroll kUnroll
  for (int s = 0; s < NS; ++s) {
    int i, j;
    const Tmpl t = from_patch(lane, s, &i, &j);
    if constexpr (kRegs) { I[s] = t.I; Ix[s] = t.Ix; Iy[s] = t.Iy; }
    const double x64 = (double)t.Ix, y64 = (double)t.Iy;
    gxx += x64 * x64; gyy += y64 * y64; gxy += x64 * y64;
  }
  const double Gxx = wave_sum(gxx), Gyy = wave_sum(gyy), Gxy = wave_sum(gxy);
  if (!(isfinite(Gxx) && isfinite(Gyy) && isfinite(Gxy))) { st->status = 4; return false; }
  const double det = Gxx * Gyy - Gxy * Gxy;
  const double dif = Gxx - Gyy;
  const double lam = ((Gxx + Gyy) - sqrt(dif * dif + 4.0 * (Gxy * Gxy))) / (2.0 * (double)NW);
  if (last) st->lam = lam;
  if (!(det > 1e-9 * Gxx * Gyy) || lam < min_eig) { st->status = 2; return false; }

  // sample s against J at (jx + hx, jy + hy): the template (from the registers, or from the patch again) and e = I - J
  const auto mismatch = [&](int ln, int s, int jx, int jy, float hx, float hy, Tmpl* t) {
    int i, j;
    if constexpr (kRegs) {
      const int kk = std::min(ln + 64 * s, NW - 1);
      i = kk / WIN; j = kk - i * WIN;
      *t = Tmpl{I[s], here(Ix[s]), here(Iy[s])};
    } else {
      *t = from_patch(ln, s, &i, &j);
    }
    const float J = bilinear(imgJ, Wl, Hl, jx + j - R, jy + i - R, hx, hy);
    return ln + 64 * s < NW ? t->I - J : 0.0f;
  };
  bool converged = false;
  for (int it = 0; it < max_iter; ++it) {
    int jx, jy;
    float hx, hy;
    split(px + st->dx, &jx, &hx);
    split(py + st->dy, &jy, &hy);
    const int ln = here(lane) & 63;   // (a sample's row and column: two multiplications where they are used, not a register held over the loop)
    double bx = 0.0, by = 0.0;
#pragma unroll kUnroll
    for (int s = 0; s < NS; ++s) {
      Tmpl t;
      const float e = mismatch(ln, s, jx, jy, hx, hy, &t);
      bx += (double)e * (double)t.Ix; by += (double)e * (double)t.Iy;
    }
    const double Bx = wave_sum(bx), By = wave_sum(by);
    if (!(isfinite(Bx) && isfinite(By))) { st->status = 4; return false; }
    const double ddx = (Gyy * Bx - Gxy * By) / det, ddy = (Gxx * By - Gxy * Bx) / det;
    st->dx += ddx; st->dy += ddy;
    st->n_iter += 1;
    const double qx = px + st->dx, qy = py + st->dy;
    if (!(qx >= 0.0 && qx <= (double)(Wl - 1) && qy >= 0.0 && qy <= (double)(Hl - 1))) { st->status = 3; return false; }
    if (ddx * ddx + ddy * ddy < eps2) { converged = true; break; }
  }
  if (last) {
    if (!converged) st->status = 1;
    int jx, jy;
    float hx, hy;
    split(px + st->dx, &jx, &hx);
    split(py + st->dy, &jy, &hy);
    const int ln = here(lane) & 63;
    double ea = 0.0;
#pragma unroll kUnroll
    for (int s = 0; s < NS; ++s) {
      Tmpl t;
      ea += (double)fabsf(mismatch(ln, s, jx, jy, hx, hy, &t));
    }
    const double err = wave_sum(ea) / (double)NW;
    if (!isfinite(err)) { st->status = 4; return false; }
    st->err = err;
  }
  return true;
}

template <typename T, int WIN>
__global__ __launch_bounds__(kWaves * 64, 4) void lk_track_kernel(const LkParams p) {
  __shared__ float patches[kWaves][(WIN + 2) * (WIN + 2)];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int64_t job = (int64_t)blockIdx.x * kWaves + wave;
  if (job >= p.n_pairs * p.N) return;   // wave-uniform: the waves of a block share nothing
  const int64_t pair = job / p.N;
  const int n = (int)(job - pair * p.N);
  const double x = p.points[pair * p.points_stride + 2 * n], y = p.points[pair * p.points_stride + 2 * n + 1];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  LkPoint st{0.0, 0.0, nan, nan, 0, 0};
  bool ok = isfinite(x) && isfinite(y);
  if (!ok) st.status = 5;
  if (ok && p.guess) {   // the guess in pixels of the coarsest level (a power of two: exact)
    st.dx = ldexp(p.guess[pair * p.guess_stride + 2 * n], 1 - p.levels);
    st.dy = ldexp(p.guess[pair * p.guess_stride + 2 * n + 1], 1 - p.levels);
  }
  float* patch = patches[wave];
  for (int lvl = p.levels - 1; lvl >= 1 && ok; --lvl) {
    const int Hl = p.H[lvl], Wl = p.W[lvl];
    const float* imgI = p.pyr[lvl] + pair * (int64_t)Hl * Wl;
    ok = lk_level<WIN, float>(imgI, imgI + (int64_t)Hl * Wl, Wl, Hl, ldexp(x, -lvl), ldexp(y, -lvl), patch, lane, p.max_iter, p.eps2,
                              p.min_eig, false, &st);
    st.dx = 2.0 * st.dx; st.dy = 2.0 * st.dy;
  }
  if (ok) {
    const int Hl = p.H[0], Wl = p.W[0];
    const T* imgI = (const T*)p.frames + pair * (int64_t)Hl * Wl;
    ok = lk_level<WIN, T>(imgI, imgI + (int64_t)Hl * Wl, Wl, Hl, x, y, patch, lane, p.max_iter, p.eps2, p.min_eig, true, &st);
  }
  if (lane == 0) {
    const double u = ok ? st.dx : nan, v = ok ? st.dy : nan;
    p.u[job] = u; p.v[job] = v;
    p.err[job] = ok ? st.err : nan;
    p.lam[job] = st.lam;
    p.n_iter[job] = st.n_iter;
    p.status[job] = (uint8_t)st.status;
    if (p.next) { p.next[2 * job] = x + u; p.next[2 * job + 1] = y + v; }
  }
}

template <typename T, int WIN>
hipError_t launch_lk(const LkParams& p, hipStream_t s) {
  const int64_t jobs = p.n_pairs * p.N;
  hipLaunchKernelGGL((lk_track_kernel<T, WIN>), dim3((unsigned)((jobs + kWaves - 1) / kWaves)), dim3(kWaves * 64), 0, s, p);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_lk_window(const LkParams& p, int window, hipStream_t s) {
  switch (window) {
    case 5: return launch_lk<T, 5>(p, s);
    case 7: return launch_lk<T, 7>(p, s);
    case 9: return launch_lk<T, 9>(p, s);
    case 11: return launch_lk<T, 11>(p, s);
    case 13: return launch_lk<T, 13>(p, s);
    case 15: return launch_lk<T, 15>(p, s);
    case 17: return launch_lk<T, 17>(p, s);
    case 19: return launch_lk<T, 19>(p, s);
    case 21: return launch_lk<T, 21>(p, s);
    case 23: return launch_lk<T, 23>(p, s);
    case 25: return launch_lk<T, 25>(p, s);
    case 27: return launch_lk<T, 27>(p, s);
    case 29: return launch_lk<T, 29>(p, s);
    case 31: return launch_lk<T, 31>(p, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_pyr_down(const void* frames, int dtype, int64_t T, int H, int W, float* out, hipStream_t s) {
  if (T == 0) return hipSuccess;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int64_t n = T * Ho * Wo;
  const dim3 grid((unsigned)((n + kPyrBlock - 1) / kPyrBlock)), block(kPyrBlock);
  if (dtype == 0)
    hipLaunchKernelGGL(pyr_down_kernel<uint8_t>, grid, block, 0, s, (const uint8_t*)frames, T, H, W, Ho, Wo, out);
  else
    hipLaunchKernelGGL(pyr_down_kernel<float>, grid, block, 0, s, (const float*)frames, T, H, W, Ho, Wo, out);
  return hipGetLastError();
}

hipError_t launch_lk_track(const LkParams& p, int dtype, int window, hipStream_t s) {
  if (p.n_pairs == 0 || p.N == 0) return hipSuccess;
  return dtype == 0 ? launch_lk_window<uint8_t>(p, window, s) : launch_lk_window<float>(p, window, s);
}

}  // namespace lspiv
