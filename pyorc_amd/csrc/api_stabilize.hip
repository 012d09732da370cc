// C ABI of liblspiv_hip.so, frame stabilisation (api_core.hip has the overview): the transform fit over the vectors of the static part of
// the image, the chain of poses and the per-frame affine warp, each as a "_dev" entry point on device pointers and as a host twin that
// stages through the context's workspaces (api_internal.h, HostCall).  Replaces pyorc/cv.py's stabilisation (feature tracks +
// estimateAffinePartial2D) and the cv2.warpAffine per frame of pyorc's Video(stabilize=...); the semantics are this project's own
// (INTEGRATION.md section 2l).
#include "api_internal.h"

#include <cmath>

#include "stabilize.h"

namespace lspiv_api __attribute__((visibility("hidden"))) {

namespace {

int check_fit(const void* u, const void* v, int64_t pairs, int64_t rows, int64_t cols, int n, int oy, int ox, int64_t H, int64_t W, int model,
              double reject0, double reject1, int min_vectors, const void* P_out, const void* n_used_out, lspiv::StabilizeFitParams* p) {
  if (!u || !v || !P_out || !n_used_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (n != 16 && n != 32 && n != 64) return fail(LSPIV_EINVAL, "stabilize: window %d not in {16, 32, 64}", n);
  if (oy < 0 || oy >= n || ox < 0 || ox >= n) return fail(LSPIV_EINVAL, "stabilize: overlap (%d, %d) outside 0 .. %d", oy, ox, n - 1);
  if (pairs < 1 || pairs > 0x7fffffff) return fail(LSPIV_EINVAL, "stabilize: %lld pairs", (long long)pairs);
  if (H < n || W < n || H > 32767 || W > 32767) return fail(LSPIV_EINVAL, "stabilize: frame (%lld, %lld) for window %d", (long long)H, (long long)W, n);
  if (rows != (H - n) / (n - oy) + 1 || cols != (W - n) / (n - ox) + 1)
    return fail(LSPIV_EINVAL, "stabilize: grid (%lld, %lld) is not the one of frame (%lld, %lld), window %d, overlap (%d, %d)", (long long)rows,
                (long long)cols, (long long)H, (long long)W, n, oy, ox);
  if (model < LSPIV_STABILIZE_TRANSLATION || model > LSPIV_STABILIZE_AFFINE) return fail(LSPIV_EINVAL, "stabilize: unknown model %d", model);
  if (!(reject1 > 0.0) || !(reject0 > reject1) || std::isinf(reject0))
    return fail(LSPIV_EINVAL, "stabilize: reject (%g, %g) must be positive and decreasing", reject0, reject1);
  if (min_vectors < 1) return fail(LSPIV_EINVAL, "stabilize: min_vectors %d < 1", min_vectors);
  const double cx = (double)(W - 1) / 2.0, cy = (double)(H - 1) / 2.0, h = (double)(n - 1) / 2.0;
  *p = lspiv::StabilizeFitParams{(int)rows, (int)cols, h - cx, h - cy, (double)(n - ox), (double)(n - oy), cx, cy, model, reject0, reject1, min_vectors};
  return LSPIV_OK;
}

int check_warp(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const void* A, const void* out) {
  if (!frames || !A || !out) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(check_frames("warp_affine", dtype, T, 1, H, W, 1));
  if (frames == out) return fail(LSPIV_EINVAL, "warp_affine: out must be another buffer than frames");
  return LSPIV_OK;
}

}  // namespace

}  // namespace lspiv_api

using namespace lspiv_api;

extern "C" {

int lspiv_stabilize_fit_dev(const float* d_u, const float* d_v, int64_t pairs, int64_t rows, int64_t cols, int n, int oy, int ox, int64_t H,
                            int64_t W, int model, double reject0, double reject1, int min_vectors, double* d_P, int32_t* d_n_used,
                            void* stream) {
  lspiv::StabilizeFitParams p;
  LSPIV_TRY(check_fit(d_u, d_v, pairs, rows, cols, n, oy, ox, H, W, model, reject0, reject1, min_vectors, d_P, d_n_used, &p));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_stabilize_fit(d_u, d_v, pairs, p, d_P, d_n_used, s); });
}

int lspiv_stabilize_chain_dev(const double* d_P, int64_t pairs, const double* d_carry_in, double* d_A, double* d_carry_out, void* stream) {
  if (!d_A || (pairs > 0 && !d_P)) return fail(LSPIV_EINVAL, "NULL argument");
  if (pairs < 0 || pairs > 0x7fffffff) return fail(LSPIV_EINVAL, "stabilize: %lld pairs", (long long)pairs);
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_stabilize_chain(d_P, pairs, d_carry_in, d_A, d_carry_out, s); });
}

int lspiv_warp_affine_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* d_A, void* d_out, void* stream) {
  LSPIV_TRY(check_warp(d_frames, dtype, T, H, W, d_A, d_out));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_warp_affine(d_frames, dtype, T, (int)H, (int)W, d_A, d_out, s); });
}

int lspiv_stabilize_fit(const float* u, const float* v, int64_t pairs, int64_t rows, int64_t cols, int n, int oy, int ox, int64_t H, int64_t W,
                        int model, double reject0, double reject1, int min_vectors, double* P, int32_t* n_used) {
  lspiv::StabilizeFitParams p;
  LSPIV_TRY(check_fit(u, v, pairs, rows, cols, n, oy, ox, H, W, model, reject0, reject1, min_vectors, P, n_used, &p));
  const size_t fb = (size_t)pairs * rows * cols * sizeof(float), pb = (size_t)pairs * 6 * sizeof(double), nb = (size_t)pairs * sizeof(int32_t);
  HostCall hc({{u, fb}, {v, fb}}, {{P, pb}, {n_used, nb}});
  if (hc.upload())
    hc.ran(launch_status(lspiv::launch_stabilize_fit(hc.in<float>(0), hc.in<float>(1), pairs, p, hc.out<double>(0), hc.out<int32_t>(1), hc.stream())));
  return hc.finish(__func__);
}

int lspiv_stabilize_chain(const double* P, int64_t pairs, const double* carry_in, double* A, double* carry_out) {
  if (!A || (pairs > 0 && !P)) return fail(LSPIV_EINVAL, "NULL argument");
  if (pairs < 0 || pairs > 0x7fffffff) return fail(LSPIV_EINVAL, "stabilize: %lld pairs", (long long)pairs);
  const size_t six = 6 * sizeof(double), pb = (size_t)pairs * six, ab = (size_t)(pairs + 1) * six;
  HostCall hc({{P, pb}, {carry_in, six}}, {{A, ab}, {carry_out, six}});
  if (hc.upload())
    hc.ran(launch_status(lspiv::launch_stabilize_chain(hc.in<double>(0), pairs, hc.in<double>(1), hc.out<double>(0), hc.out<double>(1), hc.stream())));
  return hc.finish(__func__);
}

int lspiv_warp_affine(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* A, void* out) {
  LSPIV_TRY(check_warp(frames, dtype, T, H, W, A, out));
  const size_t fb = (size_t)T * H * W * elem_size(dtype), ab = (size_t)T * 6 * sizeof(double);
  HostCall hc({{frames, fb}, {A, ab}}, {{out, fb}});
  if (hc.upload())
    hc.ran(launch_status(lspiv::launch_warp_affine(hc.in(0), dtype, T, (int)H, (int)W, hc.in<double>(1), hc.out(0), hc.stream())));
  return hc.finish(__func__);
}

}  // extern "C"
