// C ABI of liblspiv_hip.so, pyramidal Lucas-Kanade point tracking (api_core.hip has the overview): the Gaussian pyramid step and the
// tracker, each as a "_dev" entry point on device pointers and as a host twin that stages through the context's workspaces
// (api_internal.h, HostCall).  The semantics are this project's own (tests/track_ref.py).
#include "api_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "track.h"

namespace lspiv_api __attribute__((visibility("hidden"))) {

int check_frames(const char* what, int dtype, int64_t T, int64_t T_min, int64_t H, int64_t W, int64_t side_min) {
  if (dtype != LSPIV_U8 && dtype != LSPIV_F32) return fail(LSPIV_EINVAL, "%s: dtype %d not in {0:u8, 1:f32}", what, dtype);
  if (T < T_min || T > 0x7fffffff || H < side_min || W < side_min || H > 32767 || W > 32767)
    return fail(LSPIV_EINVAL, "%s: bad shape (%lld, %lld, %lld) (at least %lld frames, sides %lld .. 32767)", what, (long long)T, (long long)H,
                (long long)W, (long long)T_min, (long long)side_min);
  return LSPIV_OK;
}

namespace {

constexpr size_t kTrackWsDefault = (size_t)1 << 30;      // the pyramid workspace's cap; LSPIV_TRACK_WS_BYTES (a test hook) overrides it

// The pyramid levels >= 1 of the frames of one batch of pairs: library-owned, per device, grow-only up to the cap.  Calls are issued
// under the lock; "_dev" calls that overlap in time share one stream (as with the scratch buffer of lspiv_sti_gather_dev).
struct TrackWs { void* p = nullptr; size_t cap = 0; std::mutex lock; };
TrackWs g_track_ws[kMaxDevices];

size_t ws_limit() { return env_bytes("LSPIV_TRACK_WS_BYTES", kTrackWsDefault); }

int check_stack(const char* what, const void* frames, int dtype, int64_t T, int64_t T_min, int64_t H, int64_t W, int levels) {
  if (!frames) return fail(LSPIV_EINVAL, "NULL argument");
  if (levels < 1 || levels > lspiv::kTrackMaxLevels) return fail(LSPIV_EINVAL, "%s: levels %d outside 1 .. %d", what, levels, lspiv::kTrackMaxLevels);
  LSPIV_TRY(check_frames(what, dtype, T, T_min, H, W, 1));
  // a level that pyr_down reads needs both sides >= 3 (the reflection -1 -> 1, n -> n - 2), every level both >= 2
  int64_t h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    const int64_t need = l < levels - 1 ? 3 : 2;
    if (h < need || w < need)
      return fail(LSPIV_EINVAL, "%s: level %d of a %lld x %lld frame is %lld x %lld, below %lld x %lld: too small for %d levels", what, l,
                  (long long)H, (long long)W, (long long)h, (long long)w, (long long)need, (long long)need, levels);
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  return LSPIV_OK;
}

struct TrackCall {
  int dtype; int64_t T, H, W, N;
  const double* points; int points_per_pair;
  const double* guess; int guess_per_pair;
  int window, levels, max_iter; double eps, min_eig; int chain;
  double *u, *v, *err, *lam; int32_t* n_iter; uint8_t* status; double* xy;
};

int check_track(const TrackCall& a, const void* frames) {
  LSPIV_TRY(check_stack("lk_track", frames, a.dtype, a.T, 2, a.H, a.W, a.levels));
  if (!a.points || !a.u || !a.v || !a.err || !a.lam || !a.n_iter || !a.status) return fail(LSPIV_EINVAL, "NULL argument");
  if (a.window < lspiv::kTrackMinWindow || a.window > lspiv::kTrackMaxWindow || a.window % 2 == 0)
    return fail(LSPIV_EINVAL, "lk_track: window %d is not odd in %d .. %d", a.window, lspiv::kTrackMinWindow, lspiv::kTrackMaxWindow);
  if (a.max_iter < 1 || a.max_iter > lspiv::kTrackMaxIter) return fail(LSPIV_EINVAL, "lk_track: max_iter %d outside 1 .. %d", a.max_iter, lspiv::kTrackMaxIter);
  if (!(a.eps >= 0.0) || !std::isfinite(a.eps)) return fail(LSPIV_EINVAL, "lk_track: eps %g must be >= 0", a.eps);
  if (!(a.min_eig >= 0.0) || !std::isfinite(a.min_eig)) return fail(LSPIV_EINVAL, "lk_track: min_eig %g must be >= 0", a.min_eig);
  if (a.N < 1 || a.N > 0x7fffffff / (a.T - 1) / 2) return fail(LSPIV_EINVAL, "lk_track: %lld points x %lld pairs", (long long)a.N, (long long)(a.T - 1));
  if (a.chain && (!a.xy || a.points_per_pair))
    return fail(LSPIV_EINVAL, "lk_track: a chain starts from one set of points (points_per_pair = 0) and needs xy (T, N, 2)");
  return LSPIV_OK;
}

// Pairs [p0, p0 + n) of the run on `s`; d_frames holds frames p0 .. p0 + n.  Every pointer of `a` is a device pointer to the WHOLE run's
// array.  The pyramid of a batch of pairs (one more frame than pairs: the halo) is built in the workspace, then the batch is tracked;
// every pair stands alone, so the batches give the bits of one launch.
int run_pairs(const TrackCall& a, const void* d_frames, int64_t p0, int64_t n, hipStream_t s) {
  lspiv::LkParams p{};
  int64_t level_elems[lspiv::kTrackMaxLevels] = {0};
  int64_t per_frame = 0;   // float32 samples of levels >= 1 of one frame
  p.H[0] = (int)a.H; p.W[0] = (int)a.W;
  for (int l = 1; l < a.levels; ++l) {
    p.H[l] = (p.H[l - 1] + 1) / 2; p.W[l] = (p.W[l - 1] + 1) / 2;
    level_elems[l] = (int64_t)p.H[l] * p.W[l];
    per_frame += level_elems[l];
  }
  p.N = (int)a.N; p.levels = a.levels; p.max_iter = a.max_iter; p.eps2 = a.eps * a.eps; p.min_eig = a.min_eig;
  p.points_stride = a.points_per_pair ? 2 * a.N : 0;
  p.guess_stride = a.guess_per_pair ? 2 * a.N : 0;
  int64_t batch = n;
  TrackWs& ws = g_track_ws[current_device_slot()];
  std::lock_guard<std::mutex> ws_lock(ws.lock);
  if (per_frame) {
    const int64_t fit = std::max<int64_t>(2, (int64_t)(ws_limit() / ((size_t)per_frame * sizeof(float))));
    batch = std::min<int64_t>(n, fit - 1);
    LSPIV_TRY(ensure(&ws.p, &ws.cap, (size_t)(batch + 1) * per_frame * sizeof(float)));
  }
  const size_t frame_bytes = (size_t)a.H * a.W * elem_size(a.dtype);
  for (int64_t b0 = 0; b0 < n; b0 += batch) {
    const int64_t nb = std::min(batch, n - b0), nf = nb + 1, g0 = p0 + b0;   // g0: the batch's first pair in the run
    const void* src = (const char*)d_frames + (size_t)b0 * frame_bytes;
    float* lvl = (float*)ws.p;
    const void* from = src;
    for (int l = 1; l < a.levels; ++l) {
      LSPIV_TRY(launch_status(lspiv::launch_pyr_down(from, l == 1 ? a.dtype : LSPIV_F32, nf, p.H[l - 1], p.W[l - 1], lvl, s)));
      p.pyr[l] = lvl;
      from = lvl;
      lvl += nf * level_elems[l];
    }
    p.frames = src;
    const int64_t launches = a.chain ? nb : 1;
    for (int64_t k = 0; k < launches; ++k) {   // a chain: pair after pair in stream order, each from the row the last one wrote
      lspiv::LkParams q = p;
      const int64_t g = g0 + k, o = g * a.N;
      q.n_pairs = a.chain ? 1 : nb;
      q.frames = (const char*)src + (size_t)k * frame_bytes;
      for (int l = 1; l < a.levels; ++l) q.pyr[l] = p.pyr[l] + k * level_elems[l];
      q.points = a.chain ? a.xy + 2 * o : a.points + g * p.points_stride;
      q.guess = a.guess ? a.guess + g * p.guess_stride : nullptr;
      q.u = a.u + o; q.v = a.v + o; q.err = a.err + o; q.lam = a.lam + o; q.n_iter = a.n_iter + o; q.status = a.status + o;
      q.next = a.chain ? a.xy + 2 * (o + a.N) : nullptr;
      LSPIV_TRY(launch_status(lspiv::launch_lk_track(q, a.dtype, a.window, s)));
    }
  }
  return LSPIV_OK;
}

}  // namespace

}  // namespace lspiv_api

using namespace lspiv_api;

extern "C" {

int lspiv_pyr_down_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, float* d_out, void* stream) {
  LSPIV_TRY(check_stack("pyr_down", d_frames, dtype, T, 1, H, W, 2));
  if (!d_out) return fail(LSPIV_EINVAL, "NULL argument");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_pyr_down(d_frames, dtype, T, (int)H, (int)W, d_out, s); });
}

int lspiv_pyr_down(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, float* out) {
  LSPIV_TRY(check_stack("pyr_down", frames, dtype, T, 1, H, W, 2));
  if (!out) return fail(LSPIV_EINVAL, "NULL argument");
  const size_t in_bytes = (size_t)T * H * W * elem_size(dtype), out_bytes = (size_t)T * ((H + 1) / 2) * ((W + 1) / 2) * sizeof(float);
  return host_roundtrip(__func__, {frames, in_bytes}, {out, out_bytes}, [&](void* d_in, void* d_o, hipStream_t s) {
    return launch_status(lspiv::launch_pyr_down(d_in, dtype, T, (int)H, (int)W, (float*)d_o, s));
  });
}

int lspiv_lk_track_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* d_points, int64_t N, int points_per_pair,
                       const double* d_guess, int guess_per_pair, int window, int levels, int max_iter, double eps, double min_eig, int chain,
                       double* d_u, double* d_v, double* d_err, double* d_min_eig, int32_t* d_n_iter, uint8_t* d_status, double* d_xy,
                       void* stream) {
  const TrackCall a{dtype, T, H, W, N, d_points, points_per_pair, d_guess, guess_per_pair, window, levels, max_iter, eps, min_eig, chain,
                    d_u, d_v, d_err, d_min_eig, d_n_iter, d_status, d_xy};
  LSPIV_TRY(check_track(a, d_frames));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  if (chain) HIP_TRY(hipMemcpyAsync(d_xy, d_points, (size_t)N * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));   // row 0
  return run_pairs(a, d_frames, 0, T - 1, s);
}

int lspiv_lk_track(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t N, int points_per_pair,
                   const double* guess, int guess_per_pair, int window, int levels, int max_iter, double eps, double min_eig, int chain, double* u,
                   double* v, double* err, double* min_eig_out, int32_t* n_iter, uint8_t* status, double* xy) {
  TrackCall a{dtype, T, H, W, N, points, points_per_pair, guess, guess_per_pair, window, levels, max_iter, eps, min_eig, chain,
              u, v, err, min_eig_out, n_iter, status, xy};
  LSPIV_TRY(check_track(a, frames));
  const int64_t P = T - 1;
  const size_t frame_bytes = (size_t)H * W * elem_size(dtype);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(host_chunk_bytes() / frame_bytes) - 1));   // pairs per upload
  const size_t pb = (size_t)(points_per_pair ? P : 1) * N * 2 * sizeof(double), gb = (size_t)(guess_per_pair ? P : 1) * N * 2 * sizeof(double);
  const size_t ob = (size_t)P * N * sizeof(double), xb = (size_t)T * N * 2 * sizeof(double);
  HostCall hc({{points, pb}, {guess, gb}, {frames, (size_t)(chunk + 1) * frame_bytes, /*copy=*/false}},
              {{u, ob}, {v, ob}, {err, ob}, {min_eig_out, ob}, {n_iter, (size_t)P * N * sizeof(int32_t)}, {status, (size_t)P * N}, {chain ? xy : nullptr, xb}});
  a.points = hc.in<double>(0); a.guess = hc.in<double>(1);
  a.u = hc.out<double>(0); a.v = hc.out<double>(1); a.err = hc.out<double>(2); a.lam = hc.out<double>(3);
  a.n_iter = hc.out<int32_t>(4); a.status = hc.out<uint8_t>(5); a.xy = hc.out<double>(6);
  if (hc.upload() && chain) hc.copy(a.xy, a.points, (size_t)N * 2 * sizeof(double), hipMemcpyDeviceToDevice);   // row 0
  for (int64_t p0 = 0; p0 < P && hc.ok(); p0 += chunk) {   // frames p0 .. p0 + n: one frame of halo
    const int64_t n = std::min(chunk, P - p0);
    if (hc.copy_in(hc.in(2), (const char*)frames + (size_t)p0 * frame_bytes, (size_t)(n + 1) * frame_bytes)) hc.ran(run_pairs(a, hc.in(2), p0, n, hc.stream()));
  }
  return hc.finish(__func__);
}

}  // extern "C"
