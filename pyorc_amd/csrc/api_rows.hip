// C ABI of liblspiv_hip.so, the row entry points (api_core.hip has the overview): post-PIV masks, element-wise filters, normalize,
// reduce_rolling and the Gaussian filters, each as a "_dev" entry point on device pointers and, through HostCall (api_internal.h), on host
// ones.
#include "api_internal.h"

#include <cmath>
#include <cstdlib>

#include "project_tile.h"   // launch_blur_clip
#include "validate.h"

namespace lspiv_api __attribute__((visibility("hidden"))) {

// the frame-stack check of a filter's host entry point and its "_dev" twin: buffers, dtype, at least min_frames frames
static int check_stack(const void* in, const void* out, int dtype, int64_t T, int64_t H, int64_t W, int min_frames) {
  if (!in || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < min_frames || H <= 0 || W <= 0)
    return fail(LSPIV_ESHAPE, "need >= %d frame%s of positive size", min_frames, min_frames > 1 ? "s" : "");
  return LSPIV_OK;
}

// Frames.normalize's sampling interval round(T / samples), Python rounding (half to even); 0 = too few frames
static long normalize_interval(int64_t T, int samples) {
  const double ratio = (double)T / (double)samples;
  long iv = std::lround(ratio);
  if (ratio - std::floor(ratio) == 0.5) iv = ((long)std::floor(ratio) % 2 == 0) ? (long)std::floor(ratio) : (long)std::floor(ratio) + 1;
  return iv;
}

static int blur_common_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int k1, int k2, float* d_out,
                           void* stream, float lo = -INFINITY, float hi = INFINITY) {
  if (!d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < 1 || H <= 0 || W <= 0 || T > 65535 || H >= (1 << 30) || W >= (1 << 30)) return fail(LSPIV_ESHAPE, "bad shape");
  for (int k : {k1, k2})
    if (k != 0 && (k < 1 || k > 31 || k % 2 == 0)) return fail(LSPIV_EINVAL, "kernel size %d must be odd, 1..31", k);
  if (k1 == 0) return fail(LSPIV_EINVAL, "kernel size missing");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_blur_clip(d_frames, dtype, (int)T, (int)H, (int)W, k1, k2, lo, hi, d_out, s); });
}

static int blur_common_host(const char* name, const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int k1, int k2, float* out) {
  if (!frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2 || T < 1 || H <= 0 || W <= 0) return fail(LSPIV_EINVAL, "bad argument");
  const size_t ib = (size_t)T * H * W * elem_size(dtype), ob = (size_t)T * H * W * sizeof(float);
  return host_roundtrip(name, {frames, ib}, {out, ob}, [&](void* d_in, void* d_out, hipStream_t s) {
    return blur_common_dev(d_in, dtype, T, H, W, k1, k2, (float*)d_out, s);
  });
}

}  // namespace lspiv_api

using namespace lspiv_api;

extern "C" {

// ---- post-PIV masks (N3) ------------------------------------------------------------------------------
namespace {
const int kMaskParams[10] = {2, 2, 1, 1, 1, 2, 2, 2, 5, 6};
bool mask_is_2d(int kind) { return kind == LSPIV_MASK_COUNT || kind == LSPIV_MASK_VARIANCE; }

// a stack of fields `f` and the other buffer of the call
int check_fields(const void* f, const void* other, int64_t T, int64_t R, int64_t C) {
  if (!f) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || R < 1 || C < 1 || R >= (1 << 30) || C >= (1 << 30) || T * R * C >= ((int64_t)1 << 40))
    return fail(LSPIV_ESHAPE, "bad field shape (%lld, %lld, %lld)", (long long)T, (long long)R, (long long)C);
  if (!other) return fail(LSPIV_EINVAL, "NULL argument");
  return LSPIV_OK;
}
}  // namespace

int lspiv_mask_dev(const float* d_fields, int64_t T, int64_t R, int64_t C, int kind, const double* params, int n_params,
                   uint8_t* d_mask, void* stream) {
  LSPIV_TRY(check_fields(d_fields, d_mask, T, R, C));
  if (!params) return fail(LSPIV_EINVAL, "NULL argument");
  if (kind < 0 || kind > 9) return fail(LSPIV_EINVAL, "unknown mask kind %d", kind);
  if (n_params != kMaskParams[kind]) return fail(LSPIV_EINVAL, "mask kind %d takes %d parameters, got %d", kind, kMaskParams[kind], n_params);
  if (kind == LSPIV_MASK_ROLLING && (params[0] < 1 || params[0] > 1e6)) return fail(LSPIV_EINVAL, "rolling window must be >= 1");
  if (kind >= LSPIV_MASK_WINDOW_NAN) {
    const double* w = params + (kind == LSPIV_MASK_WINDOW_NAN ? 1 : 2);
    for (int i = 0; i < 4; ++i)
      if (!(std::fabs(w[i]) <= 1024)) return fail(LSPIV_EINVAL, "window stride %g out of range", w[i]);
  }
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_mask(d_fields, T, (int)R, (int)C, kind, params, d_mask, s); });
}

int lspiv_mask(const float* fields, int64_t T, int64_t R, int64_t C, int kind, const double* params, int n_params,
               uint8_t* mask) {
  LSPIV_TRY(check_fields(fields, mask, T, R, C));
  const size_t fb = (size_t)4 * T * R * C * sizeof(float), mb = (size_t)(mask_is_2d(kind) ? 1 : T) * R * C;
  return host_roundtrip(__func__, {fields, fb}, {mask, mb}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_mask_dev((const float*)d_in, T, R, C, kind, params, n_params, (uint8_t*)d_out, s);
  });
}

int lspiv_mask_apply_dev(float* d_fields, int64_t T, int64_t R, int64_t C, const uint8_t* d_mask, int mask_has_time,
                         void* stream) {
  LSPIV_TRY(check_fields(d_fields, d_mask, T, R, C));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_mask_apply(d_fields, T, R * C, d_mask, mask_has_time != 0, s); });
}

int lspiv_mask_apply(float* fields, int64_t T, int64_t R, int64_t C, const uint8_t* mask, int mask_has_time) {
  LSPIV_TRY(check_fields(fields, mask, T, R, C));
  const size_t fb = (size_t)4 * T * R * C * sizeof(float), mb = (size_t)(mask_has_time ? T : 1) * R * C;
  return host_roundtrip(__func__, {fields, fb}, {fields, fb, /*in=*/0}, [&](void* d_fields, void* d_mask, hipStream_t s) {
    return lspiv_mask_apply_dev((float*)d_fields, T, R, C, (const uint8_t*)d_mask, mask_has_time, s);
  }, /*aux=*/{mask, mb});
}

int lspiv_time_mean_dev(const float* d_fields, int64_t T, int64_t R, int64_t C, float* d_out, void* stream) {
  LSPIV_TRY(check_fields(d_fields, d_out, T, R, C));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_time_mean(d_fields, T, R * C, d_out, s); });
}

int lspiv_time_mean(const float* fields, int64_t T, int64_t R, int64_t C, float* out) {
  LSPIV_TRY(check_fields(fields, out, T, R, C));
  const size_t fb = (size_t)4 * T * R * C * sizeof(float), ob = (size_t)4 * R * C * sizeof(float);
  return host_roundtrip(__func__, {fields, fb}, {out, ob}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_time_mean_dev((const float*)d_in, T, R, C, (float*)d_out, s);
  });
}

int lspiv_window_replace_dev(float* d_fields, int64_t T, int64_t R, int64_t C, int x_min, int x_max, int y_min,
                             int y_max, int iter, void* stream) {
  LSPIV_TRY(check_fields(d_fields, d_fields, T, R, C));
  if (iter < 0 || std::abs(x_min) > 1024 || std::abs(x_max) > 1024 || std::abs(y_min) > 1024 || std::abs(y_max) > 1024)
    return fail(LSPIV_EINVAL, "bad window / iteration count");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const size_t fb = (size_t)4 * T * R * C * sizeof(float);
  float* d_tmp = nullptr;
  HIP_TRY(hipMalloc((void**)&d_tmp, fb));
  hipError_t e = hipSuccess;
  float *src = d_fields, *dst = d_tmp;
  for (int i = 0; i < iter && e == hipSuccess; ++i) {
    e = lspiv::launch_window_replace(src, 4 * T, (int)R, (int)C, x_min, x_max, y_min, y_max, dst, s);
    std::swap(src, dst);
  }
  if (e == hipSuccess && src != d_fields) e = hipMemcpyAsync(d_fields, src, fb, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the temporary is freed below
  hipFree(d_tmp);
  return launch_status(e, "window_replace failed");
}

int lspiv_window_replace(float* fields, int64_t T, int64_t R, int64_t C, int x_min, int x_max, int y_min, int y_max,
                         int iter) {
  LSPIV_TRY(check_fields(fields, fields, T, R, C));
  const size_t fb = (size_t)4 * T * R * C * sizeof(float);
  return host_roundtrip(__func__, {fields, fb}, {fields, fb, /*in=*/0}, [&](void* d_fields, void*, hipStream_t s) {
    return lspiv_window_replace_dev((float*)d_fields, T, R, C, x_min, x_max, y_min, y_max, iter, s);
  });
}

int lspiv_scale_velocity_dev(float* d_fields, int64_t T, int64_t n_vec, double res_x, double res_y, const double* dt,
                             void* stream) {
  if (!d_fields || !dt) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || n_vec < 1) return fail(LSPIV_ESHAPE, "bad shape");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  double* d_dt = nullptr;
  HIP_TRY(hipMalloc((void**)&d_dt, (size_t)T * sizeof(double)));
  hipError_t e = hipMemcpyAsync(d_dt, dt, (size_t)T * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = lspiv::launch_scale_velocity(d_fields, T, n_vec, (float)res_x, (float)res_y, d_dt, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // dt is a host array and the temporary is freed below
  hipFree(d_dt);
  return launch_status(e, "scale_velocity failed");
}

// ---- vector validation (normalised median test, runner-up substitution) ---------------------------------
namespace {
int check_validate(const void* u, const void* v, int64_t T, int64_t R, int64_t C, float threshold, float epsilon, int min_neighbours,
                   int replace, int iterations) {
  if (!u || !v) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || R < 1 || C < 1) return fail(LSPIV_EINVAL, "bad field shape (%lld, %lld, %lld)", (long long)T, (long long)R, (long long)C);
  if (R >= (1 << 30) || C >= (1 << 30) || T >= ((int64_t)1 << 38) || T * R * C >= ((int64_t)1 << 38))
    return fail(LSPIV_ESHAPE, "field shape (%lld, %lld, %lld) too large", (long long)T, (long long)R, (long long)C);
  if (!(threshold > 0.0f) || std::isinf(threshold)) return fail(LSPIV_EINVAL, "threshold %g must be a positive number", threshold);
  if (!(epsilon >= 0.0f) || std::isinf(epsilon)) return fail(LSPIV_EINVAL, "epsilon %g must be a number >= 0", epsilon);
  if (min_neighbours < 1 || min_neighbours > 8) return fail(LSPIV_EINVAL, "min_neighbours %d not in 1 .. 8", min_neighbours);
  if (replace != LSPIV_VALIDATE_NAN && replace != LSPIV_VALIDATE_MEDIAN) return fail(LSPIV_EINVAL, "unknown replace mode %d", replace);
  if (iterations < 1 || iterations > 8) return fail(LSPIV_EINVAL, "iterations %d not in 1 .. 8", iterations);
  return LSPIV_OK;
}
}  // namespace

int lspiv_validate_dev(float* d_u, float* d_v, const float* d_peak2, int64_t T, int64_t R, int64_t C, float threshold, float epsilon,
                       int min_neighbours, int replace, int iterations, uint8_t* d_flag, void* stream) {
  LSPIV_TRY(check_validate(d_u, d_v, T, R, C, threshold, epsilon, min_neighbours, replace, iterations));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const int64_t N = T * R * C;
  const size_t fb = (((size_t)N * sizeof(float)) + 255) & ~(size_t)255;
  // every iteration reads the field of the one before it: the fields ping-pong between the caller's buffers and the workspace, arranged
  // so that the last iteration writes the caller's (an odd count starts from a copy in the workspace); a lane owns its flag
  std::lock_guard<std::mutex> ws_lock(locks_here().validate);
  if (!c->validate_done) HIP_TRY(hipEventCreateWithFlags(&c->validate_done, hipEventDisableTiming));
  else HIP_TRY(hipStreamWaitEvent(s, c->validate_done, 0));
  if (2 * fb + (size_t)N > c->validate_cap) HIP_TRY(hipEventSynchronize(c->validate_done));   // (a never-recorded event is complete)
  LSPIV_TRY(ensure(&c->d_validate, &c->validate_cap, 2 * fb + (size_t)N));
  float *w_u = (float*)c->d_validate, *w_v = (float*)((char*)c->d_validate + fb);
  uint8_t* flag = d_flag ? d_flag : (uint8_t*)c->d_validate + 2 * fb;
  const lspiv::ValidateParams p{threshold, epsilon, min_neighbours, replace};
  hipError_t e = hipSuccess;
  bool in_ws = false;   // where the current field is
  if (iterations % 2) {
    e = hipMemcpyAsync(w_u, d_u, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(w_v, d_v, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s);
    in_ws = true;
  }
  for (int it = 0; it < iterations && e == hipSuccess; ++it) {
    e = in_ws ? lspiv::launch_validate(w_u, w_v, d_peak2, T, (int)R, (int)C, p, it == 0, d_u, d_v, flag, s)
              : lspiv::launch_validate(d_u, d_v, d_peak2, T, (int)R, (int)C, p, it == 0, w_u, w_v, flag, s);
    in_ws = !in_ws;
  }
  const hipError_t rec = hipEventRecord(c->validate_done, s);
  return launch_status(e != hipSuccess ? e : rec, "validate failed");
}

int lspiv_validate(float* u, float* v, const float* peak2, int64_t T, int64_t R, int64_t C, float threshold, float epsilon,
                   int min_neighbours, int replace, int iterations, uint8_t* flag) {
  LSPIV_TRY(check_validate(u, v, T, R, C, threshold, epsilon, min_neighbours, replace, iterations));
  // the host twin: u, v and the flags work in place in their slots, the same kernels in between
  const size_t N = (size_t)T * R * C, fb = N * sizeof(float);
  HostCall hc({{u, fb}, {v, fb}, {peak2, 4 * fb}, {flag, N, /*copy=*/false}}, {{u, fb, 0}, {v, fb, 1}, {flag, N, 3}});
  if (hc.upload())
    hc.ran(lspiv_validate_dev(hc.in<float>(0), hc.in<float>(1), hc.in<float>(2), T, R, C, threshold, epsilon, min_neighbours, replace, iterations,
                              hc.in<uint8_t>(3), hc.stream()));
  return hc.finish(__func__);
}

// ---- element-wise filters (N2) ---------------------------------------------------------------------
int lspiv_time_diff_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, float thres, int use_abs,
                        float* d_out, void* stream) {
  LSPIV_TRY(check_stack(d_frames, d_out, dtype, T, H, W, 2));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_time_diff(d_frames, dtype, H * W, T, thres, use_abs, d_out, s); });
}

int lspiv_time_diff(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, float thres, int use_abs, float* out) {
  LSPIV_TRY(check_stack(frames, out, dtype, T, H, W, 2));
  const size_t ib = (size_t)T * H * W * elem_size(dtype), ob = (size_t)(T - 1) * H * W * sizeof(float);
  return host_roundtrip(__func__, {frames, ib}, {out, ob}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_time_diff_dev(d_in, dtype, T, H, W, thres, use_abs, (float*)d_out, s);
  });
}

int lspiv_time_range_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, void* d_out, void* stream) {
  LSPIV_TRY(check_stack(d_frames, d_out, dtype, T, H, W, 1));
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_time_range(d_frames, dtype, H * W, T, d_out, s); });
}

int lspiv_time_range(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, void* out) {
  LSPIV_TRY(check_stack(frames, out, dtype, T, H, W, 1));
  const size_t ib = (size_t)T * H * W * elem_size(dtype), ob = (size_t)H * W * elem_size(dtype);
  return host_roundtrip(__func__, {frames, ib}, {out, ob}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_time_range_dev(d_in, dtype, T, H, W, d_out, s);
  });
}

int lspiv_minmax_dev(const float* d_frames, int64_t n, float lo, float hi, float* d_out, void* stream) {
  if (!d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (n < 0) return fail(LSPIV_EINVAL, "bad n");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_minmax(d_frames, n, lo, hi, d_out, s); });
}

int lspiv_minmax(const float* frames, int64_t n, float lo, float hi, float* out) {
  if (!frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (n <= 0) return n == 0 ? LSPIV_OK : fail(LSPIV_EINVAL, "bad n");
  const size_t b = (size_t)n * sizeof(float);
  return host_roundtrip(__func__, {frames, b}, {out, b, /*in=*/0}, [&](void* d_buf, void*, hipStream_t s) {
    return lspiv_minmax_dev((const float*)d_buf, n, lo, hi, (float*)d_buf, s);   // in place, one workspace
  });
}

int lspiv_normalize_mean_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, float* d_mean, void* stream) {
  if (!d_frames || !d_mean) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0 || samples < 1 || T >= 65536) return fail(LSPIV_ESHAPE, "bad shape");
  const long iv = normalize_interval(T, samples);
  if (iv == 0) return fail(LSPIV_EINVAL, "Amount of frames is too small to provide %d samples", samples);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(lspiv::launch_sample_mean(d_frames, H * W, (int)T, (int)iv, d_mean, on_stream(c, stream)));
  return LSPIV_OK;
}

int lspiv_normalize_apply_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, const float* d_mean, uint8_t* d_out,
                              void* stream) {
  if (!d_frames || !d_mean || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0 || T >= 65536) return fail(LSPIV_ESHAPE, "bad shape");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t mm_bytes = ((size_t)2 * T * sizeof(int) + 255) & ~(size_t)255;
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, mm_bytes + lspiv::normalize_part_bytes(H * W, (int)T)));   // same-stream rule below
  int* d_mm = (int*)c->d_scratch;
  float* d_part = (float*)((char*)c->d_scratch + mm_bytes);
  return launch_status(lspiv::launch_normalize_apply(d_frames, H * W, (int)T, d_mean, d_mm, d_mm + T, d_part, d_out, on_stream(c, stream)),
                       "normalize failed", LSPIV_ENOMEM);
}

int lspiv_normalize_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* d_out, void* stream) {
  if (!d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0 || samples < 1 || T >= 65536) return fail(LSPIV_ESHAPE, "bad shape");
  const long iv = normalize_interval(T, samples);
  if (iv == 0) return fail(LSPIV_EINVAL, "Amount of frames is too small to provide %d samples", samples);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  // temporaries (mean plane + per-frame min / max) live in the context's grow-only scratch buffer: no allocation and
  // no synchronisation per call.  (hipMallocAsync / hipFreeAsync on this stream gave run-to-run different outputs on
  // ROCm 7.2 and were dropped.)  Calls that overlap in time must therefore be issued on one stream.
  const size_t mean_bytes = ((size_t)H * W * sizeof(float) + 255) & ~(size_t)255;
  const size_t mm_bytes = ((size_t)2 * T * sizeof(int) + 255) & ~(size_t)255;
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, mean_bytes + mm_bytes + lspiv::normalize_part_bytes(H * W, (int)T)));
  float* d_mean = (float*)c->d_scratch;
  int* d_mm = (int*)((char*)c->d_scratch + mean_bytes);
  float* d_part = (float*)((char*)c->d_scratch + mean_bytes + mm_bytes);
  return launch_status(lspiv::launch_normalize(d_frames, H * W, (int)T, (int)iv, d_mean, d_mm, d_mm + T, d_part, d_out, on_stream(c, stream)),
                       "normalize failed", LSPIV_ENOMEM);
}

int lspiv_normalize(const uint8_t* frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* out) {
  if (!frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0) return fail(LSPIV_ESHAPE, "bad shape");
  const size_t b = (size_t)T * H * W;
  return host_roundtrip(__func__, {frames, b}, {out, b}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_normalize_dev((const uint8_t*)d_in, T, H, W, samples, (uint8_t*)d_out, s);
  });
}

int lspiv_reduce_rolling_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* d_out, void* stream) {
  if (!d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0 || samples < 1 || T >= (1 << 24)) return fail(LSPIV_ESHAPE, "bad shape");
  if (T < samples) return fail(LSPIV_EINVAL, "Amount of frames is smaller than requested rolling of %d samples", samples);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, lspiv::reduce_rolling_scratch_bytes(H * W, (int)T)));
  return launch_status(lspiv::launch_reduce_rolling(d_frames, H * W, (int)T, samples, (double*)c->d_scratch, d_out, on_stream(c, stream)),
                       "reduce_rolling failed");
}

int lspiv_reduce_rolling(const uint8_t* frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* out) {
  if (!frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 1 || H <= 0 || W <= 0) return fail(LSPIV_ESHAPE, "bad shape");
  const size_t b = (size_t)T * H * W;
  return host_roundtrip(__func__, {frames, b}, {out, b}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_reduce_rolling_dev((const uint8_t*)d_in, T, H, W, samples, (uint8_t*)d_out, s);
  });
}

int lspiv_gaussian_blur(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize, float* out) {
  return blur_common_host(__func__, frames, dtype, T, H, W, ksize, 0, out);
}
int lspiv_gaussian_blur_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize, float* d_out,
                            void* stream) {
  return blur_common_dev(d_frames, dtype, T, H, W, ksize, 0, d_out, stream);
}
int lspiv_edge_detect(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2, float* out) {
  if (ksize_2 < ksize_1) return fail(LSPIV_EINVAL, "edge_detect expects ksize_2 >= ksize_1");
  return blur_common_host(__func__, frames, dtype, T, H, W, ksize_1, ksize_2, out);
}
int lspiv_edge_detect_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2,
                          float* d_out, void* stream) {
  if (ksize_2 < ksize_1) return fail(LSPIV_EINVAL, "edge_detect expects ksize_2 >= ksize_1");
  return blur_common_dev(d_frames, dtype, T, H, W, ksize_1, ksize_2, d_out, stream);
}

int lspiv_edge_detect_clip_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2, float lo,
                               float hi, float* d_out, void* stream) {
  if (ksize_2 < ksize_1) return fail(LSPIV_EINVAL, "edge_detect expects ksize_2 >= ksize_1");
  if (lo != lo || hi != hi) return fail(LSPIV_EINVAL, "NaN limit");
  return blur_common_dev(d_frames, dtype, T, H, W, ksize_1, ksize_2, d_out, stream, lo, hi);
}

}  // extern "C"
