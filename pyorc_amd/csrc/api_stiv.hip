// C ABI of liblspiv_hip.so, space-time image velocimetry (api_core.hip has the overview): the gather of the space-time images along
// the search lines and the orientation of their streaks, each as a "_dev" entry point on device pointers and as a host twin that stages
// through the context's workspaces (api_internal.h, HostCall).  pyorc has no counterpart; the semantics are this project's own
// (INTEGRATION.md section 2m).
#include "api_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "stiv.h"

namespace lspiv_api __attribute__((visibility("hidden"))) {

namespace {

int check_gather(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t S, int64_t L, const void* sti,
                 int64_t t_offset, int64_t T_total) {
  if (!frames || !points || !sti) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(check_frames("sti_gather", dtype, T, 1, H, W, 2));
  if (S < 1 || L < 3 || S > 0x7fffffff / L) return fail(LSPIV_EINVAL, "sti_gather: %lld lines of %lld samples (at least 3 per line)", (long long)S, (long long)L);
  if (t_offset < 0 || T_total > 0x7fffffff || t_offset > T_total - T)
    return fail(LSPIV_EINVAL, "sti_gather: rows [%lld, %lld) do not fit a space-time image of %lld rows", (long long)t_offset,
                (long long)(t_offset + T), (long long)T_total);
  return LSPIV_OK;
}

// The sample table [offset | fx | fy] of a call (stiv.h, StiTable) from the points (S, L, 2) = (x, y): ix = min(floor(x), W - 2),
// fx = float32(x - ix), so x = W - 1 has fx = 1 and nothing outside the frame is read.  A point that is not finite or lies outside
// [0, W - 1] x [0, H - 1] is an error that names it.
int sti_prepare_points(const double* points, int64_t S, int64_t L, int64_t H, int64_t W, std::vector<char>* table) {
  const int64_t n = S * L;
  table->resize(lspiv::sti_table_bytes(n));
  int32_t* off = (int32_t*)table->data();
  float* fx = (float*)(off + n);
  float* fy = fx + n;
  for (int64_t p = 0; p < n; ++p) {
    const double x = points[2 * p], y = points[2 * p + 1];
    if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1)))   // false for NaN as well
      return fail(LSPIV_EINVAL, "sti_gather: point %lld of line %lld at (%.17g, %.17g) is not inside the frame [0, %lld] x [0, %lld]",
                  (long long)(p % L), (long long)(p / L), x, y, (long long)(W - 1), (long long)(H - 1));
    const int64_t ix = std::min<int64_t>((int64_t)std::floor(x), W - 2), iy = std::min<int64_t>((int64_t)std::floor(y), H - 2);
    off[p] = (int32_t)(iy * W + ix);
    fx[p] = (float)(x - (double)ix);
    fy[p] = (float)(y - (double)iy);
  }
  return LSPIV_OK;
}

// The table into the context's scratch buffer on `s`.  The host vector is pageable memory: the copy has left it when the call returns.
// Like the other users of the scratch buffer (api_rows.hip, lspiv_normalize_dev), calls that overlap in time must share one stream.
int upload_table(DeviceCtx* c, const std::vector<char>& table, int64_t n, hipStream_t s, lspiv::StiTable* t) {
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, table.size()));
  HIP_TRY(hipMemcpyAsync(c->d_scratch, table.data(), table.size(), hipMemcpyHostToDevice, s));
  const int32_t* off = (const int32_t*)c->d_scratch;
  const float* fx = (const float*)(off + n);
  *t = lspiv::StiTable{off, fx, fx + n};
  return LSPIV_OK;
}

int check_orientation(const void* sti, int64_t S, int64_t T, int64_t L, int64_t Tw, int64_t stride, int smooth, const void* tensor,
                      const void* slope, const void* coherency, int64_t* K) {
  if (!sti || !tensor || !slope || !coherency) return fail(LSPIV_EINVAL, "NULL argument");
  if (smooth < 0 || smooth > lspiv::kStiMaxSmooth) return fail(LSPIV_EINVAL, "sti_orientation: smooth %d outside 0 .. %d", smooth, lspiv::kStiMaxSmooth);
  if (S < 1 || T < 1 || L < 1 || L > 0x7fffffff || T > 0x7fffffff)
    return fail(LSPIV_EINVAL, "sti_orientation: bad shape (%lld, %lld, %lld)", (long long)S, (long long)T, (long long)L);
  const int n = 2 * smooth + 3;
  if (L < n) return fail(LSPIV_EINVAL, "sti_orientation: %lld samples per line, smooth %d needs %d", (long long)L, smooth, n);
  if (Tw < n || Tw > T) return fail(LSPIV_EINVAL, "sti_orientation: time_window %lld outside %d .. %lld (smooth %d)", (long long)Tw, n, (long long)T, smooth);
  if (stride < 1) return fail(LSPIV_EINVAL, "sti_orientation: time_stride %lld < 1", (long long)stride);
  *K = (T - Tw) / stride + 1;
  if (S > 0x7fffffff / *K) return fail(LSPIV_EINVAL, "sti_orientation: %lld lines x %lld windows", (long long)S, (long long)*K);
  return LSPIV_OK;
}

}  // namespace

}  // namespace lspiv_api

using namespace lspiv_api;

extern "C" {

int lspiv_sti_gather_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t S, int64_t L,
                         float* d_sti, int64_t t_offset, int64_t T_total, void* stream) {
  LSPIV_TRY(check_gather(d_frames, dtype, T, H, W, points, S, L, d_sti, t_offset, T_total));
  std::vector<char> table;
  LSPIV_TRY(sti_prepare_points(points, S, L, H, W, &table));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  lspiv::StiTable t;
  LSPIV_TRY(upload_table(c, table, S * L, s, &t));
  return launch_status(lspiv::launch_sti_gather(d_frames, dtype, T, (int)H, (int)W, t, S, (int)L, d_sti, t_offset, T_total, s));
}

int lspiv_sti_gather(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t S, int64_t L, float* sti,
                     int64_t t_offset, int64_t T_total) {
  LSPIV_TRY(check_gather(frames, dtype, T, H, W, points, S, L, sti, t_offset, T_total));
  std::vector<char> table;
  LSPIV_TRY(sti_prepare_points(points, S, L, H, W, &table));
  // the frames a chunk at a time through one slot; the rows of this call, (S, T, L), gathered in another and sent to their lines' rows
  const size_t frame_bytes = (size_t)H * W * elem_size(dtype), row_bytes = (size_t)T * L * sizeof(float);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)(host_chunk_bytes() / frame_bytes)));
  HostCall hc({{frames, (size_t)chunk * frame_bytes, /*copy=*/false}}, {{sti, (size_t)S * row_bytes, -1, /*copy=*/false}});
  lspiv::StiTable t;
  if (hc.ok()) hc.ran(upload_table(hc.ctx(), table, S * L, hc.stream(), &t));
  for (int64_t f0 = 0; f0 < T && hc.ok(); f0 += chunk) {
    const int64_t n = std::min(chunk, T - f0);
    if (hc.copy_in(hc.in(0), (const char*)frames + (size_t)f0 * frame_bytes, (size_t)n * frame_bytes))
      hc.ran(launch_status(lspiv::launch_sti_gather(hc.in(0), dtype, n, (int)H, (int)W, t, S, (int)L, hc.out<float>(0), f0, T, hc.stream())));
  }
  for (int64_t line = 0; line < S && hc.ok(); ++line)
    hc.copy_out(sti + (line * T_total + t_offset) * L, hc.out<float>(0) + line * T * L, row_bytes);
  return hc.finish(__func__);
}

int lspiv_sti_orientation_dev(const float* d_sti, int64_t S, int64_t T, int64_t L, int64_t time_window, int64_t time_stride, int smooth,
                              int detrend, double* d_tensor, double* d_slope, double* d_coherency, void* stream) {
  int64_t K;
  LSPIV_TRY(check_orientation(d_sti, S, T, L, time_window, time_stride, smooth, d_tensor, d_slope, d_coherency, &K));
  return launch_on(stream, [&](hipStream_t s) {
    return lspiv::launch_sti_orientation(d_sti, S, T, (int)L, time_window, time_stride, K, smooth, detrend != 0, d_tensor, d_slope, d_coherency, s);
  });
}

int lspiv_sti_orientation(const float* sti, int64_t S, int64_t T, int64_t L, int64_t time_window, int64_t time_stride, int smooth, int detrend,
                          double* tensor, double* slope, double* coherency) {
  int64_t K;
  LSPIV_TRY(check_orientation(sti, S, T, L, time_window, time_stride, smooth, tensor, slope, coherency, &K));
  const size_t sb = (size_t)S * T * L * sizeof(float), nb = (size_t)S * K * sizeof(double);
  HostCall hc({{sti, sb}}, {{tensor, 3 * nb}, {slope, nb}, {coherency, nb}});
  if (hc.upload())
    hc.ran(launch_status(lspiv::launch_sti_orientation(hc.in<float>(0), S, T, (int)L, time_window, time_stride, K, smooth, detrend != 0,
                                                       hc.out<double>(0), hc.out<double>(1), hc.out<double>(2), hc.stream())));
  return hc.finish(__func__);
}

}  // extern "C"
