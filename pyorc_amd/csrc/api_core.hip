// C ABI of liblspiv_hip.so (see include/lspiv.h for the contract and the reference call sites each entry point replaces).  Host
// logic only, split by subsystem: this file holds the device contexts, locks and trace, the run-time options, the device / memory
// / stream / event helpers, lspiv_upload_frames and the debug hooks; api_piv.hip, api_ensemble.hip, api_project.hip and
// api_rows.hip the entry points of their subsystems; api_version.hip the build provenance.  No PyTorch, no CPU compute fallback:
// without a gfx950 device every compute entry point fails with LSPIV_ENODEV.
#include "api_internal.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

namespace lspiv_api __attribute__((visibility("hidden"))) {

thread_local std::string g_err;

static int vfail(int code, const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof(buf), fmt, ap);
  g_err = buf;
  return code;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(code, fmt, ap);
  va_end(ap);
  return code;
}

// ---- per-device contexts and locks ------------------------------------------------------------------------------------------
std::mutex g_mu;        // the table of contexts itself (created lazily); never held while another lock is taken
std::vector<DeviceCtx*> g_ctx;
DeviceLocks g_locks[kMaxDevices];

int current_device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  return dev >= 0 && dev < kMaxDevices ? dev : 0;
}

int get_ctx(DeviceCtx** out) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(LSPIV_ENODEV, "no HIP device visible (%s)", hipGetErrorString(e));
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  if ((int)g_ctx.size() < ndev) g_ctx.resize(ndev, nullptr);
  if (!g_ctx[dev]) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(LSPIV_ENODEV, "device %d is %s; this library carries gfx950 (MI355X) code only", dev, prop.gcnArchName);
    DeviceCtx* c = new DeviceCtx();
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    c->arch_ok = true;
    g_ctx[dev] = c;
  }
  *out = g_ctx[dev];
  return LSPIV_OK;
}

// ---- trace ------------------------------------------------------------------------------------------------------------------
struct Trace { std::mutex mu; std::atomic<bool> on{false}; hipEvent_t base = nullptr; std::vector<TraceRec> recs; };
Trace g_trace[kMaxDevices];

TraceSpan::~TraceSpan() {
  if (r.e0) (void)hipEventDestroy(r.e0);
  if (r.e1) (void)hipEventDestroy(r.e1);
}
void trace_begin(TraceSpan* sp, int kind, hipStream_t s) {
  Trace& t = g_trace[current_device_slot()];
  if (!t.on.load()) return;
  sp->r.kind = kind;
  if (hipEventCreate(&sp->r.e0) != hipSuccess || hipEventCreate(&sp->r.e1) != hipSuccess) { (void)hipGetLastError(); return; }
  if (hipEventRecord(sp->r.e0, s) != hipSuccess) { (void)hipGetLastError(); return; }
  sp->t = &t;
}
void trace_end(TraceSpan* sp, hipStream_t s) {
  if (!sp->t) return;
  if (hipEventRecord(sp->r.e1, s) != hipSuccess) { (void)hipGetLastError(); return; }
  std::lock_guard<std::mutex> lk(sp->t->mu);
  sp->t->recs.push_back(sp->r);   // the trace owns the events from here
  sp->t = nullptr;
  sp->r = TraceRec{};
}

// ---- host staging -----------------------------------------------------------------------------------------------------------
bool is_pinned(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

int stage_ring(DeviceCtx* c, size_t frame_bytes) {
  const size_t want = getenv("LSPIV_STAGE_BYTES") ? (size_t)atoll(getenv("LSPIV_STAGE_BYTES")) : ((size_t)32 << 20);
  const size_t need = std::max(want, frame_bytes);
  if (c->pinned_cap >= need && c->pinned_cap < 2 * need + frame_bytes) return LSPIV_OK;
  for (int i = 0; i < 2; ++i) {
    if (c->pinned[i]) HIP_TRY(hipHostFree(c->pinned[i]));
    c->pinned[i] = nullptr;
  }
  c->pinned_cap = 0;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipHostMalloc(&c->pinned[i], need, hipHostMallocDefault));
    if (!c->staged[i]) HIP_TRY(hipEventCreateWithFlags(&c->staged[i], hipEventDisableTiming));
  }
  c->pinned_cap = need;
  return LSPIV_OK;
}

int stage_frames(DeviceCtx* c, int batch, void* d_dst, const void* frames, int dtype, bool src_pinned, size_t frame_elems,
                 int64_t f0, int64_t f1, float signal_threshold) {
  const int slot = batch & 1;
  if (batch >= 2) HIP_TRY(hipEventSynchronize(c->staged[slot]));  // the slot's previous DMA has drained
  const size_t frame_bytes = frame_elems * elem_size(dtype == LSPIV_F64 ? LSPIV_F32 : dtype), nb = (size_t)(f1 - f0) * frame_bytes;
  const char* src = (const char*)frames + (size_t)f0 * frame_elems * elem_size(dtype);
  const void* dma_src = c->pinned[slot];
  if (dtype == LSPIV_F64) {
    const std::vector<double> off = narrow_offsets((const double*)src, frame_elems, f1 - f0, signal_threshold);
    lspiv_host::staged_narrow((float*)c->pinned[slot], (const double*)src, frame_elems, (size_t)(f1 - f0), off.data());
  } else if (src_pinned)
    dma_src = src;   // caller's stack is pinned: no staging copy
  else
    staged_copy(c->pinned[slot], src, nb);
  HIP_TRY(hipMemcpyAsync((char*)d_dst + (size_t)f0 * frame_bytes, dma_src, nb, hipMemcpyHostToDevice, c->copy_stream));
  HIP_TRY(hipEventRecord(c->staged[slot], c->copy_stream));
  return LSPIV_OK;
}

// ---- run-time options -------------------------------------------------------------------------------------------------------
// LSPIV_BORDER_PEAK / LSPIV_SIGNAL_MODE / LSPIV_SIGNAL_POSITIVE / ... preset them
static int env_opt(const char* name, int lo, int hi) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return v < lo || v > hi ? 0 : v;
}
static int env_opt_def(const char* name, int lo, int hi, int def) {
  const char* e = getenv(name);
  if (!e) return def;
  const int v = atoi(e);
  return v < lo || v > hi ? def : v;
}
std::atomic<int> g_opt_border{env_opt("LSPIV_BORDER_PEAK", 0, 2)};
std::atomic<int> g_opt_signal_mode{env_opt("LSPIV_SIGNAL_MODE", 0, 1)};
std::atomic<int> g_opt_signal_pos{env_opt("LSPIV_SIGNAL_POSITIVE", 0, 1)};
std::atomic<int> g_opt_v_sign{env_opt("LSPIV_V_SIGN", 0, 1)};
std::atomic<int> g_opt_norm_clip{getenv("LSPIV_NORM_CLIP") && atoi(getenv("LSPIV_NORM_CLIP")) == 0 ? 0 : 1};
std::atomic<int> g_opt_std_ddof{env_opt("LSPIV_STD_DDOF", 0, 1)};
std::atomic<int> g_opt_round_odd{env_opt("LSPIV_ROUND_ODD", 0, 2)};
std::atomic<int> g_opt_rescue{env_opt_def("LSPIV_RESCUE", 0, 1, 1)};
std::atomic<int> g_opt_rescue_generic{env_opt("LSPIV_RESCUE_GENERIC", 0, 1)};
static std::atomic<int> g_opt_defer_fit{env_opt_def("LSPIV_DEFER_FIT", 0, 1, 1)};
static std::atomic<int> g_opt_unpack_dpp{env_opt_def("LSPIV_UNPACK_DPP_OPT", 0, 1, 1)};
static std::atomic<int> g_opt_lds_light{env_opt_def("LSPIV_LDS_LIGHT", 0, 1, 1)};
static std::atomic<int> g_opt_scalar_epilogue{env_opt_def("LSPIV_SCALAR_EPILOGUE", 0, 1, 1)};
std::atomic<int> g_rescue_fit_size{-1};
std::atomic<int> g_peaks_refitted{0};
std::atomic<int> g_opt_narrow_offset{env_opt_def("LSPIV_NARROW_OFFSET", -1, 1 << 30, 1024)};
std::atomic<int> g_opt_rescue_kappa{env_opt_def("LSPIV_RESCUE_KAPPA", 0, 1000000, 500)};
std::atomic<int> g_opt_rescue_tau{env_opt_def("LSPIV_RESCUE_TAU", 0, 1000000, 4000)};
std::atomic<int> g_opt_time_kernel{0};
static std::atomic<int> g_opt_walk{-1};   // lspiv_set_option("walk", v); -1: not set, fall back to the environment

std::vector<double> narrow_offsets(const double* frames, size_t frame_elems, int64_t n_frames, float signal_threshold) {
  std::vector<double> off((size_t)n_frames, 0.0);
  const int min_abs = g_opt_narrow_offset.load();
  if (min_abs < 0 || signal_threshold >= 0.0f) return off;
  for (int64_t f = 0; f < n_frames; ++f) off[(size_t)f] = lspiv_host::frame_offset(frames + (size_t)f * frame_elems, frame_elems, (double)min_abs);
  return off;
}

// the switches of lspiv_set_option / lspiv_get_option: name, value, accepted range, what the error says ("walk" apart)
struct Option { const char* name; std::atomic<int>* value; int lo, hi; const char* range; };
static const Option kOptions[] = {
    {"border_peak", &g_opt_border, 0, 2, "border_peak must be 0 (NaN), 1 (plane centre) or 2 (integer peak)"},
    {"signal_mode", &g_opt_signal_mode, 0, 1, "signal_mode must be 0 (per window pair) or 1 (per window position over the chunk)"},
    {"signal_positive", &g_opt_signal_pos, 0, 1, "signal_positive must be 0 (samples != 0) or 1 (samples > 0)"},
    {"v_sign", &g_opt_v_sign, 0, 1, "v_sign must be 0 (v = row shift of the peak) or 1 (negated)"},
    {"norm_clip", &g_opt_norm_clip, 0, 1, "norm_clip must be 1 (negative lobes of the normalised window removed) or 0"},
    {"std_ddof", &g_opt_std_ddof, 0, 1, "std_ddof must be 0 (population standard deviation) or 1 (sample)"},
    {"round_odd", &g_opt_round_odd, 0, 2, "round_odd must be 0 (half-even of x / 2), 1 (up) or 2 (down)"},
    {"rescue", &g_opt_rescue, 0, 1, "rescue must be 0 (float32 results as they are) or 1 (float64 rescue pass)"},
    {"defer_fit", &g_opt_defer_fit, 0, 1,
     "defer_fit must be 1 (32 x 32 walking kernels fit 32 planes at once) or 0 (every plane in its own iteration; same results)"},
    {"unpack_dpp", &g_opt_unpack_dpp, 0, 1,
     "unpack_dpp must be 1 (32 x 32 walking kernels exchange mirrored columns through DPP) or 0 (through LDS; same results)"},
    {"lds_light", &g_opt_lds_light, 0, 1,
     "lds_light must be 1 (32 x 32 walking kernels join the rows of their reductions with v_permlane16_swap) or 0 (ds_swizzle; same results)"},
    {"scalar_epilogue", &g_opt_scalar_epilogue, 0, 1,
     "scalar_epilogue must be 1 (32 x 32 walking kernels search the peak on ballots and the scalar unit) or 0 (in vector registers; same results)"},
    {"rescue_generic", &g_opt_rescue_generic, 0, 1,
     "rescue_generic must be 0 (fixed-size fit kernels for square 16 / 32 / 64 px windows) or 1 (run-time geometry for every launch)"},
    {"narrow_offset", &g_opt_narrow_offset, -1, INT_MAX,
     "narrow_offset must be -1 (never) or the smallest |DC offset| of a float64 frame that is removed while narrowing"},
    {"rescue_kappa", &g_opt_rescue_kappa, 0, 1000000, "rescue_kappa must be 0 .. 1000000 (units of 1e-9)"},
    {"rescue_tau", &g_opt_rescue_tau, 0, 1000000, "rescue_tau must be 0 .. 1000000 (units of 1e-9)"},
    {"time_kernel", &g_opt_time_kernel, 0, 1,
     "time_kernel must be 0 or 1 (HIP events around the PIV kernel of every launch, lspiv_kernel_times)"},
};
static const Option* find_option(const char* name) {
  for (const Option& o : kOptions)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

// every context's rescue lists of `stream` (NULL: the context's own stream) are freed, under the dispatch lock too if asked
static void drop_rescue_lists(void* stream, bool dispatch_lock) {
  std::vector<DeviceCtx*> ctxs;
  { std::lock_guard<std::mutex> lk(g_mu); ctxs = g_ctx; }
  for (size_t d = 0; d < ctxs.size() && d < (size_t)kMaxDevices; ++d) {
    DeviceCtx* c = ctxs[d];
    if (!c) continue;
    std::unique_lock<std::mutex> launch_lock(g_locks[d].dispatch, std::defer_lock);
    if (dispatch_lock) launch_lock.lock();
    std::lock_guard<std::mutex> lk(g_locks[d].lists);
    const hipStream_t s = on_stream(c, stream);
    for (size_t k = 0; k < c->rescue.size(); ++k) {
      if (c->rescue[k].stream != s) continue;
      (void)hipStreamSynchronize(s);
      if (c->rescue[k].base) (void)hipFree(c->rescue[k].base);
      c->rescue.erase(c->rescue.begin() + (long)k);
      break;
    }
  }
}

}  // namespace lspiv_api

using namespace lspiv_api;

namespace lspiv_comm_detail {   // lspiv_comm.hip reports through the same thread-local message
int comm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(code, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace lspiv_comm_detail

int lspiv::walk_setting() {
  const int v = g_opt_walk.load();
  if (v >= 0) return v;
  const char* e = getenv("LSPIV_WALK");
  return e ? atoi(e) : 1;
}

int lspiv::defer_fit_setting() { return g_opt_defer_fit.load(); }
int lspiv::unpack_dpp_setting() { return g_opt_unpack_dpp.load(); }
int lspiv::lds_light_setting() { return g_opt_lds_light.load(); }
int lspiv::scalar_epilogue_setting() { return g_opt_scalar_epilogue.load(); }

extern "C" {

const char* lspiv_last_error(void) { return g_err.c_str(); }

int lspiv_device_count(int* n) {
  if (!n) return fail(LSPIV_EINVAL, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  *n = (e == hipSuccess) ? c : 0;
  return LSPIV_OK;
}
int lspiv_set_device(int device) { HIP_TRY(hipSetDevice(device)); return LSPIV_OK; }
int lspiv_get_device(int* device) {
  if (!device) return fail(LSPIV_EINVAL, "device is NULL");
  HIP_TRY(hipGetDevice(device));
  return LSPIV_OK;
}
int lspiv_device_name(int device, char* buf, size_t len) {
  if (!buf || len == 0) return fail(LSPIV_EINVAL, "buf is NULL");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return LSPIV_OK;
}
int lspiv_synchronize(void) { HIP_TRY(hipDeviceSynchronize()); return LSPIV_OK; }

int lspiv_set_option(const char* name, int value) {
  if (!name) return fail(LSPIV_EINVAL, "option name is NULL");
  if (strcmp(name, "walk") == 0) {
    if (value < -1) return fail(LSPIV_EINVAL, "walk must be -1 (environment), 0, 1 or a segment length");
    g_opt_walk.store(value);
    return LSPIV_OK;
  }
  if (strcmp(name, "rescue_fit_size") == 0) return fail(LSPIV_EINVAL, "rescue_fit_size is read-only");
  if (strcmp(name, "peaks_refitted") == 0) return fail(LSPIV_EINVAL, "peaks_refitted is read-only");
  const Option* o = find_option(name);
  if (!o) return fail(LSPIV_EINVAL, "unknown option '%s'", name);
  if (value < o->lo || value > o->hi) return fail(LSPIV_EINVAL, "%s", o->range);
  o->value->store(value);
  return LSPIV_OK;
}
int lspiv_get_option(const char* name, int* value) {
  if (!name || !value) return fail(LSPIV_EINVAL, "NULL argument");
  if (strcmp(name, "walk") == 0) { *value = lspiv::walk_setting(); return LSPIV_OK; }
  if (strcmp(name, "rescue_fit_size") == 0) { *value = g_rescue_fit_size.load(); return LSPIV_OK; }
  if (strcmp(name, "peaks_refitted") == 0) { *value = g_peaks_refitted.load(); return LSPIV_OK; }
  const Option* o = find_option(name);
  if (!o) return fail(LSPIV_EINVAL, "unknown option '%s'", name);
  *value = o->value->load();
  return LSPIV_OK;
}

// ---- device-resident helpers ------------------------------------------------------------------
int lspiv_dev_malloc(void** d_ptr, size_t bytes) {
  if (!d_ptr) return fail(LSPIV_EINVAL, "d_ptr is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipMalloc(d_ptr, bytes));
  return LSPIV_OK;
}
int lspiv_dev_free(void* d_ptr) { if (d_ptr) HIP_TRY(hipFree(d_ptr)); return LSPIV_OK; }
// The three helpers below run on the library's stream and wait for it: the kernels are launched on a NON-BLOCKING
// stream, which does not synchronise with the null stream, and a null-stream hipMemcpy from pageable memory / hipMemset
// may return before the data has landed (seen as a flaky first launch reading a half-written stack).
int lspiv_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  if (bytes >= ((size_t)16 << 20) && !is_pinned(h_src)) {
    // a large pageable source (a frame stack, or a time chunk of one): through the two-slot pinned ring, staging threads
    // overlapped with the DMA of the previous slice, like the host entry points -- ~2x the rate of a plain pageable
    // hipMemcpy.  At least four slices per call, so that the un-overlapped first staging step stays a small part of it.
    std::lock_guard<std::mutex> host_lock(locks_here().host);
    LSPIV_TRY(stage_ring(c, 1));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the DMA runs on the copy stream: earlier kernels may still use d_dst
    const size_t slice = std::min(c->pinned_cap, std::max((size_t)4 << 20, ((bytes / 4) + 4095) & ~(size_t)4095));
    int batch = 0;
    for (size_t off = 0; off < bytes; off += slice, ++batch) {
      const int slot = batch & 1;
      const size_t nb = std::min(slice, bytes - off);
      if (batch >= 2) HIP_TRY(hipEventSynchronize(c->staged[slot]));
      staged_copy(c->pinned[slot], (const char*)h_src + off, nb);
      HIP_TRY(hipMemcpyAsync((char*)d_dst + off, c->pinned[slot], nb, hipMemcpyHostToDevice, c->copy_stream));
      HIP_TRY(hipEventRecord(c->staged[slot], c->copy_stream));
    }
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    return LSPIV_OK;
  }
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
int lspiv_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
// Host frames into a slice of an HBM-resident stack, the way the PIV host entry points bring them in (the same staging threads, the
// same float64 -> float32 conversion and DC-offset guard: a stack filled by this call holds the bytes lspiv_piv_pairs would have
// computed on), without launching anything.  Blocking.
int lspiv_upload_frames(void* d_dst, const void* frames, int dtype, int64_t n_frames, int64_t H, int64_t W, float signal_threshold) {
  if (!d_dst || !frames) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (n_frames < 0 || H <= 0 || W <= 0) return fail(LSPIV_ESHAPE, "bad shape (%lld, %lld, %lld)", (long long)n_frames, (long long)H, (long long)W);
  if (n_frames == 0) return LSPIV_OK;
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t frame_elems = (size_t)H * W, frame_bytes = frame_elems * elem_size(dtype == LSPIV_F64 ? LSPIV_F32 : dtype);
  LSPIV_TRY(stage_ring(c, frame_bytes));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the DMA runs on the copy stream: earlier kernels may still use d_dst
  const bool src_pinned = dtype != LSPIV_F64 && is_pinned(frames);
  // at least four slices per call, so that the un-overlapped first staging step stays a small part of it
  const int64_t fpb = std::max<int64_t>(1, std::min<int64_t>((int64_t)(c->pinned_cap / frame_bytes), (n_frames + 3) / 4));
  int batch = 0;
  for (int64_t f0 = 0; f0 < n_frames; ++batch) {
    const int64_t f1 = std::min<int64_t>(n_frames, f0 + fpb);
    LSPIV_TRY(stage_frames(c, batch, d_dst, frames, dtype, src_pinned, frame_elems, f0, f1, signal_threshold));
    f0 = f1;
  }
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  return LSPIV_OK;
}

int lspiv_trace(int enable) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  Trace& t = g_trace[current_device_slot()];
  HIP_TRY(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(t.mu);
  for (TraceRec& r : t.recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  t.recs.clear();
  if (enable) {
    if (!t.base) HIP_TRY(hipEventCreate(&t.base));
    HIP_TRY(hipEventRecord(t.base, c->stream));
    HIP_TRY(hipEventSynchronize(t.base));
  }
  t.on.store(enable != 0);
  return LSPIV_OK;
}
int lspiv_trace_read(int64_t cap, int32_t* kind, double* start_ms, double* end_ms, int64_t* n) {
  if (!n || cap < 0 || (cap > 0 && (!kind || !start_ms || !end_ms))) return fail(LSPIV_EINVAL, "bad argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  Trace& t = g_trace[current_device_slot()];
  HIP_TRY(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(t.mu);
  *n = (int64_t)t.recs.size();
  if (!t.base) return LSPIV_OK;
  for (int64_t i = 0; i < std::min<int64_t>(cap, *n); ++i) {
    float a = 0.0f, b = 0.0f;
    HIP_TRY(hipEventElapsedTime(&a, t.base, t.recs[(size_t)i].e0));
    HIP_TRY(hipEventElapsedTime(&b, t.base, t.recs[(size_t)i].e1));
    kind[i] = t.recs[(size_t)i].kind; start_ms[i] = a; end_ms[i] = b;
  }
  return LSPIV_OK;
}

int lspiv_host_alloc(void** h_ptr, size_t bytes) {
  if (!h_ptr) return fail(LSPIV_EINVAL, "h_ptr is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault));
  return LSPIV_OK;
}
int lspiv_host_free(void* h_ptr) {
  if (h_ptr) HIP_TRY(hipHostFree(h_ptr));
  return LSPIV_OK;
}
int lspiv_memset_dev(void* d_ptr, int value, size_t bytes) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipMemsetAsync(d_ptr, value, bytes, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_event_create(void** ev) {
  if (!ev) return fail(LSPIV_EINVAL, "ev is NULL");
  hipEvent_t e;
  HIP_TRY(hipEventCreate(&e));
  *ev = (void*)e;
  return LSPIV_OK;
}
int lspiv_event_record(void* ev) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipEventRecord((hipEvent_t)ev, c->stream));
  return LSPIV_OK;
}
int lspiv_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms) {
  if (!ms) return fail(LSPIV_EINVAL, "ms is NULL");
  HIP_TRY(hipEventSynchronize((hipEvent_t)ev_stop));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
  return LSPIV_OK;
}
int lspiv_event_destroy(void* ev) { if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return LSPIV_OK; }

int lspiv_stream_create(void** stream) {
  if (!stream) return fail(LSPIV_EINVAL, "stream is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  return LSPIV_OK;
}
int lspiv_stream_create_priority(void** stream, int priority) {
  if (!stream) return fail(LSPIV_EINVAL, "stream is NULL");
  if (priority == 0) return lspiv_stream_create(stream);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  int least = 0, greatest = 0;   // HIP: numerically LOWER = higher priority
  HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  hipStream_t s;
  HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority > 0 ? greatest : least));
  *stream = s;
  return LSPIV_OK;
}
int lspiv_stream_destroy(void* stream) {
  if (!stream) return LSPIV_OK;
  // the rescue lists of that stream go with it (a later stream may get the same handle value)
  drop_rescue_lists(stream, false);
  HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return LSPIV_OK;
}
int lspiv_stream_release(void* stream) {
  // a stream the caller created itself (hipStreamCreate) and handed to "_dev" entry points: drop what the library keeps for it
  // (the rescue lists) -- lspiv_stream_destroy does the same for streams of lspiv_stream_create
  drop_rescue_lists(stream, true);
  return LSPIV_OK;
}
int lspiv_stream_synchronize(void* stream) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipStreamSynchronize(on_stream(c, stream)));
  return LSPIV_OK;
}
int lspiv_event_record_on(void* ev, void* stream) {
  if (!ev) return fail(LSPIV_EINVAL, "event is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipEventRecord((hipEvent_t)ev, on_stream(c, stream)));
  return LSPIV_OK;
}
int lspiv_stream_wait_event(void* stream, void* ev) {
  if (!ev) return fail(LSPIV_EINVAL, "event is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  HIP_TRY(hipStreamWaitEvent(on_stream(c, stream), (hipEvent_t)ev, 0));
  return LSPIV_OK;
}

int lspiv_synth_particles_dev(void* d_frames, int64_t T, int64_t H, int64_t W, uint64_t seed, float density) {
  if (!d_frames || T < 1 || H < 8 || W < 8 || !(density > 0.0f)) return fail(LSPIV_EINVAL, "bad argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  LSPIV_TRY(launch_status(lspiv::launch_synth_particles((uint8_t*)d_frames, T, (int)H, (int)W, seed, density, c->stream), "synth failed", LSPIV_ENOMEM));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

// ---- debug hooks ------------------------------------------------------------------------------
int lspiv_debug_narrow(const double* frames, int64_t frame_elems, int64_t n_frames, int min_abs, float* out, double* offsets) {
  // test hook, host only (no device needed): the float64 -> float32 staging conversion of the host entry points
  if (!frames || !out || frame_elems < 0 || n_frames < 0) return fail(LSPIV_EINVAL, "bad argument");
  std::vector<double> off((size_t)n_frames, 0.0);
  if (min_abs >= 0)
    for (int64_t f = 0; f < n_frames; ++f) off[(size_t)f] = lspiv_host::frame_offset(frames + (size_t)f * frame_elems, (size_t)frame_elems, (double)min_abs);
  lspiv_host::staged_narrow(out, frames, (size_t)frame_elems, (size_t)n_frames, off.data());
  if (offsets) memcpy(offsets, off.data(), off.size() * sizeof(double));
  return lspiv_host::stage_threads();
}
int lspiv_debug_project_division(int* mismatches) {
  // test hook: project_mix_kernel's division-free quotient against the division, every sum 0 .. 255 c for every count c = 1 .. 255
  if (!mismatches) return fail(LSPIV_EINVAL, "NULL argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, sizeof(int)));
  HIP_TRY(hipMemsetAsync(c->d_scratch, 0, sizeof(int), c->stream));
  LSPIV_TRY(launch_status(lspiv::launch_division_check((int*)c->d_scratch, c->stream)));
  HIP_TRY(hipMemcpyAsync(mismatches, c->d_scratch, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
int lspiv_debug_hold_lock(int device, int which, int milliseconds) {
  if (device < 0 || device >= kMaxDevices || which < 0 || which > 2 + DeviceCtx::kProjSlots || milliseconds < 0 || milliseconds > 10000)
    return fail(LSPIV_EINVAL, "device %d / lock %d / %d ms out of range", device, which, milliseconds);
  DeviceLocks& l = g_locks[device];
  std::lock_guard<std::mutex> lk(which == 0 ? l.host : which == 1 ? l.dispatch : which == 2 ? l.lists : l.project[which - 3]);
  std::this_thread::sleep_for(std::chrono::milliseconds(milliseconds));
  return LSPIV_OK;
}
int lspiv_debug_segments(int64_t n_pairs, int64_t pair_offset, int seg_len, int64_t* seg_first, int64_t* n_seg) {
  if (n_pairs < 1 || n_pairs > 0x7fffffff || pair_offset < 0 || seg_len < 1 || !seg_first || !n_seg) return LSPIV_EINVAL;
  const lspiv::WalkSegments w = lspiv::walk_segments((uint32_t)n_pairs, pair_offset, (uint32_t)seg_len);
  *seg_first = w.seg_first;
  *n_seg = w.n_seg;
  return LSPIV_OK;
}

static int debug_fft(int n, int form, int inverse, const float* in, float* out, int64_t count) {
  if (!in || !out || count < 1 || count > (1 << 20)) return fail(LSPIV_EINVAL, "bad argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t bytes = (size_t)count * 2 * n * sizeof(float);
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, 2 * bytes));
  float* d_in = (float*)c->d_scratch;
  float* d_out = d_in + (size_t)count * 2 * n;
  HIP_TRY(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream));
  hipError_t e = lspiv::launch_fft_debug_form(n, form, inverse != 0, d_in, d_out, (int)count, c->stream);
  if (e == hipErrorInvalidValue) return fail(LSPIV_EUNSUPPORTED, "no register FFT of length %d in form %d", n, form);
  LSPIV_TRY(launch_status(e));
  HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
int lspiv_debug_fft(int n, int inverse, const float* in, float* out, int64_t count) { return debug_fft(n, 0, inverse, in, out, count); }
int lspiv_debug_half_reduce(int op, int form, const uint32_t* in, uint32_t* out, int64_t count) {
  if (!in || !out || count < 1 || count > (1 << 16)) return fail(LSPIV_EINVAL, "bad argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t bytes = (size_t)count * 64 * sizeof(uint32_t);
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, 2 * bytes));
  uint32_t* d_in = (uint32_t*)c->d_scratch;
  uint32_t* d_out = d_in + (size_t)count * 64;
  HIP_TRY(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream));
  hipError_t e = lspiv::launch_half_reduce_debug(op, form, d_in, d_out, (int)count, c->stream);
  if (e == hipErrorInvalidValue) return fail(LSPIV_EUNSUPPORTED, "no half-wave reduction %d in form %d", op, form);
  LSPIV_TRY(launch_status(e));
  HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
int lspiv_debug_first_match(int form, const uint32_t* in, uint32_t* out, int64_t count) {
  if (!in || !out || count < 1 || count > (1 << 16)) return fail(LSPIV_EINVAL, "bad argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t bytes = (size_t)count * 64 * sizeof(uint32_t);
  LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, 2 * bytes));
  uint32_t* d_in = (uint32_t*)c->d_scratch;
  uint32_t* d_out = d_in + (size_t)count * 64;
  HIP_TRY(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream));
  hipError_t e = lspiv::launch_first_match_debug(form, d_in, d_out, (int)count, c->stream);
  if (e == hipErrorInvalidValue) return fail(LSPIV_EUNSUPPORTED, "no first-match search in form %d", form);
  LSPIV_TRY(launch_status(e));
  HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}
int lspiv_debug_fft_form(int n, int form, int inverse, const float* in, float* out, int64_t count) {
  if (n < 1 || n > 64) return fail(LSPIV_EUNSUPPORTED, "no register FFT of length %d", n);
  return debug_fft(n, form, inverse, in, out, count);
}

}  // extern "C"
