// What the host files of the C ABI share (api_*.hip): the error report, the per-device contexts and locks, the workspaces, the
// trace spans, the staged call of the host twins (HostCall), the run-time options and the helpers of the entry points.  Host logic only.  Everything here has hidden visibility:
// the library exports the lspiv_* entry points of include/lspiv.h, not these.
#pragma once

#include "../../include/lspiv.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_slots.h"
#include "host_stage.h"
#include "piv_peaks.h"
#include "rescue_options.h"

namespace lspiv_api __attribute__((visibility("hidden"))) {

// sets the thread-local message of lspiv_last_error (api_core.hip) and returns `code`
int fail(int code, const char* fmt, ...);

// the lspiv status of a failed HIP call
inline int hip_code(hipError_t e) {
  return e == hipErrorOutOfMemory ? LSPIV_ENOMEM : (e == hipErrorNoDevice || e == hipErrorNoBinaryForGpu) ? LSPIV_ENODEV : LSPIV_EHIP;
}

#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    const hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess)                                                                                      \
      return fail(hip_code(e_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
  } while (0)

// an lspiv status other than LSPIV_OK is returned as it is (its message already set)
#define LSPIV_TRY(expr)                                                                        \
  do {                                                                                         \
    const int rc_ = (expr);                                                                    \
    if (rc_ != LSPIV_OK) return rc_;                                                           \
  } while (0)

// the status of a kernel launcher as an entry point reports it; `oom_code` for hipErrorOutOfMemory (launchers that allocate)
inline int launch_status(hipError_t e, const char* what = "kernel launch failed", int oom_code = LSPIV_EHIP) {
  if (e == hipSuccess) return LSPIV_OK;
  return fail(e == hipErrorOutOfMemory ? oom_code : LSPIV_EHIP, "%s: %s", what, hipGetErrorString(e));
}

inline size_t elem_size(int dtype) { return dtype == LSPIV_U8 ? 1 : dtype == LSPIV_F32 ? 4 : 8; }

// ---- window grid (api_piv.hip) ---------------------------------------------------------------------------------------------
struct Grid {
  int64_t n_rows = 0, n_cols = 0;
};
int make_grid(int64_t H, int64_t W, int wy, int wx, int oy, int ox, Grid* g);

// ---- per-device context: launch stream + grow-only HBM / pinned workspaces (api_core.hip) ------------------------------------
struct DeviceCtx {
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;
  void* d_frames = nullptr;  size_t frames_cap = 0;
  float* d_out = nullptr;    size_t out_cap = 0;
  float* d_planes = nullptr; size_t planes_cap = 0;
  void* d_scratch = nullptr; size_t scratch_cap = 0;   // temporaries of *_dev entry points (normalize)
  void* d_dft = nullptr; size_t dft_cap = 0;           // plane slots of the windows above 128 px (grow-only)
  uint8_t* d_keep = nullptr; size_t keep_cap = 0;      // per-window flags of the "stack" signal mode
  void* d_mp = nullptr; size_t mp_cap = 0;             // multi-pass chains: the intermediate passes' results and offsets (grow-only)
  uint8_t* d_mask = nullptr; size_t mask_cap = 0;      // the image mask of a host-fed masked launch (grow-only; under the host lock)
  float* d_peak2 = nullptr; size_t peak2_cap = 0;      // the second-peak block of a host-fed launch (grow-only; under the host lock)
  float* d_deform = nullptr; size_t deform_cap = 0;    // deformation passes: the warped frames of one batch of pairs (grow-only; under the multipass lock)
  // vector validation: the ping-pong fields [u | v] and the flags of a call without a flag buffer (grow-only; under the validate lock);
  // the event marks the end of the last call's kernels, which the next call's stream waits for before it reuses the workspace
  void* d_validate = nullptr; size_t validate_cap = 0; hipEvent_t validate_done = nullptr;
  // float64 rescue pass: one set of lists per launch stream (a stream orders its own PIV kernel -> rescue kernel pairs;
  // two streams must not share counters), grow-only
  struct RescueWs { hipStream_t stream; void* base; size_t cap_bytes; uint32_t cap_fit, cap_amb; };
  std::vector<RescueWs> rescue;
  void* pinned[2] = {nullptr, nullptr}; size_t pinned_cap = 0;  // H2D staging ring
  hipEvent_t staged[2] = {nullptr, nullptr};
  // host-pointer projection entry points (round 6): kProjSlots independent sets of {stream, input buffer, output buffer}, each under
  // its own lock (DeviceLocks::project), none of them shared with the PIV host entry points -- a project_hip block that dask runs
  // on a worker thread neither waits for the `host` lock a PIV call holds for its whole upload + kernels + download, nor for the
  // other block in flight: block k + 1 crosses PCIe while block k's kernel runs and its result goes back
  // pin[2]: pinned bounce buffers of kProjPinBytes each -- the frames of a block go up and its result comes down in slices through
  // them (staging threads on one slice, DMA on the other): a pageable hipMemcpyAsync moved a block's 93 MB of float32 result at a
  // few GB/s, which WAS the time of the generic project_hip -> get_piv path (bench.py: dropin_generic_path)
  struct ProjWs { hipStream_t stream = nullptr; void* d_in = nullptr; size_t in_cap = 0; void* d_out = nullptr; size_t out_cap = 0;
                  void* pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; };
  static constexpr size_t kProjPinBytes = (size_t)16 << 20;
  static constexpr int kProjSlots = 2;
  ProjWs proj[kProjSlots];
  bool arch_ok = false;
};
// Locks are PER DEVICE ("one host thread (or process) per GPU"): a process that drives several GPUs from several
// threads serialises only the calls that share a device's workspaces, not all of them (round 4 had three process-wide mutexes:
// every launch of every device queued behind one lock).  A fixed table, so that an entry point can take its lock before a context
// exists (and on a machine without a device: slot 0).
//   host:     host-pointer entry points share one set of workspaces (upload buffer, result buffer, pinned ring) per device
//   dispatch: the PIV kernel and the rescue kernels of ONE launch share their stream's lists and counters (see dispatch())
//   lists:    the per-stream rescue lists of a context (DeviceCtx::rescue)
//   multipass: the passes of ONE chain share the device's multi-pass workspace (DeviceCtx::d_mp): a chain is issued under it, so that
//             two host threads launching chains on the same stream cannot interleave their passes
//   project:  one per projection slot (DeviceCtx::proj): the host-pointer projection entry points; never nested with the others
//   validate: the iterations of ONE lspiv_validate_dev call share the device's validation workspace (DeviceCtx::d_validate); innermost
// Order when nested: host -> multipass -> dispatch -> lists; host -> validate.
constexpr int kMaxDevices = 64;
struct DeviceLocks { std::mutex host, multipass, dispatch, lists, validate, project[DeviceCtx::kProjSlots]; std::atomic<unsigned> next_project{0}; };
extern DeviceLocks g_locks[kMaxDevices];
int current_device_slot();
inline DeviceLocks& locks_here() { return g_locks[current_device_slot()]; }
// the context of the current device, created on first use; LSPIV_ENODEV without a gfx950 device
int get_ctx(DeviceCtx** out);
// the stream of a "_dev" entry point: the caller's, or the context's for NULL
inline hipStream_t on_stream(const DeviceCtx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }
// a "_dev" entry point's one kernel: launch(on_stream(ctx, stream)), its status as launch_status reports it
template <class Launch>
int launch_on(void* stream, Launch&& launch) {
  DeviceCtx* c;
  const int rc = get_ctx(&c);
  return rc ? rc : launch_status(launch(on_stream(c, stream)));
}

// "trace" (tests / measurement only, off by default): HIP events the LIBRARY records around the spans below, on the streams the work
// runs on; lspiv_trace_read returns them in milliseconds since lspiv_trace(1).  What a wall clock cannot show -- that a projection
// block's kernel ran INSIDE a concurrent PIV host call on the same device -- two event pairs can.
struct TraceRec { int kind; hipEvent_t e0, e1; };
struct Trace;
// a span that is begun but never ended (an error exit) destroys its events
struct TraceSpan {
  Trace* t = nullptr; TraceRec r{};
  ~TraceSpan();
};
void trace_begin(TraceSpan* sp, int kind, hipStream_t s);
void trace_end(TraceSpan* sp, hipStream_t s);

// host memory registered with HIP (hipHostMalloc / lspiv_host_alloc / hipHostRegister) can be DMA'd in place
bool is_pinned(const void* p);

// the staging copies run on persistent host threads (host_stage.cpp: LSPIV_STAGE_THREADS, AVX2 non-temporal stores); float64
// frames (what pyorc's project_numpy hands over) are narrowed to float32 while they are staged: the kernels
// convert every sample to float32 first thing anyway (same IEEE round-to-nearest conversion on both sides, so the results are
// bit-identical), and the PCIe transfer -- the bound of the host entry points -- halves
using lspiv_host::staged_copy;

// two pinned staging slots of >= one frame each (LSPIV_STAGE_BYTES per slot, default 32 MiB)
int stage_ring(DeviceCtx* c, size_t frame_bytes);
// Batch `batch` of a host stack -- frames [f0, f1) of frame_elems samples of `dtype` -- into the device stack d_dst through slot
// batch & 1 of the ring (waited for when an earlier batch used it), DMA on the copy stream, then the slot's event recorded there.
// float64 is narrowed to float32 while it is staged (narrow_offsets); a pinned source goes up in place.
int stage_frames(DeviceCtx* c, int batch, void* d_dst, const void* frames, int dtype, bool src_pinned, size_t frame_elems,
                 int64_t f0, int64_t f1, float signal_threshold);

template <typename P>
int ensure(P** ptr, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return LSPIV_OK;
  if (*ptr) HIP_TRY(hipFree(*ptr));
  *ptr = nullptr; *cap = 0;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  *ptr = static_cast<P*>(p); *cap = bytes;
  return LSPIV_OK;
}

// a byte count from the environment, read per call (test hooks); `dflt` when it is unset or no number
inline size_t env_bytes(const char* name, size_t dflt) {
  const char* e = std::getenv(name);
  char* end = nullptr;
  const unsigned long long v = e && *e ? std::strtoull(e, &end, 10) : 0;
  return end && !*end ? (size_t)v : dflt;
}
// host frame stacks go up in chunks of at most this size (lspiv_sti_gather, lspiv_lk_track); LSPIV_HOST_CHUNK_BYTES (a test hook) overrides it
inline size_t host_chunk_bytes() { return env_bytes("LSPIV_HOST_CHUNK_BYTES", (size_t)256 << 20); }

// ---- the host twins: one staged call ------------------------------------------------------------------------------------------
// A host-pointer entry point checks its arguments, then stages through the context's workspaces under the device's `host` lock:
//   HostCall hc({inputs}, {outputs});   the lock, the context, one slot per buffer (host_slots.h): inputs in d_frames, outputs in d_planes
//   if (hc.upload()) hc.ran(launch(hc.in<T>(i) .., hc.out<T>(j) .., hc.stream()));   the input copies, then the "_dev" twin or its launcher
//   return hc.finish(__func__);         the output copies if everything so far succeeded, the wait, the first error
// Pageable hipMemcpyAsync on the context's stream, as before the pinned ring existed.  Once a copy is queued, every exit synchronises
// that stream: the caller's buffers are released only once its copies are done.  A NULL host pointer is an optional argument that was
// not given: no slot, no copy, a NULL device pointer.  An output with `in` >= 0 IS that input's slot (a twin that works in place).
// `copy` = false: room only -- the chunked twins feed and drain such a slot themselves with copy_in / copy_out.
struct HostIn { const void* host = nullptr; size_t bytes = 0; bool copy = true; };
struct HostOut { void* host = nullptr; size_t bytes = 0; int in = -1; bool copy = true; };
class HostCall {
 public:
  static constexpr int kMaxSlots = 8;
  HostCall(std::initializer_list<HostIn> in, std::initializer_list<HostOut> out) : lock_(locks_here().host) {
    size_t bytes[kMaxSlots], off[kMaxSlots];
    bool present[kMaxSlots];
    if ((rc_ = get_ctx(&c_)) != LSPIV_OK) return;
    for (const HostIn& a : in) { bytes[n_in_] = a.bytes; present[n_in_] = a.host != nullptr; in_[n_in_++] = a; }
    if ((rc_ = ensure(&c_->d_frames, &c_->frames_cap, slot_layout(bytes, present, n_in_, off))) != LSPIV_OK) return;
    for (int i = 0; i < n_in_; ++i) d_in_[i] = present[i] ? (char*)c_->d_frames + off[i] : nullptr;
    for (const HostOut& a : out) { bytes[n_out_] = a.bytes; present[n_out_] = a.host != nullptr && a.in < 0; out_[n_out_++] = a; }
    if ((rc_ = ensure(&c_->d_planes, &c_->planes_cap, slot_layout(bytes, present, n_out_, off))) != LSPIV_OK) return;
    for (int i = 0; i < n_out_; ++i) d_out_[i] = out_[i].in >= 0 ? d_in_[out_[i].in] : present[i] ? (char*)c_->d_planes + off[i] : nullptr;
  }
  template <class T = void> T* in(int i) const { return (T*)d_in_[i]; }
  template <class T = void> T* out(int i) const { return (T*)d_out_[i]; }
  DeviceCtx* ctx() const { return c_; }
  hipStream_t stream() const { return c_->stream; }
  bool ok() const { return e_ == hipSuccess && rc_ == LSPIV_OK; }
  // the status of what the caller ran on stream() -- the first failure is kept; true while everything succeeded
  bool ran(int rc) { if (rc_ == LSPIV_OK) rc_ = rc; return ok(); }
  // one copy on the stream, skipped after a failure (device to device: `step` as it stands)
  bool copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* step = nullptr) {
    if (ok()) { if (step) step_ = step; queued_ = true; e_ = hipMemcpyAsync(dst, src, bytes, kind, c_->stream); }
    return ok();
  }
  bool copy_in(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice, "upload"); }
  bool copy_out(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost, "download"); }
  bool upload() {
    for (int i = 0; i < n_in_; ++i) if (d_in_[i] && in_[i].copy && in_[i].bytes) copy_in(d_in_[i], in_[i].host, in_[i].bytes);
    return ok();
  }
  int finish(const char* name) {
    for (int i = 0; i < n_out_; ++i) if (out_[i].host && out_[i].copy && out_[i].bytes) copy_out(out_[i].host, d_out_[i], out_[i].bytes);
    if (!queued_) return rc_;   // nothing of the caller's is in flight
    const hipError_t sync = hipStreamSynchronize(c_->stream);
    if (!ok()) {   // the first error is the one reported
      if (sync != hipSuccess) (void)hipGetLastError();
      return rc_ != LSPIV_OK ? rc_ : fail(hip_code(e_), "%s: %s failed: %s", name, step_, hipGetErrorString(e_));
    }
    if (sync != hipSuccess) return fail(hip_code(sync), "%s: synchronisation failed: %s", name, hipGetErrorString(sync));
    return LSPIV_OK;
  }

 private:
  std::lock_guard<std::mutex> lock_;
  DeviceCtx* c_ = nullptr;
  HostIn in_[kMaxSlots]; HostOut out_[kMaxSlots];
  void *d_in_[kMaxSlots] = {}, *d_out_[kMaxSlots] = {};
  int n_in_ = 0, n_out_ = 0, rc_ = LSPIV_OK;
  hipError_t e_ = hipSuccess;
  const char* step_ = "upload";
  bool queued_ = false;
};

// the twins with one input, one optional second input and one output: run(d_in, d_other, stream) calls the "_dev" twin, d_other being
// the output's slot or, for a twin that works in place (out.in = 0), the second input's
template <class Run>
int host_roundtrip(const char* name, HostIn in, HostOut out, Run&& run, HostIn aux = {}) {
  HostCall hc({in, aux}, {out});
  if (hc.upload()) hc.ran(run(hc.in(0), out.in == 0 ? hc.in(1) : hc.out(0), hc.stream()));
  return hc.finish(name);
}

// ---- run-time options (api_core.hip: lspiv_set_option / lspiv_get_option, initial values from the environment) ---------------
// the engine semantics that could not be pinned on a real ffpiv run, defaults = the oracle's reading
extern std::atomic<int> g_opt_border;        // 0 NaN, 1 plane centre, 2 integer peak
extern std::atomic<int> g_opt_signal_mode;   // 0 per window pair, 1 per window position over the chunk
extern std::atomic<int> g_opt_signal_pos;    // 0 samples != 0, 1 samples > 0
// the readings of ffpiv added in round 3 (same names and values as oracle/'s SEMANTICS)
extern std::atomic<int> g_opt_v_sign;        // 0 v as it comes out of the plane, 1 negated
extern std::atomic<int> g_opt_norm_clip;     // 1 negative lobes of the normalised window removed (A3), 0 kept
extern std::atomic<int> g_opt_std_ddof;      // 0 population, 1 sample standard deviation
extern std::atomic<int> g_opt_round_odd;     // round_to_even of odd sizes: 0 half-even of x / 2, 1 up, 2 down (host side; kept here so that ONE place holds every switch)
// float64 rescue pass (piv_rescue.hip): on by default; LSPIV_RESCUE=0 / lspiv_set_option("rescue", 0) keeps the float32 results.
// rescue_kappa: the plane noise the flags assume, in 1e-9 of the plane maximum (measured worst case 2.7e-7 in the units of the
// flag's error model -- tools/calib_rescue.py; default 500 = 5e-7); rescue_tau: relative arg-max gap, in 1e-9, below which the
// whole plane is re-evaluated (float32 noise between two samples is <= 8.4e-7; default 4000 = 4e-6)
extern std::atomic<int> g_opt_rescue;
extern std::atomic<int> g_opt_rescue_kappa;
extern std::atomic<int> g_opt_rescue_tau;
// ("rescue_generic" and the read-only "rescue_fit_size": rescue_options.h, shared with piv_rescue.hip)
// "peaks_refitted" (read-only): planes the last lspiv_u_v_displacement of this process fitted again in float64 (piv_peaks.h)
extern std::atomic<int> g_peaks_refitted;
// float64 host stacks: a frame whose DC offset (host_stage.h, frame_offset) reaches this magnitude has it taken off while it is
// narrowed to float32 -- PIV entry points only (the per-window normalisation does not see it), and only without a signal threshold
// (which counts samples != 0).  -1: never.
extern std::atomic<int> g_opt_narrow_offset;
// "time_kernel" (measurement only, off by default): HIP events around the PIV kernel(s) of every launch (api_piv.hip, dispatch)
extern std::atomic<int> g_opt_time_kernel;
// the DC offsets g_opt_narrow_offset takes off n_frames float64 frames (all zero when it does not apply)
std::vector<double> narrow_offsets(const double* frames, size_t frame_elems, int64_t n_frames, float signal_threshold);

// ---- PIV launches, shared with the ensemble (api_piv.hip) ------------------------------------------------------------------
int fill_params(lspiv::PivParams* p, const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx,
                int oy, int ox, float signal_threshold, const Grid& g);
// filter: 0, or LSPIV_FILTER_SPOF -- the phase-filtered kernels (piv_spof_impl.h), never followed by a rescue pass
int dispatch(const lspiv::PivParams& p0, int dtype, bool ensemble, hipStream_t s, int filter = 0);
int apply_v_sign(float* d_v, int64_t n, hipStream_t s);
int apply_signal_mode(DeviceCtx* c, lspiv::PivParams* p, int dtype, hipStream_t s);
// what the families with kernels of a fixed size compose their checks from (LSPIV_EUNSUPPORTED / LSPIV_EINVAL, `what` names the
// family in the message): the window is 16, 32 or 64 px square; the frame's sides fit an int16 (`what`: what has to hold them); the
// options norm_clip = 0 and -- unless the family scores window positions like the plain kernels -- signal_mode = 1 are refused
int check_fixed_square(int wy, int wx, const char* what);
int check_frame_fits_int16(int64_t H, int64_t W, const char* what);
// the frame stack of the families that address pixels with 16 bits (warp_affine, sti_gather, pyr_down, lk_track; api_track.hip): uint8 or
// float32, T_min .. 2^31 - 1 frames, sides side_min .. 32767; LSPIV_EINVAL, `what` names the family in the message
int check_frames(const char* what, int dtype, int64_t T, int64_t T_min, int64_t H, int64_t W, int64_t side_min);
int check_pair_options(const char* what, bool position_signal_ok = false);
// shifted passes (multi-pass PIV, multi-pass ensemble) and SPOF-filtered correlation: the three of them
int check_shift(int wy, int wx, int64_t H, int64_t W);
inline int check_multipass_options() { return check_pair_options("multi-pass PIV"); }
int check_spof(int wy, int wx);
// the kernel families, numbered as lspiv_kernel_kind reports them (include/lspiv.h)
enum KernelKind : int {
  kKindFft32 = 1, kKindFft64 = 2, kKindDirect = 3, kKindEmbed32 = 4, kKindEmbed64 = 5, kKindFft8or16 = 6, kKindEmbed16 = 7, kKindPfa = 8,
  kKindDft = 9, kKindDftGlobal = 10
};
// window kinds served by the time-walking kernels (every even square window 6 .. 64)
inline bool kind_walks(int kind) { return kind == kKindFft32 || kind == kKindFft64 || kind == kKindFft8or16 || kind == kKindPfa; }
// the anchor length the walking kernels use on a grid of n_win windows (common.h, walk_anchor)
int chunk_alignment_for(int wy, int wx, int64_t n_win);

}  // namespace lspiv_api
