// C ABI of liblspiv_hip.so, PIV (api_core.hip has the overview): the window grid, the kernel of a window's family, the float64 rescue
// pass after it, the chunk alignment, the device-pointer and host-pointer PIV entry points.
#include "api_internal.h"
#include "piv_masked.h"
#include "piv_peak2.h"
#include "piv_spof.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace lspiv_api __attribute__((visibility("hidden"))) {

int check_window(int wy, int wx, int oy, int ox) {
  if (wy < 2 || wx < 2 || wy > LSPIV_MAX_WINDOW || wx > LSPIV_MAX_WINDOW)
    return fail(LSPIV_EUNSUPPORTED, "window %dx%d outside supported range 2..%d", wy, wx, LSPIV_MAX_WINDOW);
  if (oy < 0 || ox < 0 || oy >= wy || ox >= wx)
    return fail(LSPIV_EINVAL, "overlap (%d,%d) must satisfy 0 <= overlap < window (%d,%d)", oy, ox, wy, wx);
  return LSPIV_OK;
}

// ffpiv.window.get_axis_shape restated: (dim - win)//(win - overlap) + 1
int64_t axis_shape(int64_t dim, int win, int ov) { return dim < win ? 0 : (dim - win) / (win - ov) + 1; }

int make_grid(int64_t H, int64_t W, int wy, int wx, int oy, int ox, Grid* g) {
  LSPIV_TRY(check_window(wy, wx, oy, ox));
  if (H <= 0 || W <= 0) return fail(LSPIV_ESHAPE, "frame shape (%lld,%lld) invalid", (long long)H, (long long)W);
  g->n_rows = axis_shape(H, wy, oy);
  g->n_cols = axis_shape(W, wx, ox);
  if (g->n_rows <= 0 || g->n_cols <= 0)
    return fail(LSPIV_ESHAPE, "frame (%lld,%lld) smaller than window (%d,%d)", (long long)H, (long long)W, wy, wx);
  return LSPIV_OK;
}

// the rescue lists of a launch of n_tiles windows: a quarter of them "fit" (16 bytes each), a sixteenth "amb" (4 bytes each) -- beyond that
// the excess keeps its float32 result: imagery THAT sparse has no usable peaks -- behind a header slot
struct RescueCaps {
  size_t fit, amb;
  static constexpr size_t hdr_bytes = 256;   // sizeof(RescueHdr) rounded up, keeps the lists 256-byte aligned
  size_t bytes() const { return hdr_bytes + fit * sizeof(uint4) + amb * sizeof(uint32_t); }
};
static_assert(sizeof(lspiv::RescueHdr) <= RescueCaps::hdr_bytes, "header slot too small");
static RescueCaps rescue_caps(int64_t n_tiles) { return {(size_t)std::max<int64_t>(4096, n_tiles / 4), (size_t)std::max<int64_t>(1024, n_tiles / 16)}; }

// the rescue lists of stream `s`, large enough for a launch of n_tiles windows
int rescue_ws(DeviceCtx* c, hipStream_t s, uint32_t n_tiles, lspiv::PivParams* p) {
  std::lock_guard<std::mutex> lk(locks_here().lists);
  DeviceCtx::RescueWs* ws = nullptr;
  for (auto& w : c->rescue) if (w.stream == s) ws = &w;
  if (!ws) { c->rescue.push_back({s, nullptr, 0, 0, 0}); ws = &c->rescue.back(); }
  const RescueCaps need = rescue_caps(n_tiles);
  const size_t hdr_bytes = RescueCaps::hdr_bytes;
  if (need.fit > ws->cap_fit || need.amb > ws->cap_amb || !ws->base) {
    const RescueCaps grow = {std::max<size_t>(need.fit, ws->cap_fit), std::max<size_t>(need.amb, ws->cap_amb)};
    const size_t bytes = grow.bytes();
    void* grown = nullptr;
    HIP_TRY(hipMalloc(&grown, bytes));
    if (ws->base) {
      // the header moves along: its per-pass counters are zero between passes (the rescue kernel's last block resets them) and
      // the totals of lspiv_rescue_stats ("summed over all launches") survive the regrow
      hipError_t e = hipStreamSynchronize(s);
      if (e == hipSuccess) e = hipMemcpy(grown, ws->base, hdr_bytes, hipMemcpyDeviceToDevice);
      if (e != hipSuccess) { (void)hipFree(grown); return fail(LSPIV_EHIP, "rescue lists: %s", hipGetErrorString(e)); }
      HIP_TRY(hipFree(ws->base));
    } else {
      HIP_TRY(hipMemsetAsync(grown, 0, hdr_bytes, s));   // ordered before the kernels of this stream
    }
    ws->base = grown;
    ws->cap_bytes = bytes; ws->cap_fit = (uint32_t)grow.fit; ws->cap_amb = (uint32_t)grow.amb;
  }
  p->rescue_hdr = static_cast<lspiv::RescueHdr*>(ws->base);
  p->rescue_fit = reinterpret_cast<uint4*>((char*)ws->base + hdr_bytes);
  p->rescue_amb = reinterpret_cast<uint32_t*>((char*)ws->base + hdr_bytes + (size_t)ws->cap_fit * sizeof(uint4));
  p->rescue_cap_fit = ws->cap_fit;
  p->rescue_cap_amb = ws->cap_amb;
  return LSPIV_OK;
}

int fill_params(lspiv::PivParams* p, const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx,
                int oy, int ox, float signal_threshold, const Grid& g) {
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  const int64_t n_win = g.n_rows * g.n_cols;
  const int64_t n_tiles = (T - 1) * n_win;
  if (n_tiles >= (int64_t)1 << 31 || H * W >= (int64_t)1 << 31)
    return fail(LSPIV_EINVAL, "chunk too large for one launch: %lld windows (limit 2^31); use smaller chunks",
                (long long)n_tiles);
  memset(p, 0, sizeof(*p));
  p->frames = d_frames;
  p->frame_elems = H * W;
  p->H = (int)H; p->W = (int)W;
  p->wy = wy; p->wx = wx;
  p->sy = wy - oy; p->sx = wx - ox;
  p->n_rows = (int)g.n_rows; p->n_cols = (int)g.n_cols;
  p->n_win = (uint32_t)n_win;
  p->n_tiles = (uint32_t)n_tiles;
  p->n_pairs = (uint32_t)(T - 1);
  p->signal_threshold = signal_threshold;
  p->border_mode = g_opt_border.load();
  p->nz_positive = g_opt_signal_pos.load();
  {
    const double n = (double)wy * (double)wx;
    const double g2 = g_opt_std_ddof.load() && n > 1.0 ? (n - 1.0) / n : 1.0;   // sample std: every normalised window shrinks by sqrt((n-1)/n)
    p->std_gain2 = (float)g2;
    p->std_gain = (float)std::sqrt(g2);
    p->norm_clip = g_opt_norm_clip.load();
  }
  // flag model of the rescue pass (common.h, peak_cond): k = 2 kappa / (ln 2 * 1e-4)
  p->rescue_k = (float)(2.0 * g_opt_rescue_kappa.load() * 1e-9 / (0.6931471805599453 * 1e-4));
  p->rescue_tau = (float)(g_opt_rescue_tau.load() * 1e-9);
  p->div_ncols = lspiv::FastDiv::make((uint32_t)g.n_cols);
  p->div_jobs = lspiv::FastDiv::make((uint32_t)((n_win + 1) / 2));
  p->div_nwin = lspiv::FastDiv::make((uint32_t)n_win);
  return LSPIV_OK;
}

// where a launch writes: tiles [t0, t0 + p->n_tiles) of a result block [u | v | corr_max | s2n] laid out for `total` tiles, and those
// tiles' planes (plane_elems floats each) of `planes`, if there are any
static void set_results(lspiv::PivParams* p, float* block, size_t total, size_t t0, float* planes, size_t plane_elems) {
  p->u = block + t0;
  p->v = block + total + t0;
  p->cmax = block + 2 * total + t0;
  p->s2n = block + 3 * total + t0;
  p->planes = planes ? planes + t0 * plane_elems : nullptr;
}

// search-area mode: an even square window wy = wx = n, 4 <= n <= S - 2, of frame t inside a square search area S = say = sax of
// frame t+1, S in {16, 32, 64}
static bool search_shape_ok(int say, int sax, int wy, int wx) {
  return say == sax && (say == 16 || say == 32 || say == 64) && wy == wx && wy >= 4 && wy <= say - 2 && (wy & 1) == 0;
}
static int check_search(int say, int sax, int wy, int wx) {
  if (!search_shape_ok(say, sax, wy, wx))
    return fail(LSPIV_EUNSUPPORTED, "search area %dx%d with window %dx%d is not supported: the search area must be square, 16, 32 or 64, "
                "and the window square and even with 4 <= window <= search area - 2", say, sax, wy, wx);
  return check_pair_options("a search area", true);   // (signal_mode = 1 scores the positions of the search areas)
}
// p filled for the search area (fill_params with wy = wx = S) -> window n inside it
static void set_search_window(lspiv::PivParams* p, int n) {
  p->nw = n;
  if (g_opt_std_ddof.load()) {   // sample std of BOTH windows: (n^2 - 1) / n^2 of the window times (S^2 - 1) / S^2 of the search area, under one root
    const double na = (double)n * n, nb = (double)p->wy * p->wx;
    const double g2 = std::sqrt((na - 1.0) / na * (nb - 1.0) / nb);
    p->std_gain2 = (float)g2;
    p->std_gain = (float)std::sqrt(g2);   // the rescue pass scales each window by it: only the product of the two matters
  }
}

static int dispatch_kernels(const lspiv::PivParams& p, int dtype, bool ensemble, hipStream_t s, int filter);

// PIV kernel of the window's family, then -- per-timestep mode, unless switched off -- the float64 rescue pass over the
// windows that kernel flagged (piv_rescue.hip)
// The PIV kernel and the two rescue kernels of ONE launch share the stream's lists and counters: they are issued under one
// lock, so that two host threads launching on the same stream (NULL -> the library's stream) cannot interleave as PIV 1,
// PIV 2, rescue 1 -- rescue 1 would then consume launch 2's records with launch 1's parameters.  Launches are asynchronous:
// the lock is held for microseconds.  (The rescue kernels skip a record whose index is outside their launch all the same.)
// "time_kernel" option (measurement only, off by default): HIP events on the launch's own stream right before and right after the
// PIV kernel(s) of a launch -- NOT around the rescue kernels that follow --, i.e. the duration rocprofv3 --kernel-trace reports for
// the dominant kernel, inside the launch exactly as a caller issues it (rescue pass on: the kernel appends its records).  A ring of
// the last 16 launches per device; lspiv_kernel_times reads and empties it.  bench.py's roofline.achieved comes from here.
constexpr int kTimerRing = 16;
struct KernelTimer { hipEvent_t e0[kTimerRing] = {}, e1[kTimerRing] = {}; int n = 0; };
KernelTimer g_timers[kMaxDevices];   // guarded by the device's dispatch lock
static int timed_dispatch_kernels(const lspiv::PivParams& p, int dtype, bool ensemble, hipStream_t s, int filter) {
  if (!g_opt_time_kernel.load()) return dispatch_kernels(p, dtype, ensemble, s, filter);
  KernelTimer& t = g_timers[current_device_slot()];
  const int k = t.n % kTimerRing;
  if (!t.e0[k]) { HIP_TRY(hipEventCreate(&t.e0[k])); HIP_TRY(hipEventCreate(&t.e1[k])); }
  HIP_TRY(hipEventRecord(t.e0[k], s));
  LSPIV_TRY(dispatch_kernels(p, dtype, ensemble, s, filter));
  HIP_TRY(hipEventRecord(t.e1[k], s));
  ++t.n;
  return LSPIV_OK;
}
// filter != 0 (LSPIV_FILTER_SPOF): the phase-filtered kernels, which have no rescue pass -- a filtered plane is no sum of lag products of
// the samples, so the rescue kernels could not re-evaluate it; the "rescue" option has no effect on them
int dispatch(const lspiv::PivParams& p0, int dtype, bool ensemble, hipStream_t s, int filter) {
  if (ensemble || filter || !g_opt_rescue.load()) {
    if (!g_opt_time_kernel.load()) return dispatch_kernels(p0, dtype, ensemble, s, filter);
    std::lock_guard<std::mutex> launch_lock(locks_here().dispatch);
    return timed_dispatch_kernels(p0, dtype, ensemble, s, filter);
  }
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  lspiv::PivParams p = p0;
  std::lock_guard<std::mutex> launch_lock(locks_here().dispatch);
  LSPIV_TRY(rescue_ws(c, s, p.n_tiles, &p));
  LSPIV_TRY(timed_dispatch_kernels(p, dtype, false, s, 0));
  return launch_status(lspiv::launch_piv_rescue(p, dtype, s), "rescue kernel launch failed");
}

// "v_sign" option: the engine's v negated (after the kernels and the rescue pass; the default costs nothing)
int apply_v_sign(float* d_v, int64_t n, hipStream_t s) {
  if (!g_opt_v_sign.load() || !d_v) return LSPIV_OK;
  return launch_status(lspiv::launch_negate(d_v, n, s));
}

// the families with one kernel per window size 16, 32, 64 (the entry points' checks admit no other)
using Launcher = hipError_t (*)(const lspiv::PivParams&, int, hipStream_t);
static int by_size(const Launcher (&l)[3], const lspiv::PivParams& p, int dtype, hipStream_t s) {
  return launch_status(l[p.wy == 16 ? 0 : p.wy == 32 ? 1 : 2](p, dtype, s));
}
static const Launcher kMasked[3] = {lspiv::launch_piv_masked16, lspiv::launch_piv_masked32, lspiv::launch_piv_masked64};
static const Launcher kPeak2[3] = {lspiv::launch_piv_peak2_16, lspiv::launch_piv_peak2_32, lspiv::launch_piv_peak2_64};
static const Launcher kSpof[3] = {lspiv::launch_piv_spof16, lspiv::launch_piv_spof32, lspiv::launch_piv_spof64};
static const Launcher kSpofEnsemble[3] = {lspiv::launch_piv_spof_ensemble16, lspiv::launch_piv_spof_ensemble32, lspiv::launch_piv_spof_ensemble64};
static const Launcher kDeform[3] = {lspiv::launch_piv_deform16, lspiv::launch_piv_deform32, lspiv::launch_piv_deform64};
static const Launcher kShift[3] = {lspiv::launch_piv_shift16, lspiv::launch_piv_shift32, lspiv::launch_piv_shift64};
static const Launcher kLag[3] = {lspiv::launch_piv_lag16, lspiv::launch_piv_lag32, lspiv::launch_piv_lag64};
static const Launcher kShiftEnsemble[3] = {lspiv::launch_piv_shift_ensemble16, lspiv::launch_piv_shift_ensemble32, lspiv::launch_piv_shift_ensemble64};
static const Launcher kSearch[3] = {lspiv::launch_piv_search16, lspiv::launch_piv_search32, lspiv::launch_piv_search64};

static int dispatch_kernels(const lspiv::PivParams& p, int dtype, bool ensemble, hipStream_t s, int filter) {
  if (p.peak2) {   // second correlation peak: the one-window-per-job kernels of piv_peak2_impl.h, per pair, the plain rescue pass after them
    if (ensemble || filter || p.mask || p.warped || p.shifted || p.nw) return fail(LSPIV_EUNSUPPORTED, "the second correlation peak has plain per-pair NCC kernels only");
    return by_size(kPeak2, p, dtype, s);
  }
  if (p.mask) {   // image mask: the one-window-per-job kernels of piv_masked_impl.h, per pair (the rescue pass after them reads p.mask too)
    if (ensemble || filter) return fail(LSPIV_EUNSUPPORTED, "an image mask has per-pair NCC kernels only");
    return by_size(kMasked, p, dtype, s);
  }
  if (filter) {   // SPOF phase-filtered correlation: the one-window-per-job kernels of piv_spof_impl.h, per pair or summed by one owner per window
    if (filter != LSPIV_FILTER_SPOF) return fail(LSPIV_EINVAL, "spectral filter %d not in {0: none, 1: SPOF}", filter);
    return by_size(ensemble ? kSpofEnsemble : kSpof, p, dtype, s);
  }
  if (p.warped) {   // window deformation pass: the mixed-type per-pair kernels
    if (ensemble) return fail(LSPIV_EUNSUPPORTED, "ensemble mode has no deformation kernels");
    return by_size(kDeform, p, dtype, s);
  }
  if (p.lag) {   // per-window frame lag: the shifted job with window B cut from frame t + lag (piv_lag_impl.h), per pair
    if (ensemble) return fail(LSPIV_EUNSUPPORTED, "ensemble mode has no lag kernels");
    return by_size(kLag, p, dtype, s);
  }
  if (p.shifted)   // multi-pass mode: the shifted per-pair kernels; multi-pass ensemble: one owner per window sums the shifted planes over the chunk's pairs
    return by_size(ensemble ? kShiftEnsemble : kShift, p, dtype, s);
  if (p.nw) {   // search-area mode: per-pair kernels of the search area's transform size
    if (ensemble) return fail(LSPIV_EUNSUPPORTED, "ensemble mode has no search-area kernels");
    return by_size(kSearch, p, dtype, s);
  }
  const int kind = lspiv_kernel_kind(p.wy, p.wx);
  hipError_t e;
  switch (kind) {
    case kKindEmbed16: e = lspiv::launch_piv_embed16(p, dtype, ensemble, s); break;
    case kKindEmbed32: e = lspiv::launch_piv_embed32(p, dtype, ensemble, s); break;
    case kKindEmbed64: e = lspiv::launch_piv_embed64(p, dtype, ensemble, s); break;
    case kKindFft8or16: e = p.wy == 8 ? lspiv::launch_piv_fft8(p, dtype, ensemble, s) : lspiv::launch_piv_fft16(p, dtype, ensemble, s); break;
    case kKindPfa:
      switch (p.wy) {
#define LSPIV_PFA_CASE(n) case n: e = lspiv::launch_piv_fft##n(p, dtype, ensemble, s); break;
        LSPIV_PFA_SIZES(LSPIV_PFA_CASE)
#undef LSPIV_PFA_CASE
        default: return fail(LSPIV_EUNSUPPORTED, "no prime-factor kernel for window %d", p.wy);
      }
      break;
    case kKindFft32: e = lspiv::launch_piv_fft32(p, dtype, ensemble, s); break;
    case kKindFft64: e = lspiv::launch_piv_fft64(p, dtype, ensemble, s); break;
    case kKindDirect: e = lspiv::launch_piv_direct(p, dtype, ensemble, s); break;
    case kKindDft: e = lspiv::launch_piv_dft(p, dtype, ensemble, s); break;
    case kKindDftGlobal: {   // above 128 px: the same passes on slots of HBM scratch owned by the context (one stream at a time, like the
                 // other context workspaces)
      DeviceCtx* c;
      LSPIV_TRY(get_ctx(&c));
      const size_t slot = lspiv::piv_dft_global_slot_floats(p.wy, p.wx);
      const int blocks = lspiv::piv_dft_global_blocks(ensemble ? p.n_win : p.n_tiles);
      LSPIV_TRY(ensure(&c->d_dft, &c->dft_cap, slot * (size_t)blocks * sizeof(float)));
      lspiv::PivParams q = p;
      q.dft_scratch = (float*)c->d_dft;
      q.dft_slot = slot;
      e = lspiv::launch_piv_dft_global(q, dtype, ensemble, s);
      break;
    }
    default: return fail(LSPIV_EUNSUPPORTED, "no kernel for window %dx%d", p.wy, p.wx);
  }
  return launch_status(e);
}

// "stack" signal mode: one pass over the chunk's frames leaves a keep flag per window position; the PIV kernels then run
// their threshold path with a pair threshold that always passes and consult the flags instead
int apply_signal_mode(DeviceCtx* c, lspiv::PivParams* p, int dtype, hipStream_t s) {
  if (g_opt_signal_mode.load() != 1 || p->signal_threshold < 0.0f) return LSPIV_OK;
  LSPIV_TRY(ensure(&c->d_keep, &c->keep_cap, (size_t)p->n_win));
  LSPIV_TRY(launch_status(lspiv::launch_window_signal(p->frames, dtype, (int64_t)p->n_pairs + 1, *p, p->signal_threshold, c->d_keep, s)));
  p->win_keep = c->d_keep;
  p->signal_threshold = 0.0f;
  return LSPIV_OK;
}
// run length of the window family on small grids (kWalkAnchor), 1 for per-pair kernels, a forced length as it is
static int base_alignment(int wy, int wx) {
  const int kind = lspiv_kernel_kind(wy, wx);
  if (kind < 0) return kind;
  const int walk = lspiv::walk_setting();
  if (!kind_walks(kind) || walk == 0) return 1;
  return walk > 1 ? walk : (int)lspiv::kWalkAnchor;
}
int chunk_alignment_for(int wy, int wx, int64_t n_win) {
  const int base = base_alignment(wy, wx);
  if (base <= 1 || lspiv::walk_setting() > 1) return base;     // per-pair kernels, or a forced anchor length
  return (int)lspiv::walk_anchor(wy, (uint32_t)std::min<int64_t>(n_win, 0x7fffffff));
}

// ---- what the families with kernels of a fixed size must satisfy (api_internal.h) ----
static bool fixed_square_ok(int wy, int wx) { return wy == wx && (wy == 16 || wy == 32 || wy == 64); }
int check_fixed_square(int wy, int wx, const char* what) {
  if (fixed_square_ok(wy, wx)) return LSPIV_OK;
  return fail(LSPIV_EUNSUPPORTED, "%s with window %dx%d is not supported: the window must be square and one of {16, 32, 64}", what, wy, wx);
}
int check_frame_fits_int16(int64_t H, int64_t W, const char* what) {
  if (H <= 32767 && W <= 32767) return LSPIV_OK;
  return fail(LSPIV_EINVAL, "frame (%lld,%lld): a side above 32767 does not fit %s", (long long)H, (long long)W, what);
}
int check_pair_options(const char* what, bool position_signal_ok) {
  if (!g_opt_norm_clip.load())
    return fail(LSPIV_EUNSUPPORTED, "option norm_clip = 0 is served by the block-per-window kernels only, not by %s", what);
  if (!position_signal_ok && g_opt_signal_mode.load() == 1)
    return fail(LSPIV_EUNSUPPORTED, "option signal_mode = 1 scores a window position over a chunk, the kernels of %s score the two windows of a "
                "pair: not supported", what);
  return LSPIV_OK;
}
int check_shift(int wy, int wx, int64_t H, int64_t W) {
  LSPIV_TRY(check_fixed_square(wy, wx, "shifted pass"));
  LSPIV_TRY(check_frame_fits_int16(H, W, "the int16 offsets"));
  return check_multipass_options();
}
int check_spof(int wy, int wx) {
  LSPIV_TRY(check_fixed_square(wy, wx, "SPOF-filtered correlation"));
  return check_pair_options("SPOF-filtered correlation");
}
// second correlation peak: besides, the exclusion radius lies in 1 .. N / 4 and the output block is there, one aligned float4 per window
static int check_peak2(int wy, int wx, int peak_exclusion, const void* peak2, bool in_hbm) {
  LSPIV_TRY(check_fixed_square(wy, wx, "the second correlation peak"));
  LSPIV_TRY(check_pair_options("the second correlation peak"));
  if (peak_exclusion < 1 || peak_exclusion > wy / 4)
    return fail(LSPIV_EINVAL, "peak_exclusion %d not in 1 .. %d (a quarter of the window)", peak_exclusion, wy / 4);
  if (!peak2) return fail(LSPIV_EINVAL, "peak2 is NULL");
  if (in_hbm && ((uintptr_t)peak2 & 15u)) return fail(LSPIV_EINVAL, "d_peak2 is not 16-byte aligned");   // (a host block goes through the context's own)
  return LSPIV_OK;
}
// ... on planes: any plane of 4 .. 4096 px per side, the radius within a quarter of the shorter side
static int check_second_peak(const void* planes, const void* peak2, int64_t n_planes, int wy, int wx, int peak_exclusion) {
  if (!planes || !peak2) return fail(LSPIV_EINVAL, "NULL buffer");
  if (n_planes < 0 || n_planes >= (int64_t)1 << 31) return fail(LSPIV_EINVAL, "%lld planes: not in 0 .. 2^31 - 1", (long long)n_planes);
  if (wy < 4 || wx < 4 || wy > 4096 || wx > 4096) return fail(LSPIV_EINVAL, "plane %dx%d outside 4 .. 4096", wy, wx);
  if (peak_exclusion < 1 || peak_exclusion > std::min(wy, wx) / 4)
    return fail(LSPIV_EINVAL, "peak_exclusion %d not in 1 .. %d (a quarter of the plane)", peak_exclusion, std::min(wy, wx) / 4);
  return LSPIV_OK;
}
// image mask: besides, k_min lies in 2 .. N^2
static int check_masked(int wy, int wx, const void* mask, int64_t k_min) {
  LSPIV_TRY(check_fixed_square(wy, wx, "masked correlation"));
  LSPIV_TRY(check_pair_options("masked correlation"));
  if (!mask) return fail(LSPIV_EINVAL, "mask is NULL");
  if (k_min < 2 || k_min > (int64_t)wy * wx)
    return fail(LSPIV_EINVAL, "k_min %lld not in 2 .. %d (max(2, ceil(mask_coverage_min * window area)))", (long long)k_min, wy * wx);
  return LSPIV_OK;
}

}  // namespace lspiv_api

using namespace lspiv_api;

uint32_t lspiv::job_slots(int waves_per_simd, int groups) {
  static const int cus = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return 256;
    return prop.multiProcessorCount;
  }();
  return (uint32_t)(cus * 4 * waves_per_simd * groups);
}

extern "C" {

int lspiv_kernel_times(float* ms, int cap, int* n) {
  if (!ms || !n || cap < 0) return fail(LSPIV_EINVAL, "bad argument");
  std::lock_guard<std::mutex> launch_lock(locks_here().dispatch);
  KernelTimer& t = g_timers[current_device_slot()];
  const int have = std::min(std::min(t.n, kTimerRing), cap);
  for (int i = 0; i < have; ++i) {
    const int k = (t.n - have + i) % kTimerRing;
    HIP_TRY(hipEventSynchronize(t.e1[k]));
    HIP_TRY(hipEventElapsedTime(&ms[i], t.e0[k], t.e1[k]));
  }
  *n = have;
  t.n = 0;
  return LSPIV_OK;
}

int lspiv_rescue_stats(void* stream, int64_t* stats) {
  if (!stats) return fail(LSPIV_EINVAL, "stats is NULL");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  void* base = nullptr;
  {
    std::lock_guard<std::mutex> lk(locks_here().lists);
    for (auto& w : c->rescue) if (w.stream == s) base = w.base;
  }
  for (int k = 0; k < 5; ++k) stats[k] = 0;
  if (!base) return LSPIV_OK;   // no pass has run on this stream
  lspiv::RescueHdr h;
  HIP_TRY(hipMemcpyAsync(&h, base, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  stats[0] = h.last_fit; stats[1] = h.last_amb;
  stats[2] = (int64_t)h.total_fit; stats[3] = (int64_t)h.total_amb; stats[4] = (int64_t)h.total_windows;
  return LSPIV_OK;
}

int lspiv_debug_rescue_lists(void* stream, uint32_t* fit, int64_t cap_fit, uint32_t* amb, int64_t cap_amb, int64_t* counts) {
  if (!counts || cap_fit < 0 || cap_amb < 0 || (cap_fit && !fit) || (cap_amb && !amb)) return fail(LSPIV_EINVAL, "counts is NULL, or a list without its buffer");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  std::lock_guard<std::mutex> launch_lock(locks_here().dispatch);   // no launch regrows or refills the lists meanwhile
  void* base = nullptr;
  size_t ws_cap_fit = 0, ws_cap_amb = 0;
  {
    std::lock_guard<std::mutex> lk(locks_here().lists);
    for (auto& w : c->rescue) if (w.stream == s) { base = w.base; ws_cap_fit = w.cap_fit; ws_cap_amb = w.cap_amb; }
  }
  counts[0] = counts[1] = 0;
  if (!base) return LSPIV_OK;   // no pass has run on this stream
  lspiv::RescueHdr h;
  HIP_TRY(hipMemcpyAsync(&h, base, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t n_fit = std::min<size_t>(h.last_fit, ws_cap_fit), n_amb = std::min<size_t>(h.last_amb, ws_cap_amb);
  counts[0] = (int64_t)n_fit; counts[1] = (int64_t)n_amb;
  const char* d_fit = (const char*)base + RescueCaps::hdr_bytes;
  const char* d_amb = d_fit + ws_cap_fit * sizeof(uint4);
  const size_t c_fit = std::min<size_t>(n_fit, (size_t)cap_fit), c_amb = std::min<size_t>(n_amb, (size_t)cap_amb);
  if (c_fit) HIP_TRY(hipMemcpyAsync(fit, d_fit, c_fit * sizeof(uint4), hipMemcpyDeviceToHost, s));
  if (c_amb) HIP_TRY(hipMemcpyAsync(amb, d_amb, c_amb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return LSPIV_OK;
}

int lspiv_kernel_kind(int wy, int wx) {
  if (wy < 2 || wx < 2 || wy > LSPIV_MAX_WINDOW || wx > LSPIV_MAX_WINDOW) return LSPIV_EUNSUPPORTED;
  if (wy > 64 || wx > 64) return lspiv::piv_dft_fits(wy, wx) ? kKindDft : kKindDftGlobal;   // 2-D DFT of any shape: LDS-resident up to 128 x 128, HBM slots above
  // the area from which the DFT kernel takes over from the direct one (below), fixed at the first call
  static const int dft_min_area = getenv("LSPIV_DFT_MIN_AREA") ? atoi(getenv("LSPIV_DFT_MIN_AREA")) : 1500;
  const auto block_per_window = [&] { return wy * wx >= dft_min_area && lspiv::piv_dft_fits(wy, wx) ? kKindDft : kKindDirect; };
  // the un-clipped reading of A3 lives in the block-per-window kernels only (a switch, not a tuned path); so do the non-square windows
  if (!g_opt_norm_clip.load() || wy != wx) return block_per_window();
  // A/B switches, read at every call: the P * 2^m sizes without their own FFT kernels; the direct kernel for every other size
  const bool no_pfa = getenv("LSPIV_NO_PFA") != nullptr, no_embed = getenv("LSPIV_NO_EMBED") != nullptr;
  if (wy == 32) return kKindFft32;
  if (wy == 64) return kKindFft64;
  if (wy == 16) return kKindFft8or16;
  if (!no_pfa) {
    if (wy == 8) return kKindFft8or16;
    switch (wy) {
#define LSPIV_PFA_CASE(n) case n:
      LSPIV_PFA_SIZES(LSPIV_PFA_CASE)
#undef LSPIV_PFA_CASE
        return kKindPfa;
      default: break;
    }
  }
  if (!no_embed && wy >= 4 && wy <= 8) return kKindEmbed16;
  if (!no_embed && wy >= 9 && wy <= 15) return kKindEmbed32;
  // 17..20: the direct kernel's N^4 multiply-adds are still cheaper than two 64-point transforms per window (measured
  // crossover between 20 and 22, tools/direct_bench.py)
  if (!no_embed && wy > 20 && wy < 32) return kKindEmbed64;
  // what is left -- non-square windows, odd 17 / 19 / 33 .. 63: the direct spatial kernel costs wy wx multiply-adds per plane
  // sample, the LDS-resident DFT passes (wy + wx) complex ones, a composite length in two shorter passes.  Measured on
  // 785 x 875 frames (tools/gpu_ab_direct.sh; M window pairs/s, direct | DFT): 40 x 24 23.2 | 13.1, 35 x 35 14.0 | 12.2,
  // 48 x 32 10.4 | 11.9, 41 x 41 8.1 | 9.2, 64 x 32 6.1 | 11.3, 49 x 49 3.6 | 10.7, 63 x 63 1.6 | 7.2 -- the DFT kernel takes over
  // from 1500 samples per window (LSPIV_DFT_MIN_AREA)
  return block_per_window();
}

int lspiv_grid_shape(int64_t H, int64_t W, int wy, int wx, int oy, int ox, int64_t* n_rows, int64_t* n_cols) {
  if (!n_rows || !n_cols) return fail(LSPIV_EINVAL, "output pointer is NULL");
  LSPIV_TRY(check_window(wy, wx, oy, ox));
  *n_rows = axis_shape(H, wy, oy);
  *n_cols = axis_shape(W, wx, ox);
  return LSPIV_OK;
}

int lspiv_grid_coords(int64_t H, int64_t W, int wy, int wx, int oy, int ox, int64_t* rows, int64_t* cols) {
  int64_t nr, nc;
  LSPIV_TRY(lspiv_grid_shape(H, W, wy, wx, oy, ox, &nr, &nc));
  if ((nr > 0 && !rows) || (nc > 0 && !cols)) return fail(LSPIV_EINVAL, "output pointer is NULL");
  // ffpiv.window.get_axis_coords restated: int64(arange(n) * (win - overlap) + win / 2.0)
  for (int64_t k = 0; k < nr; ++k) rows[k] = (int64_t)std::floor((double)k * (wy - oy) + wy / 2.0);
  for (int64_t k = 0; k < nc; ++k) cols[k] = (int64_t)std::floor((double)k * (wx - ox) + wx / 2.0);
  return LSPIV_OK;
}

int64_t lspiv_required_bytes(int64_t T, int64_t H, int64_t W, int dtype, int wy, int wx, int oy, int ox,
                             int with_planes) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  if (dtype < 0 || dtype > 2 || T < 2) return fail(LSPIV_EINVAL, "bad dtype/T");
  const int64_t n_tiles = (T - 1) * g.n_rows * g.n_cols;
  int64_t b = T * H * W * (int64_t)elem_size(dtype) + 4 * n_tiles * 4;
  if (with_planes) b += n_tiles * wy * wx * 4;
  if (g_opt_rescue.load()) b += (int64_t)rescue_caps(n_tiles).bytes();   // the rescue lists of the launch stream
  return b;
}

int lspiv_available_bytes(int64_t* free_bytes, int64_t* total_bytes) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  size_t f = 0, t = 0;
  HIP_TRY(hipMemGetInfo(&f, &t));
  // workspaces this library already holds are reusable, count them as free
  f += c->frames_cap + c->out_cap + c->planes_cap;
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return LSPIV_OK;
}

// Without a grid: the alignment that is right for EVERY frame shape -- the longest run length the family uses, a multiple of the
// shorter one (ABI 5; it returned the short one before, which cut chunks off the anchors of large grids: ADVICE r05)
int lspiv_chunk_alignment(int wy, int wx) {
  const int base = base_alignment(wy, wx);
  if (base <= 1 || lspiv::walk_setting() > 1) return base;
  static_assert(lspiv::kWalkAnchorLong % lspiv::kWalkAnchor == 0, "the long anchor must be a multiple of the short one");
  return (int)lspiv::kWalkAnchorLong;
}
int lspiv_chunk_alignment_grid(int64_t H, int64_t W, int wy, int wx, int oy, int ox) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  return chunk_alignment_for(wy, wx, g.n_rows * g.n_cols);
}

// what a per-pair launch is besides its window, all zero for the plain one (the exported wrappers have run the mode's check):
struct PairMode {
  int nw = 0;                      // the window inside the search area wy x wx (search-area mode)
  int filter = 0;                  // LSPIV_FILTER_SPOF
  const uint8_t* mask = nullptr;   // the image mask of the frames' shape, where the entry point's frames are: HBM (_dev) or host
  int64_t k_min = 0;               // ... and the smallest count of valid samples of a window
  float* peak2 = nullptr;          // the second-peak block n_tiles x {u2, v2, corr2, peak_ratio}, where the entry point's results are: HBM (_dev) or host
  int peak_excl = 0;               // ... and the exclusion radius around the primary peak
  bool per_pair() const { return nw || filter || mask || peak2; }   // one window pair per job: no anchors to cut launches at
};
// what every device-pointer entry point checks first
static int check_dev_call(const void* d_frames, const void* d_out, int64_t pair_offset) {
  if (!d_frames || !d_out) return fail(LSPIV_EINVAL, "d_frames / d_out is NULL");
  if (pair_offset < 0) return fail(LSPIV_EINVAL, "pair_offset %lld is negative", (long long)pair_offset);
  return LSPIV_OK;
}
static int piv_pairs_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                         float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes, void* stream, const PairMode& m) {
  LSPIV_TRY(check_dev_call(d_frames, d_out, pair_offset));
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  lspiv::PivParams p;
  LSPIV_TRY(fill_params(&p, d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, g));
  if (m.nw) set_search_window(&p, m.nw);
  p.pair_offset = pair_offset;
  set_results(&p, d_out, p.n_tiles, 0, d_corr_planes, 0);
  p.mask = m.mask;
  p.k_min = (uint32_t)m.k_min;
  p.peak2 = m.peak2;
  p.peak_excl = m.peak_excl;
  p.peak2_v_neg = m.peak2 ? g_opt_v_sign.load() : 0;
  hipStream_t s = on_stream(c, stream);
  LSPIV_TRY(apply_signal_mode(c, &p, dtype, s));
  LSPIV_TRY(dispatch(p, dtype, false, s, m.filter));
  return apply_v_sign(p.v, (int64_t)p.n_tiles, s);
}

int lspiv_piv_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy,
                           int ox, float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes,
                           void* stream) {
  return piv_pairs_dev(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, d_out, d_corr_planes, stream, {});
}

int lspiv_spof_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

int lspiv_piv_spof_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                                float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes, void* stream) {
  LSPIV_TRY(check_spof(wy, wx));
  return piv_pairs_dev(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, d_out, d_corr_planes, stream, {.filter = LSPIV_FILTER_SPOF});
}

int lspiv_mask_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

int lspiv_piv_masked_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                                  const uint8_t* d_mask, int64_t k_min, float signal_threshold, int64_t pair_offset, float* d_out,
                                  float* d_corr_planes, void* stream) {
  LSPIV_TRY(check_masked(wy, wx, d_mask, k_min));
  return piv_pairs_dev(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, d_out, d_corr_planes, stream,
                       {.mask = d_mask, .k_min = k_min});
}

int lspiv_peak2_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

int lspiv_piv_peak2_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                                 float signal_threshold, int64_t pair_offset, int peak_exclusion, float* d_out, float* d_peak2,
                                 float* d_corr_planes, void* stream) {
  LSPIV_TRY(check_peak2(wy, wx, peak_exclusion, d_peak2, true));
  return piv_pairs_dev(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, d_out, d_corr_planes, stream,
                       {.peak2 = d_peak2, .peak_excl = peak_exclusion});
}

int lspiv_second_peak_dev(const float* d_planes, int64_t n_planes, int wy, int wx, int peak_exclusion, float* d_peak2, void* stream) {
  LSPIV_TRY(check_second_peak(d_planes, d_peak2, n_planes, wy, wx, peak_exclusion));
  return launch_on(stream, [&](hipStream_t s) {
    return lspiv::launch_second_peak(d_planes, (uint32_t)n_planes, wy, wx, peak_exclusion, g_opt_border.load(), g_opt_v_sign.load(), d_peak2, s);
  });
}

int lspiv_search_supported(int say, int sax, int wy, int wx) { return search_shape_ok(say, sax, wy, wx) ? 1 : 0; }

int lspiv_piv_search_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int say, int sax, int wy, int wx,
                                  int oy, int ox, float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes,
                                  void* stream) {
  LSPIV_TRY(check_search(say, sax, wy, wx));
  return piv_pairs_dev(d_frames, dtype, T, H, W, say, sax, oy, ox, signal_threshold, pair_offset, d_out, d_corr_planes, stream, {.nw = wy});
}

// ---- multi-pass PIV (include/lspiv.h) ---------------------------------------------------------------
// one shifted pass on stream s: kernel + rescue pass (both write the residual), then the clamped offset is added; v_sign is the caller's
static int shift_pass(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox, float signal_threshold,
                      int64_t pair_offset, const int16_t* d_shift, float* d_out, float* d_planes, hipStream_t s, lspiv::PivParams* out_p) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  lspiv::PivParams p;
  LSPIV_TRY(fill_params(&p, d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, g));
  p.pair_offset = pair_offset;
  p.shifted = 1;
  p.shift = d_shift;
  set_results(&p, d_out, p.n_tiles, 0, d_planes, 0);
  LSPIV_TRY(dispatch(p, dtype, false, s));
  LSPIV_TRY(launch_status(lspiv::launch_add_shift(p, s)));
  if (out_p) *out_p = p;
  return LSPIV_OK;
}

static int pass_grid(int64_t H, int64_t W, int wy, int wx, int oy, int ox, lspiv::PassGrid* pg) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  if ((wy & 1) || (wx & 1)) return fail(LSPIV_EINVAL, "window %dx%d: the passes of a chain are even", wy, wx);
  *pg = {wy, wx, wy - oy, wx - ox, (int)g.n_rows, (int)g.n_cols};
  return LSPIV_OK;
}

// the clamped offsets of a pass, as the kernels used them: the predictor clamps what it stores, so its output IS the clamped array
// ---- window deformation passes (include/lspiv.h) ------------------------------------------------------
// The warped frames of one BATCH of pairs live in a per-device workspace of at most kDeformWsBytes (one frame at least): a pass runs
// batch by batch -- warp, mixed-type kernel, rescue pass, nodes added -- before the workspace is reused.  Results are per pair, so the
// batching cannot change a bit.
constexpr size_t kDeformWsBytes = (size_t)256 << 20;
// test hook: LSPIV_DEFORM_WS_BYTES stands in for kDeformWsBytes (read on every call), so that a small stack runs in several batches
static size_t deform_ws_bytes() {
  if (const char* e = getenv("LSPIV_DEFORM_WS_BYTES")) return (size_t)std::max<long long>(0, atoll(e));
  return kDeformWsBytes;
}
static int64_t deform_batch_pairs(int64_t n_pairs, int64_t H, int64_t W) {
  const int64_t fit = std::max<int64_t>(1, (int64_t)(deform_ws_bytes() / ((size_t)H * (size_t)W * sizeof(float))));
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_pairs, fit), 65535));   // (65535: the warp's grid runs the pairs along z)
}
static int check_deform(int wy, int wx, int oy, int ox, int64_t H, int64_t W) {
  if (!fixed_square_ok(wy, wx) || oy != ox)
    return fail(LSPIV_EUNSUPPORTED, "deformation pass with window %dx%d, overlap (%d,%d) is not supported: the window must be square and one of "
                "{16, 32, 64}, the overlap the same on both axes", wy, wx, oy, ox);
  LSPIV_TRY(check_frame_fits_int16(H, W, "the nodes' range"));
  return check_multipass_options();
}
// one deformation pass on stream s: d_nodes (T-1) * n_win * {v, u} -> d_out [u | v | corr_max | s2n] of all pairs (kernel orientation;
// v_sign is the caller's).  The caller holds the device's multipass lock: the workspace is shared
static int deform_pass(DeviceCtx* c, const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int n, int ov, float signal_threshold,
                       const int32_t* d_nodes, float* d_out, float* d_planes, hipStream_t s) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, n, n, ov, ov, &g));
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  const int64_t P = T - 1, n_win = g.n_rows * g.n_cols, batch = deform_batch_pairs(P, H, W);
  const size_t frame_elems = (size_t)H * W, n_tiles = (size_t)P * n_win;
  LSPIV_TRY(ensure(&c->d_deform, &c->deform_cap, (size_t)batch * frame_elems * sizeof(float)));
  for (int64_t b0 = 0; b0 < P; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, P - b0);
    lspiv::PivParams p;
    LSPIV_TRY(fill_params(&p, (const char*)d_frames + (size_t)b0 * frame_elems * elem_size(dtype), dtype, nb + 1, H, W, n, n, ov, ov,
                          signal_threshold, g));
    const size_t t0 = (size_t)b0 * n_win;
    p.nodes = d_nodes + 2 * t0;
    p.warped = c->d_deform;
    set_results(&p, d_out, n_tiles, t0, d_planes, (size_t)n * n);
    LSPIV_TRY(launch_status(lspiv::launch_deform_warp(p, dtype, c->d_deform, s)));
    LSPIV_TRY(dispatch(p, dtype, false, s));
    LSPIV_TRY(launch_status(lspiv::launch_add_nodes(p, s)));
  }
  return LSPIV_OK;
}

static int multipass_dev(DeviceCtx* c, const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes,
                         float signal_threshold, int64_t pair_offset, float* d_out, float* d_planes, int16_t* d_shift_out, hipStream_t s,
                         int n_deform = 0) {
  LSPIV_TRY(check_dev_call(d_frames, d_out, pair_offset));
  if (!passes) return fail(LSPIV_EINVAL, "passes is NULL");
  if (n_passes < 1 || n_passes > 8) return fail(LSPIV_EINVAL, "n_passes %d not in 1..8", n_passes);
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  LSPIV_TRY(check_multipass_options());
  LSPIV_TRY(check_frame_fits_int16(H, W, "the int16 offsets"));
  lspiv::PassGrid pg[8];
  size_t max_tiles = 0;
  for (int k = 0; k < n_passes; ++k) {
    const int* q = passes + 4 * k;
    if (q[0] != q[1]) return fail(LSPIV_EINVAL, "pass %d: window %dx%d is not square", k, q[0], q[1]);
    if (k > 0 && !fixed_square_ok(q[0], q[1]))
      return fail(LSPIV_EUNSUPPORTED, "pass %d: window %dx%d is not supported: the windows of passes after the first must be one of {16, 32, 64}", k, q[0], q[1]);
    if (k > 0 && q[0] > passes[4 * (k - 1)]) return fail(LSPIV_EINVAL, "pass %d: window %d is larger than pass %d's %d", k, q[0], k - 1, passes[4 * (k - 1)]);
    LSPIV_TRY(pass_grid(H, W, q[0], q[1], q[2], q[3], &pg[k]));
    if (k + 1 < n_passes) max_tiles = std::max(max_tiles, (size_t)(T - 1) * pg[k].n_rows * pg[k].n_cols);
  }
  const int* last = passes + 4 * (n_passes - 1);
  const size_t last_tiles = (size_t)(T - 1) * pg[n_passes - 1].n_rows * pg[n_passes - 1].n_cols;
  if (n_deform < 0 || n_deform > 4) return fail(LSPIV_EINVAL, "n_deform %d not in 0..4", n_deform);
  if (n_deform) LSPIV_TRY(check_deform(last[0], last[1], last[2], last[3], H, W));
  if (n_passes == 1 && !n_deform) {
    if (d_shift_out) HIP_TRY(hipMemsetAsync(d_shift_out, 0, last_tiles * 2 * sizeof(int16_t), s));
    return lspiv_piv_pairs_dev_at(d_frames, dtype, T, H, W, last[0], last[1], last[2], last[3], signal_threshold, pair_offset, d_out, d_planes, s);
  }
  // the passes of one chain are issued under one lock: they share the workspace below, and a second chain on the same stream must come
  // after this one's last pass, not between two of them (chains on DIFFERENT streams of one device still share it: one stream at a time)
  std::lock_guard<std::mutex> chain_lock(locks_here().multipass);
  // workspace: two result blocks of the largest intermediate pass (ping-pong) and one offset array of the largest pass that takes one
  size_t max_shift = 0;
  for (int k = 1; k < n_passes; ++k) max_shift = std::max(max_shift, (size_t)(T - 1) * pg[k].n_rows * pg[k].n_cols);
  const size_t blk = (4 * max_tiles * sizeof(float) + 255) & ~(size_t)255;
  const size_t shift_bytes = (max_shift * 2 * sizeof(int16_t) + 255) & ~(size_t)255;
  LSPIV_TRY(ensure(&c->d_mp, &c->mp_cap, 2 * blk + shift_bytes + (n_deform ? last_tiles * 2 * sizeof(int32_t) : 0)));
  float* res[2] = {reinterpret_cast<float*>(c->d_mp), reinterpret_cast<float*>((char*)c->d_mp + blk)};
  int16_t* ws_shift = reinterpret_cast<int16_t*>((char*)c->d_mp + 2 * blk);
  int32_t* ws_nodes = reinterpret_cast<int32_t*>((char*)c->d_mp + 2 * blk + shift_bytes);
  // pass 0: today's per-timestep path on its own grid, in the kernels' orientation (no v_sign before the end)
  {
    const int* q = passes;
    float* r0 = n_passes == 1 ? d_out : res[0];   // (a chain of one pass that deformation passes follow)
    Grid g;
    LSPIV_TRY(make_grid(H, W, q[0], q[1], q[2], q[3], &g));
    lspiv::PivParams p;
    LSPIV_TRY(fill_params(&p, d_frames, dtype, T, H, W, q[0], q[1], q[2], q[3], signal_threshold, g));
    p.pair_offset = pair_offset;
    set_results(&p, r0, p.n_tiles, 0, nullptr, 0);
    LSPIV_TRY(dispatch(p, dtype, false, s));
    if (n_passes == 1 && d_shift_out) HIP_TRY(hipMemsetAsync(d_shift_out, 0, last_tiles * 2 * sizeof(int16_t), s));
  }
  for (int k = 1; k < n_passes; ++k) {
    const int* q = passes + 4 * k;
    const bool final_pass = k == n_passes - 1;
    const float* prev = res[(k - 1) & 1];
    const size_t prev_tiles = (size_t)(T - 1) * pg[k - 1].n_rows * pg[k - 1].n_cols;
    int16_t* shift = final_pass && d_shift_out ? d_shift_out : ws_shift;
    LSPIV_TRY(launch_status(lspiv::launch_predict_shift(prev, prev + prev_tiles, (uint32_t)(T - 1), (int)H, (int)W, pg[k - 1], pg[k], shift, s)));
    LSPIV_TRY(shift_pass(d_frames, dtype, T, H, W, q[0], q[1], q[2], q[3], signal_threshold, pair_offset, shift, final_pass ? d_out : res[k & 1],
                         final_pass && !n_deform ? d_planes : nullptr, s, nullptr));
  }
  // the deformation passes on the final grid, each fed with the (u, v) of the pass before it: the nodes are read off d_out, then the
  // pass overwrites it (stream order); the planes are those of the last one
  for (int d = 0; d < n_deform; ++d) {
    const lspiv::PassGrid& fg = pg[n_passes - 1];
    LSPIV_TRY(launch_status(lspiv::launch_predict_deform(d_out, d_out + last_tiles, (uint32_t)(T - 1), fg.n_rows, fg.n_cols, ws_nodes, s)));
    LSPIV_TRY(deform_pass(c, d_frames, dtype, T, H, W, last[0], last[2], signal_threshold, ws_nodes, d_out, d == n_deform - 1 ? d_planes : nullptr, s));
  }
  return apply_v_sign(d_out + last_tiles, (int64_t)last_tiles, s);
}

int lspiv_shift_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

int lspiv_piv_shift_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                                 float signal_threshold, int64_t pair_offset, const int16_t* d_shift, float* d_out, float* d_corr_planes,
                                 void* stream) {
  LSPIV_TRY(check_dev_call(d_frames, d_out, pair_offset));
  LSPIV_TRY(check_shift(wy, wx, H, W));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  lspiv::PivParams p;
  LSPIV_TRY(shift_pass(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, d_shift, d_out, d_corr_planes, s, &p));
  return apply_v_sign(p.v, (int64_t)p.n_tiles, s);
}

int lspiv_piv_predict_shift_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t H, int64_t W, int cwy, int cwx, int coy, int cox,
                                int fwy, int fwx, int foy, int fox, int16_t* d_shift, void* stream) {
  if (!d_u || !d_v || !d_shift) return fail(LSPIV_EINVAL, "NULL argument");
  if (n_pairs < 0) return fail(LSPIV_EINVAL, "n_pairs %lld is negative", (long long)n_pairs);
  LSPIV_TRY(check_frame_fits_int16(H, W, "the int16 offsets"));
  lspiv::PassGrid cg, fg;
  LSPIV_TRY(pass_grid(H, W, cwy, cwx, coy, cox, &cg));
  LSPIV_TRY(pass_grid(H, W, fwy, fwx, foy, fox, &fg));
  if (n_pairs * (int64_t)fg.n_rows * fg.n_cols >= (int64_t)1 << 31 || n_pairs * (int64_t)cg.n_rows * cg.n_cols >= (int64_t)1 << 31)
    return fail(LSPIV_EINVAL, "too many windows for one launch (limit 2^31)");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_predict_shift(d_u, d_v, (uint32_t)n_pairs, (int)H, (int)W, cg, fg, d_shift, s); });
}

// ---- per-window frame lag (include/lspiv.h) ----------------------------------------------------------------
int lspiv_lag_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

static int check_lag(int wy, int wx, int64_t H, int64_t W, int64_t T, int64_t n_pairs, int lag_form, int k, int target128, const void* lag_in,
                     const void* shift_in) {
  LSPIV_TRY(check_fixed_square(wy, wx, "a frame lag"));
  LSPIV_TRY(check_frame_fits_int16(H, W, "the int16 offsets"));
  LSPIV_TRY(check_pair_options("a frame lag"));
  if (n_pairs < 1 || n_pairs > T - 1) return fail(LSPIV_ESHAPE, "n_pairs %lld not in 1 .. T - 1 = %lld", (long long)n_pairs, (long long)(T - 1));
  if (lag_form < LSPIV_LAG_UNIFORM || lag_form > LSPIV_LAG_ADAPTIVE) return fail(LSPIV_EINVAL, "lag_form %d not in 0 .. 3", lag_form);
  if ((lag_form == LSPIV_LAG_UNIFORM || lag_form == LSPIV_LAG_ADAPTIVE) && (k < 1 || k > lspiv::kMaxLag))
    return fail(LSPIV_EINVAL, "lag %d not in 1 .. %d", k, lspiv::kMaxLag);
  if ((lag_form == LSPIV_LAG_WINDOW || lag_form == LSPIV_LAG_TABLE) && !lag_in) return fail(LSPIV_EINVAL, "lag_form %d without a lag array", lag_form);
  if (lag_form == LSPIV_LAG_ADAPTIVE) {
    if (shift_in || lag_in) return fail(LSPIV_EINVAL, "the adaptive form predicts its own lags and offsets: d_lag and d_shift must be NULL");
    if (target128 < 1 || target128 > 64 * wy) return fail(LSPIV_EINVAL, "target %d / 128 px not in (0, window / 2]", target128);
  }
  return LSPIV_OK;
}

// the pass itself on stream s: the table, the lag kernel + rescue pass (both write the residual of the frame pair (t, t + lag)), then the
// offset is added and the sum divided by the lag.  p_lag1: the lag-1 pass of the adaptive form (d_out holds its field, overwritten here)
static int lag_pass(DeviceCtx* c, const void* d_frames, int dtype, int64_t T, int64_t n_pairs, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                    float signal_threshold, int64_t pair_offset, int lag_form, int k, int target128, const uint8_t* d_lag_in,
                    const int16_t* d_shift_in, float* d_out, float* d_planes, uint8_t* d_lag_out, int16_t* d_shift_out, hipStream_t s) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  lspiv::PivParams p;
  LSPIV_TRY(fill_params(&p, d_frames, dtype, n_pairs + 1, H, W, wy, wx, oy, ox, signal_threshold, g));   // n_pairs pairs; the frames behind them are the lags'
  p.pair_offset = pair_offset;
  set_results(&p, d_out, p.n_tiles, 0, nullptr, 0);
  const int16_t* shift = d_shift_in;
  if (lag_form == LSPIV_LAG_ADAPTIVE) {
    // pass 0: the plain per-timestep path at lag 1 on this grid (lspiv_piv_pairs_dev_at's launch, kernel orientation: no v_sign)
    LSPIV_TRY(apply_signal_mode(c, &p, dtype, s));
    LSPIV_TRY(dispatch(p, dtype, false, s));
    int16_t* ws_shift = d_shift_out;
    if (!ws_shift) {
      LSPIV_TRY(ensure(&c->d_mp, &c->mp_cap, (size_t)p.n_tiles * 2 * sizeof(int16_t)));
      ws_shift = static_cast<int16_t*>(c->d_mp);
    }
    lspiv::PassGrid pg;
    LSPIV_TRY(pass_grid(H, W, wy, wx, oy, ox, &pg));
    LSPIV_TRY(launch_status(lspiv::launch_lag_predict(p.u, p.v, p.n_pairs, T, (int)H, (int)W, pg, k, target128, d_lag_out, ws_shift, s)));
    shift = ws_shift;
  } else {
    LSPIV_TRY(launch_status(lspiv::launch_lag_fill(lag_form, k, d_lag_in, p.n_pairs, p.n_win, T, d_lag_out, s)));
  }
  p.planes = d_planes;
  p.shifted = 1;
  p.shift = shift;
  p.lag = d_lag_out;
  LSPIV_TRY(dispatch(p, dtype, false, s));
  LSPIV_TRY(launch_status(lspiv::launch_lag_divide(p, d_shift_out, s)));
  return apply_v_sign(p.v, (int64_t)p.n_tiles, s);
}

int lspiv_piv_lag_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t n_pairs, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                               float signal_threshold, int64_t pair_offset, int lag_form, int k, int target128, const uint8_t* d_lag,
                               const int16_t* d_shift, float* d_out, float* d_corr_planes, uint8_t* d_lag_out, int16_t* d_shift_out,
                               void* stream) {
  LSPIV_TRY(check_dev_call(d_frames, d_out, pair_offset));
  if (!d_lag_out) return fail(LSPIV_EINVAL, "d_lag_out is NULL");
  LSPIV_TRY(check_lag(wy, wx, H, W, T, n_pairs, lag_form, k, target128, d_lag, d_shift));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  std::lock_guard<std::mutex> chain_lock(locks_here().multipass);   // (the adaptive form's offsets may live in the multi-pass workspace)
  return lag_pass(c, d_frames, dtype, T, n_pairs, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, lag_form, k, target128, d_lag, d_shift,
                  d_out, d_corr_planes, d_lag_out, d_shift_out, on_stream(c, stream));
}

int lspiv_lag_predict_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                          int k_max, int target128, uint8_t* d_lag, int16_t* d_shift, void* stream) {
  if (!d_u || !d_v || !d_lag || !d_shift) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(check_fixed_square(wy, wx, "a frame lag"));
  LSPIV_TRY(check_frame_fits_int16(H, W, "the int16 offsets"));
  if (n_pairs < 0 || n_pairs > T - 1) return fail(LSPIV_ESHAPE, "n_pairs %lld not in 0 .. T - 1 = %lld", (long long)n_pairs, (long long)(T - 1));
  if (k_max < 1 || k_max > lspiv::kMaxLag) return fail(LSPIV_EINVAL, "k_max %d not in 1 .. %d", k_max, lspiv::kMaxLag);
  if (target128 < 1 || target128 > 64 * wy) return fail(LSPIV_EINVAL, "target %d / 128 px not in (0, window / 2]", target128);
  lspiv::PassGrid pg;
  LSPIV_TRY(pass_grid(H, W, wy, wx, oy, ox, &pg));
  if (n_pairs * (int64_t)pg.n_rows * pg.n_cols >= (int64_t)1 << 31) return fail(LSPIV_EINVAL, "too many windows for one launch (limit 2^31)");
  return launch_on(stream, [&](hipStream_t s) {
    return lspiv::launch_lag_predict(d_u, d_v, (uint32_t)n_pairs, T, (int)H, (int)W, pg, k_max, target128, d_lag, d_shift, s);
  });
}

int lspiv_piv_multipass_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes,
                               float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes, int16_t* d_shift_out, void* stream) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  return multipass_dev(c, d_frames, dtype, T, H, W, n_passes, passes, signal_threshold, pair_offset, d_out, d_corr_planes, d_shift_out,
                       on_stream(c, stream));
}

int lspiv_deform_supported(int wy, int wx) { return fixed_square_ok(wy, wx) ? 1 : 0; }

int64_t lspiv_deform_required_bytes(int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox) {
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  return deform_batch_pairs(T - 1, H, W) * H * W * (int64_t)sizeof(float) + (T - 1) * g.n_rows * g.n_cols * 2 * (int64_t)sizeof(int32_t);
}

int lspiv_piv_predict_deform_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t n_rows, int64_t n_cols, int32_t* d_nodes, void* stream) {
  if (!d_u || !d_v || !d_nodes) return fail(LSPIV_EINVAL, "NULL argument");
  if (n_pairs < 0 || n_rows < 1 || n_cols < 1) return fail(LSPIV_ESHAPE, "grid (%lld, %lld, %lld) invalid", (long long)n_pairs, (long long)n_rows, (long long)n_cols);
  if (n_rows > 32767 || n_cols > 32767 || n_pairs * n_rows * n_cols >= (int64_t)1 << 31)
    return fail(LSPIV_EINVAL, "too many windows for one launch (limit 2^31)");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_predict_deform(d_u, d_v, (uint32_t)n_pairs, (int)n_rows, (int)n_cols, d_nodes, s); });
}

int lspiv_piv_deform_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                                  float signal_threshold, int64_t pair_offset, const int32_t* d_nodes, float* d_out, float* d_corr_planes,
                                  void* stream) {
  LSPIV_TRY(check_dev_call(d_frames, d_out, pair_offset));
  if (!d_nodes) return fail(LSPIV_EINVAL, "d_nodes is NULL");
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  LSPIV_TRY(check_deform(wy, wx, oy, ox, H, W));
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  std::lock_guard<std::mutex> chain_lock(locks_here().multipass);
  LSPIV_TRY(deform_pass(c, d_frames, dtype, T, H, W, wy, oy, signal_threshold, d_nodes, d_out, d_corr_planes, s));
  const int64_t n_tiles = (T - 1) * g.n_rows * g.n_cols;
  return apply_v_sign(d_out + n_tiles, n_tiles, s);
}

int lspiv_piv_multipass_deform_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes,
                                      int n_deform, float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes,
                                      int16_t* d_shift_out, void* stream) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  return multipass_dev(c, d_frames, dtype, T, H, W, n_passes, passes, signal_threshold, pair_offset, d_out, d_corr_planes, d_shift_out,
                       on_stream(c, stream), n_deform);
}

// ---- the host-pointer entry points -----------------------------------------------------------------------------------------------
// What both check before they touch the device, the sizes they share, and the workspaces the frames and the planes go through: the
// stack is copied into c->d_frames through a two-slot pinned ring in batches of whole frames.  The caller holds the `host` lock.
struct HostStack {
  DeviceCtx* c;
  Grid g;
  int dev_dtype;   // float64 is narrowed to float32 while it is staged
  size_t frame_elems, frame_bytes, n_win, n_tiles;
  int64_t frames_per_batch;
  bool src_pinned;
};
static int host_stack(HostStack* h, const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                      int64_t pair_offset, const float* u, const float* v, const float* corr_max, const float* s2n, const float* corr_planes) {
  if (!frames || !u || !v || !corr_max || !s2n) return fail(LSPIV_EINVAL, "NULL buffer");
  if (pair_offset < 0) return fail(LSPIV_EINVAL, "pair_offset %lld is negative", (long long)pair_offset);
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &h->g));
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  LSPIV_TRY(get_ctx(&h->c));
  h->dev_dtype = dtype == LSPIV_F64 ? LSPIV_F32 : dtype;
  h->frame_elems = (size_t)H * W;
  h->frame_bytes = h->frame_elems * elem_size(h->dev_dtype);
  h->n_win = (size_t)h->g.n_rows * h->g.n_cols;
  h->n_tiles = (size_t)(T - 1) * h->n_win;
  LSPIV_TRY(ensure(&h->c->d_frames, &h->c->frames_cap, (size_t)T * h->frame_bytes));
  if (corr_planes) LSPIV_TRY(ensure(&h->c->d_planes, &h->c->planes_cap, h->n_tiles * wy * wx * sizeof(float)));
  LSPIV_TRY(stage_ring(h->c, h->frame_bytes));
  h->frames_per_batch = std::max<int64_t>(1, (int64_t)(h->c->pinned_cap / h->frame_bytes));
  h->src_pinned = dtype != LSPIV_F64 && is_pinned(frames);
  return LSPIV_OK;
}
// queues what a host entry point hands back on the context's stream: the four blocks of c->d_out, the planes (plane_elems floats per
// window), the chain's offsets
static int results_to_host(const HostStack& h, float* u, float* v, float* corr_max, float* s2n, float* corr_planes, size_t plane_elems,
                           int16_t* shift_out = nullptr, const int16_t* d_shift = nullptr) {
  DeviceCtx* c = h.c;
  float* const out[4] = {u, v, corr_max, s2n};
  for (int k = 0; k < 4; ++k)
    HIP_TRY(hipMemcpyAsync(out[k], c->d_out + k * h.n_tiles, h.n_tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (corr_planes) HIP_TRY(hipMemcpyAsync(corr_planes, c->d_planes, h.n_tiles * plane_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (shift_out) HIP_TRY(hipMemcpyAsync(shift_out, d_shift, h.n_tiles * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  return LSPIV_OK;
}

// the chain on a host stack: the whole chunk is staged first (the later passes need every frame of a pair anyway), then the chain runs on it
static int multipass_host(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes, int n_deform,
                          float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n, float* corr_planes,
                          int16_t* shift_out) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!passes) return fail(LSPIV_EINVAL, "NULL buffer");
  if (n_passes < 1 || n_passes > 8) return fail(LSPIV_EINVAL, "n_passes %d not in 1..8", n_passes);
  const int* last = passes + 4 * (n_passes - 1);
  HostStack h;
  LSPIV_TRY(host_stack(&h, frames, dtype, T, H, W, last[0], last[1], last[2], last[3], pair_offset, u, v, corr_max, s2n, corr_planes));
  DeviceCtx* c = h.c;
  const size_t out_bytes = (4 * h.n_tiles * sizeof(float) + 255) & ~(size_t)255;   // (the offsets follow the results, 256-byte aligned)
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, out_bytes + (shift_out ? h.n_tiles * 2 * sizeof(int16_t) : 0)));
  int16_t* d_shift = shift_out ? reinterpret_cast<int16_t*>((char*)c->d_out + out_bytes) : nullptr;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int batch = 0;
  for (int64_t f0 = 0; f0 < T; ++batch) {
    const int64_t f1 = std::min<int64_t>(T, f0 + h.frames_per_batch);
    LSPIV_TRY(stage_frames(c, batch, c->d_frames, frames, dtype, h.src_pinned, h.frame_elems, f0, f1, signal_threshold));
    f0 = f1;
  }
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  const int rc = multipass_dev(c, c->d_frames, h.dev_dtype, T, H, W, n_passes, passes, signal_threshold, pair_offset, c->d_out,
                               corr_planes ? c->d_planes : nullptr, d_shift, c->stream, n_deform);
  if (rc != LSPIV_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  LSPIV_TRY(results_to_host(h, u, v, corr_max, s2n, corr_planes, (size_t)last[0] * last[1], shift_out, d_shift));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_piv_multipass_deform_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes, int n_deform,
                                  float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n,
                                  float* corr_planes, int16_t* shift_out) {
  return multipass_host(frames, dtype, T, H, W, n_passes, passes, n_deform, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes, shift_out);
}

int lspiv_piv_multipass_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int n_passes, const int* passes, float signal_threshold,
                           int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n, float* corr_planes, int16_t* shift_out) {
  return multipass_host(frames, dtype, T, H, W, n_passes, passes, 0, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes, shift_out);
}

// a lagged pass on a host stack: the T frames are staged first (a pair needs frames up to 16 on), the tables go up next to the results,
// the pass runs, results, lags and clamped offsets come back
int lspiv_piv_lag_pairs_at(const void* frames, int dtype, int64_t T, int64_t n_pairs, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                           float signal_threshold, int64_t pair_offset, int lag_form, int k, int target128, const uint8_t* lag, const int16_t* shift,
                           float* u, float* v, float* corr_max, float* s2n, float* corr_planes, uint8_t* lag_out, int16_t* shift_out) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!lag_out) return fail(LSPIV_EINVAL, "NULL buffer");
  LSPIV_TRY(check_lag(wy, wx, H, W, T, n_pairs, lag_form, k, target128, lag, shift));
  HostStack h;
  LSPIV_TRY(host_stack(&h, frames, dtype, T, H, W, wy, wx, oy, ox, pair_offset, u, v, corr_max, s2n, corr_planes));
  h.n_tiles = (size_t)n_pairs * h.n_win;   // (the workspaces above are sized for T - 1 pairs: never smaller)
  DeviceCtx* c = h.c;
  // behind the four result blocks, each 256-byte aligned: the lags handed out, the lags handed in, the offsets (in and out share one block)
  const size_t out_bytes = (4 * h.n_tiles * sizeof(float) + 255) & ~(size_t)255;
  const size_t lag_bytes = (h.n_tiles + 255) & ~(size_t)255;
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, out_bytes + 2 * lag_bytes + h.n_tiles * 2 * sizeof(int16_t)));
  uint8_t* d_lag_out = reinterpret_cast<uint8_t*>((char*)c->d_out + out_bytes);
  uint8_t* d_lag_in = d_lag_out + lag_bytes;
  int16_t* d_shift = reinterpret_cast<int16_t*>(d_lag_in + lag_bytes);
  HIP_TRY(hipStreamSynchronize(c->stream));
  int batch = 0;
  for (int64_t f0 = 0; f0 < T; ++batch) {
    const int64_t f1 = std::min<int64_t>(T, f0 + h.frames_per_batch);
    LSPIV_TRY(stage_frames(c, batch, c->d_frames, frames, dtype, h.src_pinned, h.frame_elems, f0, f1, signal_threshold));
    f0 = f1;
  }
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  const bool lag_up = lag_form == LSPIV_LAG_WINDOW || lag_form == LSPIV_LAG_TABLE;
  if (lag_up) HIP_TRY(hipMemcpyAsync(d_lag_in, lag, lag_form == LSPIV_LAG_WINDOW ? h.n_win : h.n_tiles, hipMemcpyHostToDevice, c->stream));
  if (shift) HIP_TRY(hipMemcpyAsync(d_shift, shift, h.n_tiles * 2 * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
  int rc;
  {
    std::lock_guard<std::mutex> chain_lock(locks_here().multipass);
    rc = lag_pass(c, c->d_frames, h.dev_dtype, T, n_pairs, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, lag_form, k, target128,
                  lag_up ? d_lag_in : nullptr, shift ? d_shift : nullptr, c->d_out, corr_planes ? c->d_planes : nullptr, d_lag_out, d_shift, c->stream);
  }
  if (rc != LSPIV_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  LSPIV_TRY(results_to_host(h, u, v, corr_max, s2n, corr_planes, (size_t)wy * wx, shift_out, d_shift));
  HIP_TRY(hipMemcpyAsync(lag_out, d_lag_out, h.n_tiles, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_lag_predict(const float* u, const float* v, int64_t n_pairs, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox, int k_max,
                      int target128, uint8_t* lag, int16_t* shift) {
  if (!u || !v || !lag || !shift) return fail(LSPIV_EINVAL, "NULL buffer");
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  if (n_pairs < 0 || n_pairs > T - 1) return fail(LSPIV_ESHAPE, "n_pairs %lld not in 0 .. T - 1 = %lld", (long long)n_pairs, (long long)(T - 1));
  const size_t n = (size_t)n_pairs * g.n_rows * g.n_cols;
  if (n == 0) return LSPIV_OK;
  const size_t fb = (n * sizeof(float) + 255) & ~(size_t)255, lb = (n + 255) & ~(size_t)255;
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, 2 * fb + lb + n * 2 * sizeof(int16_t)));
  float* d_u = c->d_out;
  float* d_v = reinterpret_cast<float*>((char*)c->d_out + fb);
  uint8_t* d_lag = reinterpret_cast<uint8_t*>((char*)c->d_out + 2 * fb);
  int16_t* d_shift = reinterpret_cast<int16_t*>(d_lag + lb);
  HIP_TRY(hipMemcpyAsync(d_u, u, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_v, v, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  const int rc = lspiv_lag_predict_dev(d_u, d_v, n_pairs, T, H, W, wy, wx, oy, ox, k_max, target128, d_lag, d_shift, c->stream);
  if (rc != LSPIV_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  HIP_TRY(hipMemcpyAsync(lag, d_lag, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(shift, d_shift, n * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_piv_pairs_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy,
                        int ox, float signal_threshold, float* d_out, float* d_corr_planes, void* stream) {
  return lspiv_piv_pairs_dev_at(d_frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, 0, d_out, d_corr_planes, stream);
}

// the per-pair modes on a host stack, optionally with the px -> m/s scaling of pyorc/velocimetry/ffpiv.py:418-419 applied on the device
// before the results come back (dt != NULL: seconds per pair, T - 1 entries)
// Pipelined upload: the kernel for the pairs that have become resident runs while the next batch is staged and DMA'd.  Launches are cut
// at the anchors of the walking kernels' segments (multiples of lspiv_chunk_alignment of the absolute pair index), so the pipelined run
// issues exactly the jobs of one launch over the whole stack: same bits as lspiv_piv_pairs_dev_at.
static int piv_pairs_host(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                          float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n,
                          float* corr_planes, const PairMode& m, const double* dt = nullptr, double res_x = 1.0, double res_y = 1.0) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  HostStack h;
  LSPIV_TRY(host_stack(&h, frames, dtype, T, H, W, wy, wx, oy, ox, pair_offset, u, v, corr_max, s2n, corr_planes));
  DeviceCtx* c = h.c;
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, 4 * h.n_tiles * sizeof(float)));
  lspiv::PivParams base;
  LSPIV_TRY(fill_params(&base, c->d_frames, h.dev_dtype, T, H, W, wy, wx, oy, ox, signal_threshold, h.g));
  if (m.nw) set_search_window(&base, m.nw);
  if (m.mask) {   // the image mask goes up once, into the context's own buffer (under the host lock, like the frames' workspace), ahead of the kernels
    LSPIV_TRY(ensure(&c->d_mask, &c->mask_cap, h.frame_elems));
    HIP_TRY(hipMemcpyAsync(c->d_mask, m.mask, h.frame_elems, hipMemcpyHostToDevice, c->stream));
    base.mask = c->d_mask;
    base.k_min = (uint32_t)m.k_min;
  }
  if (m.peak2) {   // the second-peak block of the whole stack in the context's own buffer: every launch writes its windows' float4s
    LSPIV_TRY(ensure(&c->d_peak2, &c->peak2_cap, 4 * h.n_tiles * sizeof(float)));
    base.peak_excl = m.peak_excl;
    base.peak2_v_neg = g_opt_v_sign.load();
  }
  const int64_t align = m.per_pair() ? 1 : std::max(1, chunk_alignment_for(wy, wx, (int64_t)h.n_win));
  // "stack" signal mode scores a window position over ALL frames of the chunk: one launch once everything is resident
  const bool whole_chunk_only = g_opt_signal_mode.load() == 1 && signal_threshold >= 0.0f;
  int64_t launched = 0;   // pairs [0, launched) have been issued
  TraceSpan span;
  trace_begin(&span, LSPIV_TRACE_PIV_HOST, c->stream);
  int batch = 0;
  for (int64_t f0 = 0; f0 < T; ++batch) {
    const int64_t f1 = std::min<int64_t>(T, f0 + h.frames_per_batch);
    LSPIV_TRY(stage_frames(c, batch, c->d_frames, frames, dtype, h.src_pinned, h.frame_elems, f0, f1, signal_threshold));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->staged[batch & 1], 0));
    // pairs whose two frames are resident: [0, f1 - 1); issue up to the last anchor below that (everything at the end)
    int64_t p1 = f1 - 1;
    if (f1 < T) p1 = whole_chunk_only ? 0 : ((pair_offset + p1) / align) * align - pair_offset;
    const int64_t p0 = launched;
    if (p1 > p0) {
      lspiv::PivParams p = base;
      p.frames = (const char*)c->d_frames + (size_t)p0 * h.frame_bytes;
      p.pair_offset = pair_offset + p0;
      p.n_pairs = (uint32_t)(p1 - p0);
      p.n_tiles = (uint32_t)((p1 - p0) * h.n_win);
      set_results(&p, c->d_out, h.n_tiles, (size_t)p0 * h.n_win, corr_planes ? c->d_planes : nullptr, (size_t)wy * wx);
      if (m.peak2) p.peak2 = c->d_peak2 + 4 * (size_t)p0 * h.n_win;
      LSPIV_TRY(apply_signal_mode(c, &p, h.dev_dtype, c->stream));
      LSPIV_TRY(dispatch(p, h.dev_dtype, false, c->stream, m.filter));
      LSPIV_TRY(apply_v_sign(p.v, (int64_t)p.n_tiles, c->stream));
      launched = p1;
    }
    f0 = f1;
  }
  if (dt) {
    // u, v to metres per second where they are: (u * res / dt).astype(float32) -- float32 product, float64 division, one rounding
    // (masks.hip, scale_velocity_kernel: bit for bit what numpy computes for a python-float resolution, tests/test_masks.py)
    LSPIV_TRY(ensure(&c->d_scratch, &c->scratch_cap, (size_t)(T - 1) * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->d_scratch, dt, (size_t)(T - 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LSPIV_TRY(launch_status(lspiv::launch_scale_velocity(c->d_out, T - 1, (int64_t)h.n_win, (float)res_x, (float)res_y, (const double*)c->d_scratch, c->stream)));
  }
  LSPIV_TRY(results_to_host(h, u, v, corr_max, s2n, corr_planes, (size_t)wy * wx));
  if (m.peak2) HIP_TRY(hipMemcpyAsync(m.peak2, c->d_peak2, 4 * h.n_tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  trace_end(&span, c->stream);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_piv_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                       float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n,
                       float* corr_planes) {
  return piv_pairs_host(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes, {});
}

int lspiv_piv_spof_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                            float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n,
                            float* corr_planes) {
  LSPIV_TRY(check_spof(wy, wx));
  return piv_pairs_host(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes,
                        {.filter = LSPIV_FILTER_SPOF});
}

int lspiv_piv_masked_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                              const uint8_t* mask, int64_t k_min, float signal_threshold, int64_t pair_offset, float* u, float* v,
                              float* corr_max, float* s2n, float* corr_planes) {
  LSPIV_TRY(check_masked(wy, wx, mask, k_min));
  return piv_pairs_host(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes,
                        {.mask = mask, .k_min = k_min});
}

int lspiv_piv_peak2_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                             float signal_threshold, int64_t pair_offset, int peak_exclusion, float* u, float* v, float* corr_max, float* s2n,
                             float* peak2, float* corr_planes) {
  LSPIV_TRY(check_peak2(wy, wx, peak_exclusion, peak2, false));
  return piv_pairs_host(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes,
                        {.peak2 = peak2, .peak_excl = peak_exclusion});
}

int lspiv_piv_search_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int say, int sax, int wy, int wx, int oy,
                              int ox, float signal_threshold, int64_t pair_offset, float* u, float* v, float* corr_max, float* s2n,
                              float* corr_planes) {
  LSPIV_TRY(check_search(say, sax, wy, wx));
  return piv_pairs_host(frames, dtype, T, H, W, say, sax, oy, ox, signal_threshold, pair_offset, u, v, corr_max, s2n, corr_planes, {.nw = wy});
}

int lspiv_piv_velocity_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                          float signal_threshold, int64_t pair_offset, double res_x, double res_y, const double* dt, float* v_x, float* v_y,
                          float* corr_max, float* s2n) {
  if (!dt) return fail(LSPIV_EINVAL, "dt is NULL");
  return piv_pairs_host(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, pair_offset, v_x, v_y, corr_max, s2n, nullptr, {}, dt, res_x, res_y);
}

int lspiv_piv_pairs(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                    float signal_threshold, float* u, float* v, float* corr_max, float* s2n, float* corr_planes) {
  return lspiv_piv_pairs_at(frames, dtype, T, H, W, wy, wx, oy, ox, signal_threshold, 0, u, v, corr_max, s2n, corr_planes);
}

int lspiv_u_v_displacement(const float* corr_planes, int64_t P, int64_t n_win, int wy, int wx, float* u, float* v) {
  if (!corr_planes || !u || !v) return fail(LSPIV_EINVAL, "NULL buffer");
  if (P < 0 || n_win < 0 || wy < 1 || wx < 1 || wy > 4096 || wx > 4096) return fail(LSPIV_EINVAL, "bad shape");
  const int64_t n = P * n_win;
  if (n == 0) return LSPIV_OK;
  if (n >= (int64_t)1 << 31) return fail(LSPIV_EINVAL, "too many planes for one launch");
  uint32_t n_refit = 0;   // planes re-fitted: a device counter that comes back with the results
  HostCall hc({{corr_planes, (size_t)n * wy * wx * sizeof(float)}}, {{u, n * sizeof(float)}, {v, n * sizeof(float)}, {&n_refit, sizeof(uint32_t)}});
  // no frames behind these planes, so no rescue pass: the windows its criterion flags (no plane noise here: the allowance of the fused
  // kernels, not doubled) get the float64 fit of their five samples instead (piv_peaks.h); "rescue" = 0 keeps the float32 fits
  const float refit_k = g_opt_rescue.load() ? (float)(2.0 * g_opt_rescue_kappa.load() * 1e-9 / (0.6931471805599453 * 1e-4)) : 0.0f;
  if (hc.upload() && hc.ran(launch_status(hipMemsetAsync(hc.out(2), 0, sizeof(uint32_t), hc.stream()), "hipMemsetAsync failed")) &&
      hc.ran(launch_status(lspiv::launch_peaks_from_planes(hc.in<float>(0), (uint32_t)n, wy, wx, g_opt_border.load(), hc.out<float>(0), hc.out<float>(1),
                                                           refit_k, hc.out<uint32_t>(2), hc.stream()))))
    hc.ran(apply_v_sign(hc.out<float>(1), n, hc.stream()));
  const int rc = hc.finish(__func__);   // waits for the stream on every exit: u, v and n_refit are the caller's and this frame's
  if (rc == LSPIV_OK) g_peaks_refitted.store((int)std::min<uint32_t>(n_refit, 0x7fffffffu));
  return rc;
}

int lspiv_second_peak(const float* corr_planes, int64_t P, int64_t n_win, int wy, int wx, int peak_exclusion, float* peak2) {
  if (P < 0 || n_win < 0 || (n_win > 0 && P > (((int64_t)1 << 31) - 1) / n_win)) return fail(LSPIV_EINVAL, "bad shape");
  const int64_t n = P * n_win;
  LSPIV_TRY(check_second_peak(corr_planes, peak2, n, wy, wx, peak_exclusion));
  if (n == 0) return LSPIV_OK;
  const size_t pb = (size_t)n * wy * wx * sizeof(float);
  return host_roundtrip(__func__, {corr_planes, pb}, {peak2, 4 * (size_t)n * sizeof(float)}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_second_peak_dev((const float*)d_in, n, wy, wx, peak_exclusion, (float*)d_out, s);
  });
}

}  // extern "C"
