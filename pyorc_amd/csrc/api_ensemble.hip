// C ABI of liblspiv_hip.so, ensemble correlation (api_core.hip has the overview): the summed correlation planes of a video, their
// fit, and the float64 rescue of that fit in stages (piv_rescue.hip, ens_*).
#include "api_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace lspiv_api;

struct lspiv_ensemble {
  int64_t H, W;
  int wy, wx, oy, ox;
  Grid g;
  int device;
  float* d_sum;    // n_win * wy * wx
  float* d_count;  // n_win
  float* d_part;   // walking kernels: per-segment partial sums + counts (grow-only workspace)
  size_t part_cap;
  int64_t pairs_done;   // pairs accumulated so far = absolute index of the next chunk's first pair (segment anchoring)
  // float64 rescue of the final fit (piv_rescue.hip, ens_*): the chunks' frames and masked corr_max stay reachable until
  // lspiv_ensemble_finish -- owned copies (host entry point: the upload buffer itself; "_dev": a device copy, LSPIV_RETAIN_COPY)
  // or the caller's pointer (LSPIV_RETAIN_BORROW)
  struct Kept { void* d_frames; bool owned; int dtype; int64_t T; float* d_cmax; };
  std::vector<Kept> kept;
  int retain_mode;          // "_dev" entry point: LSPIV_RETAIN_*; the host entry point always keeps its upload buffers
  size_t kept_bytes;        // HBM held BECAUSE of this handle: owned frame copies, the corr_max records, and the borrowed chunks too
                            // (they are the caller's allocations, but it keeps them alive for the handle): all against the budget
  // the chunks' masked corr_max records live in a few large blocks (geometric growth) instead of one hipMalloc per accumulate
  struct CmaxBlock { char* base; size_t cap, used; };
  std::vector<CmaxBlock> cmax_blocks;
  // accumulate_dev may run on caller streams while flag / partials / finish run on the context's stream: one event per stream
  // that accumulated, recorded after each accumulate, waited for by every reader of the sums and of the kept records
  struct AccEvent { hipStream_t stream; hipEvent_t ev; };
  std::vector<AccEvent> acc_events;
  bool retain_complete;     // false: some chunk could not be kept (budget, mode NONE, imported state) -> no rescue from frames (ensemble_refit_planes)
  void* d_rescue; size_t rescue_cap;     // EnsRescueHdr (256 B) + records
  double* d_partial; size_t partial_cap;
  double* d_totals; size_t totals_cap;   // (n_rec, kEnsMaxCand * 5): the partial sums merged over this handle's pair-blocks
  int64_t last_flagged, last_rescued, last_skipped;
  bool foreign;             // the sums were replaced by lspiv_ensemble_import: they hold other handles' pairs as well
  uint32_t n_rec;           // records of the last lspiv_ensemble_flag (sorted by window), 0 if none
  uint64_t rec_digest;      // FNV-1a over (w, ncand, pos[0 .. ncand-1]) of those records: what ranks compare before they sum partials
  float flag_min_count;     // count_min * n_frames of that call
  // sliding ensemble (lspiv_ensemble_set_sliding): outputs over windows of sl_window pairs advancing by sl_stride pairs.  The block
  // store keeps one slot per (block of sl_stride pairs, window) for the whole run, in the layout the accumulating kernel writes:
  // block b's plane sums at d_store + b * n_win * wy * wx, its counts at d_store_cnt + b * n_win; d_sum / d_count stay untouched
  int64_t sl_window, sl_stride;   // 0: not a sliding handle
  float* d_store; float* d_store_cnt;
  size_t store_blocks;      // capacity, in blocks
  bool tail_open;           // the last accumulate ended inside a block: it was the last one
  // multi-pass ensemble (lspiv_ensemble_set_shift): a SHIFTED handle -- frame t+1's window of every pair sits at
  // the window's own offset.  d_shift: n_win x {dy, dx}, already clamped (launch_clamp_shift: window_shift's clamp is idempotent);
  // shift_host: the same values, for lspiv_ensemble_get_shift and the comparison in lspiv_ensemble_allreduce.  nullptr: the plain ensemble
  int16_t* d_shift;
  std::vector<int16_t> shift_host;
  // SPOF phase-filtered ensemble (lspiv_ensemble_set_spectral_filter): LSPIV_FILTER_SPOF -- every pair's plane
  // comes from the filtered one-owner kernel (piv_spof_impl.h); no float64 rescue of the final fit, nothing retained for it.  0: none
  int filter;
  int sl_layout;            // slot layout of the store, recorded by the first accumulate: 0 nothing written yet, 1 fft-shifted row-major, 2 lane-major (64 x 64 walking kernel)
};

// HBM the retained chunks of one ensemble may occupy: LSPIV_ENSEMBLE_RETAIN_BYTES, default a quarter of the device
static size_t ensemble_retain_budget() {
  if (const char* e = getenv("LSPIV_ENSEMBLE_RETAIN_BYTES")) return (size_t)atoll(e);
  size_t f = 0, t = 0;
  if (hipMemGetInfo(&f, &t) != hipSuccess) { (void)hipGetLastError(); return (size_t)16 << 30; }
  return t / 4;
}
static void ensemble_drop_kept(lspiv_ensemble* h) {
  for (auto& k : h->kept)
    if (k.owned && k.d_frames) (void)hipFree(k.d_frames);
  for (auto& b : h->cmax_blocks) (void)hipFree(b.base);
  h->kept.clear();
  h->cmax_blocks.clear();
  h->kept_bytes = 0;
}
// n bytes (256-byte granules) from the handle's record blocks; a new block is twice the last one (>= 1 MiB, >= n, <= 1 GiB unless n
// is larger): a handle that takes hundreds of chunks calls hipMalloc a dozen times, not hundreds
static void* ensemble_cmax_alloc(lspiv_ensemble* h, size_t n) {
  n = (n + 255) & ~(size_t)255;
  if (!h->cmax_blocks.empty()) {
    auto& b = h->cmax_blocks.back();
    if (b.used + n <= b.cap) { void* p = b.base + b.used; b.used += n; return p; }
  }
  const size_t last = h->cmax_blocks.empty() ? 0 : h->cmax_blocks.back().cap;
  const size_t cap = std::max(n, std::min<size_t>(std::max<size_t>(2 * last, (size_t)1 << 20), (size_t)1 << 30));
  void* base = nullptr;
  if (hipMalloc(&base, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  h->cmax_blocks.push_back({(char*)base, cap, n});
  h->kept_bytes += cap;
  return base;
}
// the handle stops being rescuable: what it kept is of no use any more (the float32 fits stay, lspiv_ensemble_stats says so)
static void ensemble_give_up_retention(lspiv_ensemble* h) {
  h->retain_complete = false;
  ensemble_drop_kept(h);
}
// keep the masked corr_max of a chunk (the kernels' keep decisions) next to its frames (`frame_bytes` of them: counted against
// the budget whether the handle owns them or borrows them); on any failure -- budget, allocation, copy -- the ensemble simply stops
// being rescuable, the accumulation itself is not affected.  Takes ownership of an `owned` buffer either way.
static void ensemble_keep(lspiv_ensemble* h, void* d_frames, bool owned, size_t frame_bytes, int dtype, int64_t T, const float* d_cmax,
                          hipStream_t s) {
  const size_t n_tiles = (size_t)(T - 1) * h->g.n_rows * h->g.n_cols;
  void* cm = nullptr;
  if (h->kept_bytes + frame_bytes + n_tiles * sizeof(float) > ensemble_retain_budget() ||
      !(cm = ensemble_cmax_alloc(h, n_tiles * sizeof(float))) ||
      hipMemcpyAsync(cm, d_cmax, n_tiles * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    (void)hipGetLastError();
    if (owned) (void)hipFree(d_frames);
    ensemble_give_up_retention(h);
    return;
  }
  h->kept.push_back({d_frames, owned, dtype, T, (float*)cm});
  h->kept_bytes += frame_bytes;
}
// accumulate_dev ran on stream `s`: note where that stream stands; readers on another stream wait for it
static void ensemble_mark_accumulated(lspiv_ensemble* h, hipStream_t s) {
  lspiv_ensemble::AccEvent* a = nullptr;
  for (auto& e : h->acc_events) if (e.stream == s) a = &e;
  if (!a) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); return; }
    h->acc_events.push_back({s, ev});
    a = &h->acc_events.back();
  }
  if (hipEventRecord(a->ev, s) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); }
}
static void ensemble_wait_accumulated(lspiv_ensemble* h, hipStream_t reader) {
  for (auto& e : h->acc_events)
    if (e.stream != reader && hipStreamWaitEvent(reader, e.ev, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(e.stream); }
}

// ---- lspiv_ensemble_allreduce: corr_sum / corr_count of several handles summed on the first handle's device ----------------------
constexpr int kAllreduceMax = 64;
struct AllreduceSrc { const float* p[kAllreduceMax]; };
// out[i] = ((src0[i] + src1[i]) + src2[i]) + ...: adds only, one rounding each, in handle order (numpy's float32 sum in that order)
__global__ __launch_bounds__(256) void ensemble_allreduce_kernel(AllreduceSrc src, int n, int64_t count, float* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    float acc = src.p[0][i];
    for (int k = 1; k < n; ++k) acc = __fadd_rn(acc, src.p[k][i]);
    out[i] = acc;
  }
}
static int launch_allreduce(const AllreduceSrc& src, int n, int64_t count, float* out, hipStream_t s) {
  if (count <= 0) return LSPIV_OK;
  const int64_t blocks = std::min<int64_t>((count + 255) / 256, 65536);
  hipLaunchKernelGGL(ensemble_allreduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, n, count, out);
  return launch_status(hipGetLastError(), "allreduce kernel launch failed");
}
// peer access from `dev` to `peer`, enabled once per ordered pair for the process (the caller has `dev` current)
static bool peer_reachable(int dev, int peer) {
  static std::mutex mu;
  static signed char state[kMaxDevices][kMaxDevices];   // 0 unknown, 1 enabled, -1 not possible
  if (dev == peer) return true;
  if (dev < 0 || peer < 0 || dev >= kMaxDevices || peer >= kMaxDevices) return false;
  std::lock_guard<std::mutex> lk(mu);
  if (state[dev][peer] == 0) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dev, peer) != hipSuccess) { (void)hipGetLastError(); can = 0; }
    if (can) {
      const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
      (void)hipGetLastError();
    }
    state[dev][peer] = can ? 1 : -1;
  }
  return state[dev][peer] == 1;
}
// the state sum itself, with the devices' host locks held and handles[0]'s device current
static int ensemble_allreduce_locked(lspiv_ensemble** handles, int n) {
  lspiv_ensemble* root = handles[0];
  const int rd = root->device;
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t n_win = (size_t)root->g.n_rows * root->g.n_cols, np = n_win * root->wy * root->wx;
  // every handle's accumulations have been issued on its device's streams: the root's stream waits for the local ones, the host for
  // the remote ones (an event of another device is not waited for by a stream)
  for (int k = 0; k < n; ++k) {
    if (handles[k]->device == rd) ensemble_wait_accumulated(handles[k], c->stream);
    else for (auto& e : handles[k]->acc_events) HIP_TRY(hipEventSynchronize(e.ev));
  }
  AllreduceSrc ss{}, sc{};
  std::vector<void*> staging;
  int rc = LSPIV_OK;
  for (int k = 0; k < n && rc == LSPIV_OK; ++k) {
    lspiv_ensemble* h = handles[k];
    if (h->device == rd || peer_reachable(rd, h->device)) { ss.p[k] = h->d_sum; sc.p[k] = h->d_count; continue; }
    void* p = nullptr;
    if (hipMalloc(&p, (np + n_win) * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); rc = fail(LSPIV_ENOMEM, "hipMalloc allreduce staging"); break; }
    staging.push_back(p);
    float* f = (float*)p;
    if (hipMemcpyPeerAsync(f, rd, h->d_sum, h->device, np * sizeof(float), c->stream) != hipSuccess ||
        hipMemcpyPeerAsync(f + np, rd, h->d_count, h->device, n_win * sizeof(float), c->stream) != hipSuccess) {
      rc = fail(LSPIV_EHIP, "hipMemcpyPeerAsync: %s", hipGetErrorString(hipGetLastError()));
      break;
    }
    ss.p[k] = f; sc.p[k] = f + np;
  }
  // in place on the root handle: element i is read from every source before it is written, by the same thread
  if (rc == LSPIV_OK) rc = launch_allreduce(ss, n, (int64_t)np, root->d_sum, c->stream);
  if (rc == LSPIV_OK) rc = launch_allreduce(sc, n, (int64_t)n_win, root->d_count, c->stream);
  for (int k = 1; k < n && rc == LSPIV_OK; ++k) {
    lspiv_ensemble* h = handles[k];
    if (h == root) continue;
    hipError_t e1, e2;
    if (h->device == rd) {
      e1 = hipMemcpyAsync(h->d_sum, root->d_sum, np * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
      e2 = hipMemcpyAsync(h->d_count, root->d_count, n_win * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    } else {
      e1 = hipMemcpyPeerAsync(h->d_sum, h->device, root->d_sum, rd, np * sizeof(float), c->stream);
      e2 = hipMemcpyPeerAsync(h->d_count, h->device, root->d_count, rd, n_win * sizeof(float), c->stream);
    }
    if (e1 != hipSuccess || e2 != hipSuccess) rc = fail(LSPIV_EHIP, "allreduce copy back: %s", hipGetErrorString(hipGetLastError()));
  }
  const hipError_t se = hipStreamSynchronize(c->stream);   // also before the staging buffers go
  for (void* p : staging) (void)hipFree(p);
  if (rc == LSPIV_OK && se != hipSuccess) rc = fail(LSPIV_EHIP, "allreduce: %s", hipGetErrorString(se));
  return rc;
}

// ---- sliding ensemble: the block store --------------------------------------------------------------------------------------
// room for `blocks` blocks (geometric growth; the blocks written so far move along).  `s`: the stream the caller launches on next.
static int sliding_reserve(lspiv_ensemble* h, size_t blocks, hipStream_t s) {
  if (blocks <= h->store_blocks) return LSPIV_OK;
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols, plane = (size_t)h->wy * h->wx;
  const size_t used = (size_t)(h->pairs_done / h->sl_stride);
  void *ps = nullptr, *pc = nullptr;
  size_t cap = std::max(blocks, 2 * h->store_blocks);
  for (;;) {
    if (hipMalloc(&ps, cap * n_win * plane * sizeof(float)) == hipSuccess) {
      if (hipMalloc(&pc, cap * n_win * sizeof(float)) == hipSuccess) break;
      (void)hipFree(ps);
    }
    (void)hipGetLastError();
    ps = pc = nullptr;
    if (cap == blocks)
      return fail(LSPIV_ENOMEM, "sliding ensemble: the block store needs %zu bytes for %zu blocks of %lld pairs", blocks * n_win * (plane + 1) * sizeof(float),
                  blocks, (long long)h->sl_stride);
    cap = blocks;   // the doubled store did not fit: what this call needs
  }
  if (used) {
    ensemble_wait_accumulated(h, s);   // earlier accumulate_dev calls may have written the store on other streams
    hipError_t e = hipMemcpyAsync(ps, h->d_store, used * n_win * plane * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pc, h->d_store_cnt, used * n_win * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(ps); (void)hipFree(pc); return fail(LSPIV_EHIP, "sliding ensemble: moving the block store: %s", hipGetErrorString(e)); }
  }
  if (h->d_store) (void)hipFree(h->d_store);
  if (h->d_store_cnt) (void)hipFree(h->d_store_cnt);
  h->d_store = (float*)ps; h->d_store_cnt = (float*)pc; h->store_blocks = cap;
  return LSPIV_OK;
}
static int not_on_sliding(const lspiv_ensemble* h, const char* call) {
  if (h && h->sl_stride) return fail(LSPIV_EINVAL, "%s: this is a sliding ensemble handle (lspiv_ensemble_set_sliding); its results come from lspiv_ensemble_sliding_finish", call);
  return LSPIV_OK;
}

extern "C" {

// ---- ensemble -------------------------------------------------------------------------------
int lspiv_ensemble_begin(int64_t H, int64_t W, int wy, int wx, int oy, int ox, lspiv_ensemble** handle) {
  if (!handle) return fail(LSPIV_EINVAL, "handle is NULL");
  Grid g;
  LSPIV_TRY(make_grid(H, W, wy, wx, oy, ox, &g));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  lspiv_ensemble* h = new lspiv_ensemble();
  h->H = H; h->W = W; h->wy = wy; h->wx = wx; h->oy = oy; h->ox = ox; h->g = g;
  h->retain_mode = LSPIV_RETAIN_NONE; h->retain_complete = true;   // (the rest value-initialised: zeros, nullptr)
  HIP_TRY(hipGetDevice(&h->device));
  const size_t n_win = (size_t)g.n_rows * g.n_cols;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, n_win * wy * wx * sizeof(float));
  if (e != hipSuccess) { delete h; return fail(LSPIV_ENOMEM, "hipMalloc corr_sum: %s", hipGetErrorString(e)); }
  h->d_sum = (float*)p;
  e = hipMalloc(&p, n_win * sizeof(float));
  if (e != hipSuccess) { hipFree(h->d_sum); delete h; return fail(LSPIV_ENOMEM, "hipMalloc corr_count: %s", hipGetErrorString(e)); }
  h->d_count = (float*)p;
  HIP_TRY(hipMemsetAsync(h->d_sum, 0, n_win * wy * wx * sizeof(float), c->stream));
  HIP_TRY(hipMemsetAsync(h->d_count, 0, n_win * sizeof(float), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // lspiv_ensemble_accumulate_dev may be given another stream
  *handle = h;
  return LSPIV_OK;
}

static int ensemble_launch(lspiv_ensemble* h, DeviceCtx* c, const void* d_frames, int dtype, int64_t T, float corr_min,
                           float s2n_min, float signal_threshold, float* d_cmax, float* d_s2n, hipStream_t s) {
  lspiv::PivParams p;
  LSPIV_TRY(fill_params(&p, d_frames, dtype, T, h->H, h->W, h->wy, h->wx, h->oy, h->ox, signal_threshold, h->g));
  p.cmax = d_cmax;
  p.s2n = d_s2n;
  p.corr_min = corr_min;
  p.s2n_min = s2n_min;
  p.corr_sum = h->d_sum;
  p.corr_count = h->d_count;
  const int kind = lspiv_kernel_kind(h->wy, h->wx);
  const int walk = lspiv::walk_setting();
  p.pair_offset = h->pairs_done;   // advanced only once the launch has been issued (a failed accumulate changes nothing)
  if (h->filter) {
    // filtered handle: the one-owner kernel on the filtered planes (piv_spof_impl.h, "filtered ensemble kernel"); no walking, no segments --
    // its sums are the same bits for every chunking
    LSPIV_TRY(check_spof(h->wy, h->wx));   // (signal_mode = 1, norm_clip = 0: refused here, where the per-pair entry points refuse them)
    LSPIV_TRY(dispatch(p, dtype, true, s, h->filter));
    h->pairs_done += p.n_pairs;
    return LSPIV_OK;
  }
  if (h->d_shift) {
    // shifted handle: the one-owner kernel on shifted windows (piv_fft_impl.h, "shifted ensemble kernel"); no walking, no segments --
    // its sums are the same bits for every chunking
    LSPIV_TRY(check_multipass_options());   // (signal_mode = 1, norm_clip = 0: refused here, where multi-pass PIV refuses them)
    p.shifted = 1;
    p.shift = h->d_shift;
    LSPIV_TRY(dispatch(p, dtype, true, s));
    h->pairs_done += p.n_pairs;
    return LSPIV_OK;
  }
  if (h->sl_stride) {
    // sliding ensemble: the sums of this call's blocks go into the block store, nothing into d_sum / d_count
    if (h->tail_open)
      return fail(LSPIV_EINVAL, "sliding ensemble: the previous accumulate call did not end on a multiple of %lld pairs, so it was the last one", (long long)h->sl_stride);
    const int64_t sp = h->sl_stride, blk0 = h->pairs_done / sp, nb = ((int64_t)p.n_pairs + sp - 1) / sp;   // (a trailing partial block gets a slot too; no output reads it)
    LSPIV_TRY(sliding_reserve(h, (size_t)(blk0 + nb), s));
    // the slot layout is the store's for the whole run: what the first call wrote is what lspiv_ensemble_sliding_finish decodes
    const bool walking = kind_walks(kind) && walk != 0;
    int lane_major = 0;
    if (walking) lspiv::walk_ensemble_slot_layout(h->wy, &lane_major);
    const int layout = lane_major ? 2 : 1;
    if (h->sl_layout && h->sl_layout != layout)
      return fail(LSPIV_EINVAL, "sliding ensemble: the 'walk' setting (LSPIV_WALK) changed between accumulate calls; the block store of a %d x %d window holds %s slots and this call would write %s ones",
                  h->wy, h->wx, h->sl_layout == 2 ? "lane-major" : "row-major", layout == 2 ? "lane-major" : "row-major");
    const size_t plane = (size_t)h->wy * h->wx;
    float* const slots = h->d_store + (size_t)blk0 * p.n_win * plane;
    float* const counts = h->d_store_cnt + (size_t)blk0 * p.n_win;
    LSPIV_TRY(apply_signal_mode(c, &p, dtype, s));   // "stack" mode: one set of keep flags per call, as in the plain ensemble
    if (walking) {
      // the walking kernel with segment = block and WITHOUT its merge (corr_sum = nullptr): every (block, window) job writes its
      // whole slot and its count, in the kernel's own slot layout (ensemble_sliding_mean_kernel decodes it)
      const lspiv::WalkSegments w = lspiv::walk_segments(p.n_pairs, p.pair_offset, (uint32_t)sp);
      p.seg_len = w.seg_len; p.seg_first = w.seg_first; p.n_seg = w.n_seg;
      p.part_sum = slots; p.part_cnt = counts;
      p.corr_sum = nullptr; p.corr_count = nullptr;
      LSPIV_TRY(dispatch(p, dtype, true, s));
    } else {
      // every other window family: the one-owner ensemble kernel once per block, adding into that block's zeroed row-major slot
      HIP_TRY(hipMemsetAsync(slots, 0, (size_t)nb * p.n_win * plane * sizeof(float), s));
      HIP_TRY(hipMemsetAsync(counts, 0, (size_t)nb * p.n_win * sizeof(float), s));
      const size_t frame_bytes = (size_t)h->H * h->W * elem_size(dtype);
      for (int64_t b = 0; b < nb; ++b) {
        lspiv::PivParams q = p;
        const int64_t first = b * sp;
        q.n_pairs = (uint32_t)std::min<int64_t>(sp, (int64_t)p.n_pairs - first);
        q.n_tiles = q.n_pairs * p.n_win;
        q.frames = (const char*)d_frames + (size_t)first * frame_bytes;
        q.cmax = d_cmax + (size_t)first * p.n_win;
        q.s2n = d_s2n + (size_t)first * p.n_win;
        q.pair_offset = p.pair_offset + first;
        q.corr_sum = slots + (size_t)b * p.n_win * plane;
        q.corr_count = counts + (size_t)b * p.n_win;
        LSPIV_TRY(dispatch(q, dtype, true, s));
      }
    }
    h->pairs_done += p.n_pairs;
    h->tail_open = (p.n_pairs % sp) != 0;
    h->sl_layout = layout;
    return LSPIV_OK;
  }
  if (kind_walks(kind) && walk != 0) {
    // segments anchored at multiples of the anchor length of the absolute pair index (common.h): the partial sums, and
    // the order they are merged in, are the same for every chunking whose boundaries are multiples of that length
    const lspiv::WalkSegments w = lspiv::walk_segments(p.n_pairs, p.pair_offset, walk > 1 ? (uint32_t)walk : lspiv::walk_anchor(h->wy, p.n_win));
    p.seg_len = w.seg_len; p.seg_first = w.seg_first; p.n_seg = w.n_seg;
    const size_t plane = (size_t)h->wy * h->wx;
    const size_t need = (size_t)p.n_seg * p.n_win * (plane + 1) * sizeof(float);
    LSPIV_TRY(ensure(&h->d_part, &h->part_cap, need));
    // not zeroed: every (segment, window) job writes its whole slot and its count (first iteration stores, later ones add)
    p.part_sum = h->d_part;
    p.part_cnt = h->d_part + (size_t)p.n_seg * p.n_win * plane;
  }
  LSPIV_TRY(apply_signal_mode(c, &p, dtype, s));
  LSPIV_TRY(dispatch(p, dtype, true, s));
  h->pairs_done += p.n_pairs;
  return LSPIV_OK;
}

int lspiv_ensemble_accumulate_dev(lspiv_ensemble* h, const void* d_frames, int dtype, int64_t T, float corr_min,
                                  float s2n_min, float signal_threshold, float* d_corr_s2n, void* stream) {
  if (!h || !d_frames || !d_corr_s2n) return fail(LSPIV_EINVAL, "NULL argument");
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t n_tiles = (size_t)(T - 1) * h->g.n_rows * h->g.n_cols;
  hipStream_t s = on_stream(c, stream);
  LSPIV_TRY(ensemble_launch(h, c, d_frames, dtype, T, corr_min, s2n_min, signal_threshold, d_corr_s2n, d_corr_s2n + n_tiles, s));
  // retention for the float64 rescue of the final fit (lspiv_ensemble_set_retain)
  const size_t fbytes = (size_t)T * h->H * h->W * elem_size(dtype);
  if (h->retain_mode == LSPIV_RETAIN_NONE || !h->retain_complete || !g_opt_rescue.load() || h->filter) {   // (a filtered handle has no rescue)
    if (h->retain_complete) ensemble_give_up_retention(h);
  } else if (h->retain_mode == LSPIV_RETAIN_BORROW) {
    ensemble_keep(h, const_cast<void*>(d_frames), false, fbytes, dtype, T, d_corr_s2n, s);
  } else {
    void* copy = nullptr;
    if (h->kept_bytes + fbytes > ensemble_retain_budget() || hipMalloc(&copy, fbytes) != hipSuccess) {
      (void)hipGetLastError();
      ensemble_give_up_retention(h);
    } else if (hipMemcpyAsync(copy, d_frames, fbytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      (void)hipGetLastError(); (void)hipFree(copy);
      ensemble_give_up_retention(h);
    } else {
      ensemble_keep(h, copy, true, fbytes, dtype, T, d_corr_s2n, s);
    }
  }
  ensemble_mark_accumulated(h, s);   // flag / partials / finish (context stream) wait for the sums, the records and the copies
  return LSPIV_OK;
}

int lspiv_ensemble_accumulate(lspiv_ensemble* h, const void* frames, int dtype, int64_t T, float corr_min,
                              float s2n_min, float signal_threshold, float* corr_max, float* s2n) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !frames || !corr_max || !s2n) return fail(LSPIV_EINVAL, "NULL argument");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < 2) return fail(LSPIV_ESHAPE, "need at least 2 frames, got %lld", (long long)T);
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols, n_tiles = (size_t)(T - 1) * n_win;
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, 2 * n_tiles * sizeof(float)));
  // Pipelined like lspiv_piv_pairs: the ensemble sums are additive over pairs, so the pairs of sub-batch k are
  // accumulated (in order, on one stream) while sub-batch k+1 is staged and DMA'd.  float64 is narrowed while staged.
  const int dev_dtype = dtype == LSPIV_F64 ? LSPIV_F32 : dtype;
  const size_t frame_elems = (size_t)h->H * h->W;
  const size_t frame_bytes = frame_elems * elem_size(dev_dtype);
  // the chunk is uploaded into a buffer of its own that stays with the handle until finish (float64 rescue of the final fit),
  // as long as the retained chunks fit their budget; beyond it, into the shared workspace as before (float32 fits stay)
  void* own = nullptr;
  if (g_opt_rescue.load() && !h->filter && h->retain_complete && h->kept_bytes + (size_t)T * frame_bytes <= ensemble_retain_budget()) {
    if (hipMalloc(&own, (size_t)T * frame_bytes) != hipSuccess) { (void)hipGetLastError(); own = nullptr; }
  }
  if (!own) {
    if (h->retain_complete) ensemble_give_up_retention(h);
    LSPIV_TRY(ensure(&c->d_frames, &c->frames_cap, (size_t)T * frame_bytes));
  }
  char* const d_chunk = own ? (char*)own : (char*)c->d_frames;
  struct OwnGuard { void* p; ~OwnGuard() { if (p) (void)hipFree(p); } } own_guard{own};   // released on every error path below
  LSPIV_TRY(stage_ring(c, frame_bytes));
  const int64_t fpb = std::max<int64_t>(1, (int64_t)(c->pinned_cap / frame_bytes));
  // sub-batches are cut on the segment anchors -- on the blocks of a sliding handle
  const int64_t align = h->sl_stride ? h->sl_stride : (h->d_shift || h->filter) ? 1 : std::max(1, chunk_alignment_for(h->wy, h->wx, (int64_t)n_win)), base_offset = h->pairs_done;
  if (h->sl_stride)   // the block store grows once per call, not once per sub-batch
    LSPIV_TRY(sliding_reserve(h, (size_t)((base_offset + T - 1 + h->sl_stride - 1) / h->sl_stride), c->stream));
  int64_t launched = 0;
  {
    int batch = 0;
    for (int64_t f0 = 0; f0 < T; ++batch) {
      const int64_t f1 = std::min<int64_t>(T, f0 + fpb);
      LSPIV_TRY(stage_frames(c, batch, d_chunk, frames, dtype, false, frame_elems, f0, f1, signal_threshold));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->staged[batch & 1], 0));
      // pairs [0, f1 - 1) are resident; accumulate up to the last segment anchor below that (everything at the end)
      int64_t p1 = f1 - 1;
      if (f1 < T) p1 = (g_opt_signal_mode.load() == 1 && signal_threshold >= 0.0f) ? 0 : ((base_offset + p1) / align) * align - base_offset;
      const int64_t p0 = launched;
      if (p1 > p0) {
        LSPIV_TRY(ensemble_launch(h, c, d_chunk + (size_t)p0 * frame_bytes, dev_dtype, p1 - p0 + 1, corr_min, s2n_min,
                                  signal_threshold, c->d_out + p0 * n_win, c->d_out + n_tiles + p0 * n_win, c->stream));
        launched = p1;
      }
      f0 = f1;
    }
  }
  if (own) {
    own_guard.p = nullptr;          // the handle owns it from here
    ensemble_keep(h, own, true, (size_t)T * frame_bytes, dev_dtype, T, c->d_out, c->stream);
  }
  HIP_TRY(hipMemcpyAsync(corr_max, c->d_out, n_tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(s2n, c->d_out + n_tiles, n_tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

// ---- float64 rescue of the final fit, in stages (piv_rescue.hip, ens_*) ---------------------------------------------------
// mean planes (count filter) -> c->d_planes, their float32 fits -> c->d_out [u | v]
static int ensemble_mean_fit(lspiv_ensemble* h, DeviceCtx* c, float min_count) {
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols;
  ensemble_wait_accumulated(h, c->stream);   // accumulate_dev may have run on caller streams
  LSPIV_TRY(ensure(&c->d_planes, &c->planes_cap, n_win * h->wy * h->wx * sizeof(float)));
  LSPIV_TRY(ensure(&c->d_out, &c->out_cap, 2 * n_win * sizeof(float)));
  LSPIV_TRY(launch_status(lspiv::launch_ensemble_mean(h->d_sum, h->d_count, min_count, (uint32_t)n_win, h->wy * h->wx, c->d_planes, c->stream)));
  return launch_status(lspiv::launch_peaks_from_planes(c->d_planes, (uint32_t)n_win, h->wy, h->wx, g_opt_border.load(), c->d_out,
                                                       c->d_out + n_win, c->stream));
}
// flag model of the per-pair epilogues (fill_params); the block-per-window kernels (kinds 3 / 9 / 10) assume twice the plane noise
// of the fused FFT kernels there, and so does the mean of their planes here
static float ensemble_flag_k(const lspiv_ensemble* h) {
  const int kind = lspiv_kernel_kind(h->wy, h->wx);
  const double noise_mult = (kind == 3 || kind == 9 || kind == 10) ? 2.0 : 1.0;
  return (float)(noise_mult * 2.0 * g_opt_rescue_kappa.load() * 1e-9 / (0.6931471805599453 * 1e-4));
}
// The flagged windows of a sum whose frames are not all at hand (an imported state, a chunk that could not be retained): nothing to
// re-evaluate them from, but the mean planes in c->d_planes are what the caller gets and what the fit is a function of -- the fit of
// their five samples in float64 (piv_peaks.h) over c->d_out [u | v]; windows the model does not flag keep their bits.  The counters keep
// their meaning: these windows stay "flagged" and "skipped" (left without a re-evaluation from the frames).
static int ensemble_refit_planes(lspiv_ensemble* h, DeviceCtx* c, size_t n_planes = 0) {
  const size_t n_win = n_planes ? n_planes : (size_t)h->g.n_rows * h->g.n_cols;
  return launch_status(lspiv::launch_peaks_from_planes(c->d_planes, (uint32_t)n_win, h->wy, h->wx, g_opt_border.load(), c->d_out,
                                                       c->d_out + n_win, ensemble_flag_k(h), nullptr, c->stream));
}
static lspiv::EnsRescueRec* ensemble_recs(lspiv_ensemble* h) { return reinterpret_cast<lspiv::EnsRescueRec*>((char*)h->d_rescue + 256); }

// flag the windows whose float32 fit (c->d_out, of the mean planes in c->d_planes) cannot be trusted to 1e-4; the records end
// up sorted by window index -- the same list on every handle that holds the same state (multi-GPU: after the all-reduce)
// (n_planes: the planes in c->d_planes and results in c->d_out [u | v] -- the handle's windows, or a tile of a sliding handle's outputs)
static int ensemble_flag(lspiv_ensemble* h, DeviceCtx* c, uint32_t n_planes = 0) {
  h->last_flagged = h->last_rescued = h->last_skipped = 0;
  h->n_rec = 0;
  const uint32_t n_win = n_planes ? n_planes : (uint32_t)(h->g.n_rows * h->g.n_cols);
  const size_t hdr_bytes = 256;
  LSPIV_TRY(ensure(&h->d_rescue, &h->rescue_cap, hdr_bytes + (size_t)n_win * sizeof(lspiv::EnsRescueRec)));
  lspiv::EnsRescueHdr* d_hdr = static_cast<lspiv::EnsRescueHdr*>(h->d_rescue);
  HIP_TRY(hipMemsetAsync(d_hdr, 0, hdr_bytes, c->stream));
  const float k = ensemble_flag_k(h);
  LSPIV_TRY(launch_status(lspiv::launch_ens_flag(c->d_planes, n_win, h->wy, h->wx, c->d_out, c->d_out + n_win, k, (float)(g_opt_rescue_tau.load() * 1e-9),
                                                d_hdr, ensemble_recs(h), n_win, c->stream)));
  lspiv::EnsRescueHdr hdr;
  HIP_TRY(hipMemcpyAsync(&hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  h->last_flagged = hdr.n_rec;
  h->last_skipped = hdr.n_skipped;
  const uint32_t n_rec = std::min<uint32_t>(hdr.n_rec, n_win);
  uint64_t digest = 0xcbf29ce484222325ull;   // FNV-1a
  if (n_rec > 0) {   // the kernel appends in whatever order its waves finish: sort (a few records, once per video)
    std::vector<lspiv::EnsRescueRec> recs(n_rec);
    HIP_TRY(hipMemcpy(recs.data(), ensemble_recs(h), n_rec * sizeof(lspiv::EnsRescueRec), hipMemcpyDeviceToHost));
    std::sort(recs.begin(), recs.end(), [](const lspiv::EnsRescueRec& a, const lspiv::EnsRescueRec& b) { return a.w < b.w; });
    if (n_rec > 1) HIP_TRY(hipMemcpy(ensemble_recs(h), recs.data(), n_rec * sizeof(lspiv::EnsRescueRec), hipMemcpyHostToDevice));
    auto mix = [&digest](uint32_t v) { for (int b = 0; b < 4; ++b) { digest ^= (v >> (8 * b)) & 0xffu; digest *= 0x100000001b3ull; } };
    for (const auto& r : recs) {
      mix(r.w); mix(r.ncand);
      for (uint32_t k = 0; k < std::min<uint32_t>(r.ncand, lspiv::kEnsMaxCand); ++k) mix(r.pos[k]);
    }
  }
  h->rec_digest = digest;
  h->n_rec = n_rec;
  return LSPIV_OK;
}

// this handle's share of the float64 sums: over the pairs of its retained chunks, merged in pair-block order -> h->d_totals
// (n_rec, kEnsMaxCand * 5).  *complete = false (and zeros) when some chunk of this handle could not be kept.
// Sliding handle (count != nullptr): the records index the tile of outputs that starts at output `out0`, `count` is that tile's
// (output, window) count array, and a record sums the pairs of its own output only.
static int ensemble_partials(lspiv_ensemble* h, DeviceCtx* c, bool* complete, const float* count = nullptr, int64_t out0 = 0) {
  const size_t row = (size_t)lspiv::kEnsMaxCand * 5 * sizeof(double);
  LSPIV_TRY(ensure(&h->d_totals, &h->totals_cap, std::max<size_t>(1, h->n_rec) * row));
  ensemble_wait_accumulated(h, c->stream);   // the kept records and frame copies were written on the accumulating streams
  HIP_TRY(hipMemsetAsync(h->d_totals, 0, std::max<size_t>(1, h->n_rec) * row, c->stream));
  *complete = h->retain_complete;
  if (h->n_rec == 0 || !h->retain_complete || h->kept.empty()) return LSPIV_OK;
  uint32_t n_blk = 0;
  for (const auto& kp : h->kept) n_blk += (uint32_t)((kp.T - 1 + lspiv::kEnsPairBlock - 1) / lspiv::kEnsPairBlock);
  const size_t per_rec = (size_t)n_blk * row;
  if ((size_t)h->n_rec * per_rec > ((size_t)4 << 30)) { *complete = false; return LSPIV_OK; }   // (thousands of flagged windows x thousands of pair-blocks)
  LSPIV_TRY(ensure(&h->d_partial, &h->partial_cap, (size_t)h->n_rec * per_rec));
  lspiv::EnsRescueArgs a;
  memset(&a, 0, sizeof(a));
  a.recs = ensemble_recs(h); a.n_rec = h->n_rec; a.n_blk = n_blk; a.partial = h->d_partial; a.count = count ? count : h->d_count;
  if (count) {
    a.virt_nwin = (uint32_t)(h->g.n_rows * h->g.n_cols); a.out0 = (uint32_t)out0;
    a.stride = (uint32_t)h->sl_stride; a.window = (uint32_t)h->sl_window;
  }
  lspiv::PivParams p;
  uint32_t blk0 = 0;
  int64_t pair0 = 0;   // (every chunk of the run is kept, in order: retain_complete)
  for (const auto& kp : h->kept) {
    LSPIV_TRY(fill_params(&p, kp.d_frames, kp.dtype, kp.T, h->H, h->W, h->wy, h->wx, h->oy, h->ox, -1.0f, h->g));
    p.shift = h->d_shift;   // shifted handle: frame t+1's window at the window's clamped offset (ens_partial_kernel, window_shift)
    a.cmax = kp.d_cmax; a.n_pairs = (uint32_t)(kp.T - 1); a.blk0 = blk0; a.pair0 = (uint32_t)pair0;
    LSPIV_TRY(launch_status(lspiv::launch_ens_partial(p, kp.dtype, a, c->stream)));
    blk0 += (a.n_pairs + lspiv::kEnsPairBlock - 1) / lspiv::kEnsPairBlock;
    pair0 += kp.T - 1;
  }
  return launch_status(lspiv::launch_ens_merge(a, h->d_totals, c->stream));
}

// the fit of the flagged windows from the float64 totals (all pairs of the sum), overwriting c->d_out [u | v]
static int ensemble_final(lspiv_ensemble* h, DeviceCtx* c, const double* d_totals, const float* count = nullptr, size_t n_planes = 0) {
  if (h->n_rec == 0) return LSPIV_OK;
  const size_t n_win = n_planes ? n_planes : (size_t)h->g.n_rows * h->g.n_cols;
  lspiv::PivParams p;
  memset(&p, 0, sizeof(p));
  p.wy = h->wy; p.wx = h->wx; p.border_mode = g_opt_border.load();
  lspiv::EnsRescueArgs a;
  memset(&a, 0, sizeof(a));
  a.recs = ensemble_recs(h); a.n_rec = h->n_rec; a.count = count ? count : h->d_count;
  LSPIV_TRY(launch_status(lspiv::launch_ens_final(p, a, d_totals, c->d_out, c->d_out + n_win, c->stream)));
  h->last_rescued = (int64_t)h->n_rec - h->last_skipped;
  return LSPIV_OK;
}

// results of c->d_out / c->d_planes / the count to the caller ("v_sign" applied first)
static int ensemble_deliver(lspiv_ensemble* h, DeviceCtx* c, float* u, float* v, float* corr_count, float* corr_mean) {
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols;
  if (h->d_shift) {
    // shifted handle: the fit and its float64 rescue gave the RESIDUAL; the total displacement adds the clamped offset (one "pair" of
    // n_win results: add_shift_kernel's index is the window then)
    lspiv::PivParams p;
    LSPIV_TRY(fill_params(&p, nullptr, 0, 2, h->H, h->W, h->wy, h->wx, h->oy, h->ox, -1.0f, h->g));
    p.shift = h->d_shift;
    p.u = c->d_out;
    p.v = c->d_out + n_win;
    LSPIV_TRY(launch_status(lspiv::launch_add_shift(p, c->stream)));
  }
  LSPIV_TRY(apply_v_sign(c->d_out + n_win, (int64_t)n_win, c->stream));
  HIP_TRY(hipMemcpyAsync(u, c->d_out, n_win * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(v, c->d_out + n_win, n_win * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (corr_count) HIP_TRY(hipMemcpyAsync(corr_count, h->d_count, n_win * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (corr_mean) HIP_TRY(hipMemcpyAsync(corr_mean, c->d_planes, n_win * h->wy * h->wx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_ensemble_flag(lspiv_ensemble* h, float count_min, float n_frames, int64_t* n_records) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !n_records) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_flag"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  h->flag_min_count = count_min * n_frames;
  h->n_rec = 0;
  *n_records = 0;
  if (!g_opt_rescue.load() || h->filter) return LSPIV_OK;   // (a filtered handle has no rescue: no records, the float32 fits stay)
  LSPIV_TRY(ensemble_mean_fit(h, c, h->flag_min_count));
  LSPIV_TRY(ensemble_flag(h, c));
  *n_records = h->n_rec;
  return LSPIV_OK;
}

int lspiv_ensemble_flag_digest(lspiv_ensemble* h, uint64_t* digest) {
  if (!h || !digest) return fail(LSPIV_EINVAL, "NULL argument");
  *digest = h->n_rec ? h->rec_digest : 0;
  return LSPIV_OK;
}

int lspiv_ensemble_partials(lspiv_ensemble* h, double* partials, int* complete) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !complete || (h->n_rec && !partials)) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_partials"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  bool ok = false;
  LSPIV_TRY(ensemble_partials(h, c, &ok));
  *complete = ok ? 1 : 0;
  if (h->n_rec)
    HIP_TRY(hipMemcpyAsync(partials, h->d_totals, (size_t)h->n_rec * LSPIV_ENS_PARTIAL_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_ensemble_finish_partials(lspiv_ensemble* h, const double* partials, float* u, float* v, float* corr_count, float* corr_mean) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !u || !v || (h->n_rec && !partials)) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_finish_partials"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  LSPIV_TRY(ensemble_mean_fit(h, c, h->flag_min_count));   // the shared workspaces may have been used since lspiv_ensemble_flag
  if (h->n_rec) {
    const size_t bytes = (size_t)h->n_rec * LSPIV_ENS_PARTIAL_DOUBLES * sizeof(double);
    LSPIV_TRY(ensure(&h->d_totals, &h->totals_cap, bytes));
    HIP_TRY(hipMemcpyAsync(h->d_totals, partials, bytes, hipMemcpyHostToDevice, c->stream));
    LSPIV_TRY(ensemble_final(h, c, h->d_totals));
  }
  return ensemble_deliver(h, c, u, v, corr_count, corr_mean);
}

int lspiv_ensemble_set_retain(lspiv_ensemble* h, int mode) {
  if (!h) return fail(LSPIV_EINVAL, "NULL argument");
  if (mode < LSPIV_RETAIN_NONE || mode > LSPIV_RETAIN_BORROW) return fail(LSPIV_EINVAL, "retain mode %d not in {0, 1, 2}", mode);
  h->retain_mode = mode;
  return LSPIV_OK;
}

int lspiv_ensemble_stats(lspiv_ensemble* h, int64_t* stats) {
  if (!h || !stats) return fail(LSPIV_EINVAL, "NULL argument");
  stats[0] = h->last_flagged; stats[1] = h->last_rescued; stats[2] = h->last_skipped;
  stats[3] = (int64_t)h->kept.size(); stats[4] = (int64_t)h->kept_bytes; stats[5] = h->retain_complete ? 1 : 0;
  return LSPIV_OK;
}

int lspiv_ensemble_finish(lspiv_ensemble* h, float count_min, float n_frames, float* u, float* v, float* corr_count,
                          float* corr_mean) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !u || !v) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_finish"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  h->flag_min_count = count_min * n_frames;
  h->n_rec = 0;
  LSPIV_TRY(ensemble_mean_fit(h, c, h->flag_min_count));
  if (h->filter) h->last_flagged = h->last_rescued = h->last_skipped = 0;
  if (g_opt_rescue.load() && !h->filter) {   // (a filtered plane is no sum of lag products: nothing to re-evaluate it from)
    // float64 rescue of the ill-conditioned fits (include/lspiv.h): needs the frames of EVERY pair in the sum -- a state that
    // was imported holds other handles' pairs (the multi-GPU path runs the three stages itself and all-reduces the partials)
    LSPIV_TRY(ensemble_flag(h, c));
    bool complete = false;
    if (h->n_rec && !h->foreign) LSPIV_TRY(ensemble_partials(h, c, &complete));
    if (h->n_rec && complete) LSPIV_TRY(ensemble_final(h, c, h->d_totals));
    else {
      h->last_skipped = h->last_flagged;
      if (h->last_flagged) LSPIV_TRY(ensemble_refit_planes(h, c));
    }
  }
  return ensemble_deliver(h, c, u, v, corr_count, corr_mean);
}

// ---- multi-pass ensemble: shifted handles -------------------------------------------------------------
// `src` (host, or device when on_device) -> the handle's own field, clamped by window_shift on the device; nullptr clears it
static int ensemble_set_shift(lspiv_ensemble* h, const int16_t* src, bool on_device, void* stream, const char* call) {
  if (!h) return fail(LSPIV_EINVAL, "NULL argument");
  if (h->sl_stride) return fail(LSPIV_EINVAL, "%s: this is a sliding ensemble handle (lspiv_ensemble_set_sliding); a sliding ensemble has no shifted pass", call);
  if (h->pairs_done || h->foreign) return fail(LSPIV_EINVAL, "%s must be called before the first accumulate", call);
  if (h->filter && src) return fail(LSPIV_EINVAL, "%s: this is a filtered handle (lspiv_ensemble_set_spectral_filter); a filtered ensemble has no shifted pass", call);
  if (!src) {
    if (h->d_shift) (void)hipFree(h->d_shift);
    h->d_shift = nullptr;
    h->shift_host.clear();
    return LSPIV_OK;
  }
  if (!lspiv_shift_supported(h->wy, h->wx))
    return fail(LSPIV_EUNSUPPORTED, "shifted ensemble pass with window %dx%d is not supported: the window must be square and one of {16, 32, 64}", h->wy, h->wx);
  if (!g_opt_norm_clip.load())
    return fail(LSPIV_EUNSUPPORTED, "option norm_clip = 0 is served by the block-per-window kernels only, not by a shifted ensemble pass");
  if (h->H > 32767 || h->W > 32767)
    return fail(LSPIV_EINVAL, "frame (%lld,%lld): a side above 32767 does not fit the int16 offsets", (long long)h->H, (long long)h->W);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols, bytes = n_win * 2 * sizeof(int16_t);
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(LSPIV_ENOMEM, "hipMalloc window offsets"); }
  std::vector<int16_t> host(n_win * 2);
  lspiv::PivParams p;
  int rc = fill_params(&p, nullptr, 0, 2, h->H, h->W, h->wy, h->wx, h->oy, h->ox, -1.0f, h->g);
  if (rc == LSPIV_OK) {
    p.shift = (const int16_t*)d;
    hipError_t e = hipMemcpyAsync(d, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = lspiv::launch_clamp_shift(p, (int16_t*)d, s);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the field is complete before any accumulate, on whatever stream
    if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(LSPIV_EHIP, "%s: %s", call, hipGetErrorString(e)); }
  }
  if (rc != LSPIV_OK) { (void)hipFree(d); return rc; }
  if (h->d_shift) (void)hipFree(h->d_shift);
  h->d_shift = (int16_t*)d;
  h->shift_host.swap(host);
  return LSPIV_OK;
}
int lspiv_ensemble_set_shift(lspiv_ensemble* h, const int16_t* shift) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  return ensemble_set_shift(h, shift, false, nullptr, "lspiv_ensemble_set_shift");
}
int lspiv_ensemble_set_shift_dev(lspiv_ensemble* h, const int16_t* d_shift, void* stream) {
  return ensemble_set_shift(h, d_shift, true, stream, "lspiv_ensemble_set_shift_dev");
}
int lspiv_ensemble_get_shift(lspiv_ensemble* h, int16_t* shift) {
  if (!h || !shift) return fail(LSPIV_EINVAL, "NULL argument");
  if (!h->d_shift) return fail(LSPIV_EINVAL, "lspiv_ensemble_get_shift: not a shifted handle (lspiv_ensemble_set_shift)");
  memcpy(shift, h->shift_host.data(), h->shift_host.size() * sizeof(int16_t));
  return LSPIV_OK;
}

// ---- SPOF phase-filtered ensemble ---------------------------------------------------------------------
int lspiv_ensemble_set_spectral_filter(lspiv_ensemble* h, int filter) {
  if (!h) return fail(LSPIV_EINVAL, "NULL argument");
  if (filter != LSPIV_FILTER_NONE && filter != LSPIV_FILTER_SPOF) return fail(LSPIV_EINVAL, "spectral filter %d not in {0: none, 1: SPOF}", filter);
  if (h->pairs_done || h->foreign) return fail(LSPIV_EINVAL, "lspiv_ensemble_set_spectral_filter must be called before the first accumulate");
  if (filter && h->sl_stride)
    return fail(LSPIV_EINVAL, "lspiv_ensemble_set_spectral_filter: this is a sliding ensemble handle (lspiv_ensemble_set_sliding); a sliding ensemble has no spectral filter");
  if (filter && h->d_shift)
    return fail(LSPIV_EINVAL, "lspiv_ensemble_set_spectral_filter: this is a shifted handle (lspiv_ensemble_set_shift); a shifted ensemble pass has no spectral filter");
  if (filter) LSPIV_TRY(check_spof(h->wy, h->wx));
  h->filter = filter;
  return LSPIV_OK;
}
int lspiv_ensemble_get_spectral_filter(lspiv_ensemble* h, int* filter) {
  if (!h || !filter) return fail(LSPIV_EINVAL, "NULL argument");
  *filter = h->filter;
  return LSPIV_OK;
}

// ---- sliding ensemble ---------------------------------------------------------------------------------------------------
int lspiv_ensemble_set_sliding(lspiv_ensemble* h, int64_t window_pairs, int64_t stride_pairs) {
  if (!h) return fail(LSPIV_EINVAL, "NULL argument");
  if (h->pairs_done || h->foreign) return fail(LSPIV_EINVAL, "lspiv_ensemble_set_sliding must be called before the first accumulate");
  if (h->d_shift) return fail(LSPIV_EINVAL, "lspiv_ensemble_set_sliding: this is a shifted handle (lspiv_ensemble_set_shift); a sliding ensemble has no shifted pass");
  if (h->filter) return fail(LSPIV_EINVAL, "lspiv_ensemble_set_sliding: this is a filtered handle (lspiv_ensemble_set_spectral_filter); a sliding ensemble has no spectral filter");
  if (stride_pairs < 1 || stride_pairs > window_pairs || window_pairs % stride_pairs != 0 || window_pairs >= (int64_t)1 << 24)
    return fail(LSPIV_EINVAL, "sliding ensemble: need 1 <= stride <= window and window %% stride == 0, got window %lld, stride %lld",
                (long long)window_pairs, (long long)stride_pairs);
  h->sl_window = window_pairs; h->sl_stride = stride_pairs;
  return LSPIV_OK;
}

int lspiv_ensemble_sliding_reserve(lspiv_ensemble* h, int64_t n_pairs) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h) return fail(LSPIV_EINVAL, "NULL argument");
  if (!h->sl_stride) return fail(LSPIV_EINVAL, "lspiv_ensemble_sliding_reserve: not a sliding handle (lspiv_ensemble_set_sliding)");
  if (n_pairs < 0) return fail(LSPIV_EINVAL, "lspiv_ensemble_sliding_reserve: n_pairs %lld", (long long)n_pairs);
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  return sliding_reserve(h, (size_t)((n_pairs + h->sl_stride - 1) / h->sl_stride), c->stream);
}

int lspiv_ensemble_sliding_finish(lspiv_ensemble* h, float count_min, int64_t first_out, int64_t n_out, float* u, float* v,
                                  float* corr_count, float* corr_mean) {
  std::lock_guard<std::mutex> host_lock(locks_here().host);
  if (!h || !u || !v || !corr_count) return fail(LSPIV_EINVAL, "NULL argument");
  if (!h->sl_stride) return fail(LSPIV_EINVAL, "lspiv_ensemble_sliding_finish: not a sliding handle (lspiv_ensemble_set_sliding)");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const int64_t q = h->sl_window / h->sl_stride, n_blk = h->pairs_done / h->sl_stride, total = n_blk - q + 1;
  if (first_out < 0 || n_out < 0 || first_out + n_out > std::max<int64_t>(total, 0))
    return fail(LSPIV_EINVAL, "sliding ensemble: outputs [%lld, %lld) asked for, %lld pairs in blocks of %lld with windows of %lld pairs give %lld",
                (long long)first_out, (long long)(first_out + n_out), (long long)h->pairs_done, (long long)h->sl_stride, (long long)h->sl_window,
                (long long)std::max<int64_t>(total, 0));
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols, plane = (size_t)h->wy * h->wx;
  const float min_count = count_min * (float)h->sl_window;
  const int lane_major = h->sl_layout == 2 ? h->wy : 0;   // as the accumulate calls wrote the store, whatever 'walk' says now
  // tiles of outputs sized to the plane workspace: what it already holds, at least 256 MiB worth, at least one output
  const size_t out_bytes = n_win * plane * sizeof(float);
  // (test hook: LSPIV_SLIDING_TILE_BYTES, read on every call, stands in for that size, so that a few outputs make several tiles)
  const char* tile_env = getenv("LSPIV_SLIDING_TILE_BYTES");
  const size_t tile_bytes = tile_env ? (size_t)std::max<long long>(0, atoll(tile_env)) : std::max<size_t>(c->planes_cap, (size_t)256 << 20);
  int64_t tile = (int64_t)(tile_bytes / out_bytes);
  tile = std::max<int64_t>(1, std::min<int64_t>(tile, std::min<int64_t>(n_out, 65535)));
  tile = std::max<int64_t>(1, std::min<int64_t>(tile, (int64_t)(0x7fffffff / n_win)));   // (records carry the tile's plane index in 32 bits)
  int64_t flagged = 0, rescued = 0, skipped = 0;
  ensemble_wait_accumulated(h, c->stream);   // accumulate_dev may have run on caller streams
  for (int64_t j0 = first_out; j0 < first_out + n_out; j0 += tile) {
    const int64_t nt = std::min<int64_t>(tile, first_out + n_out - j0);
    const size_t n_planes = (size_t)nt * n_win;
    LSPIV_TRY(ensure(&c->d_planes, &c->planes_cap, n_planes * plane * sizeof(float)));
    LSPIV_TRY(ensure(&c->d_out, &c->out_cap, 3 * n_planes * sizeof(float)));   // [u | v | count]
    float* const d_cnt = c->d_out + 2 * n_planes;
    LSPIV_TRY(launch_status(lspiv::launch_ensemble_sliding_mean(h->d_store, h->d_store_cnt, (uint32_t)q, j0, (uint32_t)nt, (uint32_t)n_win, (int)plane,
                                                                min_count, c->d_planes, d_cnt, c->stream, lane_major)));
    LSPIV_TRY(launch_status(lspiv::launch_peaks_from_planes(c->d_planes, (uint32_t)n_planes, h->wy, h->wx, g_opt_border.load(), c->d_out,
                                                             c->d_out + n_planes, c->stream)));
    if (g_opt_rescue.load()) {
      // the float64 rescue of lspiv_ensemble_finish per output: a flagged (output, window) is re-evaluated over that output's pairs
      LSPIV_TRY(ensemble_flag(h, c, (uint32_t)n_planes));
      bool complete = false;
      if (h->n_rec) LSPIV_TRY(ensemble_partials(h, c, &complete, d_cnt, j0));
      if (h->n_rec && complete) LSPIV_TRY(ensemble_final(h, c, h->d_totals, d_cnt, n_planes));
      else {
        h->last_skipped = h->last_flagged;
        if (h->last_flagged) LSPIV_TRY(ensemble_refit_planes(h, c, n_planes));
      }
      flagged += h->last_flagged; rescued += h->last_rescued; skipped += h->last_skipped;
    }
    LSPIV_TRY(apply_v_sign(c->d_out + n_planes, (int64_t)n_planes, c->stream));
    const size_t o = (size_t)(j0 - first_out) * n_win;
    HIP_TRY(hipMemcpyAsync(u + o, c->d_out, n_planes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(v + o, c->d_out + n_planes, n_planes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(corr_count + o, d_cnt, n_planes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (corr_mean) HIP_TRY(hipMemcpyAsync(corr_mean + o * plane, c->d_planes, n_planes * plane * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the workspaces are reused by the next tile
  }
  h->last_flagged = flagged; h->last_rescued = rescued; h->last_skipped = skipped;
  h->n_rec = 0;
  return LSPIV_OK;
}

int lspiv_ensemble_export(lspiv_ensemble* h, float* corr_sum, float* corr_count) {
  if (!h || !corr_sum || !corr_count) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_export"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols;
  ensemble_wait_accumulated(h, c->stream);
  HIP_TRY(hipMemcpyAsync(corr_sum, h->d_sum, n_win * h->wy * h->wx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(corr_count, h->d_count, n_win * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LSPIV_OK;
}

int lspiv_ensemble_import(lspiv_ensemble* h, const float* corr_sum, const float* corr_count, int add) {
  if (!h || !corr_sum || !corr_count) return fail(LSPIV_EINVAL, "NULL argument");
  LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_import"));
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  const size_t n_win = (size_t)h->g.n_rows * h->g.n_cols, np = n_win * h->wy * h->wx;
  // the sums now hold pairs whose frames this handle never saw.  Replaced by a total over several handles (multi-GPU: the
  // all-reduced state): the staged finish (lspiv_ensemble_flag / _partials / _finish_partials) still reaches every pair, each handle
  // through its own retained chunks.  Added to: this handle's chunks no longer tell which pairs are in the sum -- float32 fits.
  if (add) ensemble_give_up_retention(h);
  else h->foreign = true;
  ensemble_wait_accumulated(h, c->stream);
  if (!add) {
    HIP_TRY(hipMemcpyAsync(h->d_sum, corr_sum, np * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(h->d_count, corr_count, n_win * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LSPIV_OK;
  }
  // add on the host side of the boundary: export, sum, import (a few tens of MB, once per video)
  std::vector<float> s(np), k(n_win);
  LSPIV_TRY(lspiv_ensemble_export(h, s.data(), k.data()));
  for (size_t i = 0; i < np; ++i) s[i] += corr_sum[i];
  for (size_t i = 0; i < n_win; ++i) k[i] += corr_count[i];
  return lspiv_ensemble_import(h, s.data(), k.data(), 0);
}

int lspiv_ensemble_allreduce(lspiv_ensemble** handles, int n) {
  if (!handles || n < 1) return fail(LSPIV_EINVAL, "need at least one handle");
  if (n > kAllreduceMax) return fail(LSPIV_EINVAL, "at most %d handles, got %d", kAllreduceMax, n);
  std::vector<int> devs;
  for (int k = 0; k < n; ++k) {
    const lspiv_ensemble* h = handles[k];
    if (!h) return fail(LSPIV_EINVAL, "handle %d is NULL", k);
    LSPIV_TRY(not_on_sliding(h, "lspiv_ensemble_allreduce"));
    const lspiv_ensemble* r = handles[0];
    if (h->H != r->H || h->W != r->W || h->wy != r->wy || h->wx != r->wx || h->oy != r->oy || h->ox != r->ox)
      return fail(LSPIV_ESHAPE, "handle %d has another geometry than handle 0", k);
    if (h->shift_host != r->shift_host)   // (both empty: two plain handles)
      return fail(LSPIV_EINVAL, "handle %d has other window offsets (lspiv_ensemble_set_shift) than handle 0: their sums are not sums of the same planes", k);
    if (h->filter != r->filter)
      return fail(LSPIV_EINVAL, "handle %d has another spectral filter (lspiv_ensemble_set_spectral_filter) than handle 0: their sums are not sums of the same planes", k);
    if (h->device < 0 || h->device >= kMaxDevices) return fail(LSPIV_EINVAL, "handle %d: device %d out of range", k, h->device);
    devs.push_back(h->device);
  }
  std::sort(devs.begin(), devs.end());
  devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  int rc = LSPIV_OK;
  {
    // the host locks of every device involved, in ascending device order (two callers cannot hold one each and wait for the other)
    std::vector<std::unique_lock<std::mutex>> held;
    for (int d : devs) held.emplace_back(g_locks[d].host);
    if (hipSetDevice(handles[0]->device) != hipSuccess) rc = fail(LSPIV_EHIP, "hipSetDevice(%d): %s", handles[0]->device, hipGetErrorString(hipGetLastError()));
    if (rc == LSPIV_OK) rc = ensemble_allreduce_locked(handles, n);
    // the sums now hold pairs whose frames each handle never saw: what lspiv_ensemble_import(add = 0) records (the staged finish)
    if (rc == LSPIV_OK) for (int k = 0; k < n; ++k) handles[k]->foreign = true;
  }
  (void)hipSetDevice(prev);
  return rc;
}

int lspiv_ensemble_destroy(lspiv_ensemble* h) {
  if (!h) return LSPIV_OK;
  ensemble_drop_kept(h);
  for (auto& e : h->acc_events) (void)hipEventDestroy(e.ev);
  for (void* p : {(void*)h->d_sum, (void*)h->d_count, (void*)h->d_part, h->d_rescue, (void*)h->d_partial, (void*)h->d_totals,
                  (void*)h->d_store, (void*)h->d_store_cnt, (void*)h->d_shift})
    if (p) hipFree(p);
  delete h;
  return LSPIV_OK;
}

}  // extern "C"
