// C ABI of liblspiv_hip.so, projection (api_core.hip has the overview): the orthoprojection plans and their tiles, project_cv, the
// host-pointer projection path through the projection slots, and the int16 packing of the results.
#include "api_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "project_tile.h"
#include "project_fused.h"

namespace lspiv {   // project.hip
hipError_t launch_project_u8(const uint8_t* frames, int64_t src_elems, int n_frames, const int* qlo1, const int* qlo2,
                             const uint32_t* qdesc, const int* nn_src, uint8_t* out, int n_out, hipStream_t s);
}

namespace lspiv_api __attribute__((visibility("hidden"))) {

// A projection slot of the current device, locked: the first free one, else the next in turn (callers queue fairly on two locks).
struct ProjSlot {
  std::unique_lock<std::mutex> lk;
  DeviceCtx::ProjWs* ws = nullptr;
};
int take_proj_slot(DeviceCtx* c, ProjSlot* out) {
  DeviceLocks& l = locks_here();
  int k = -1;
  for (int i = 0; i < DeviceCtx::kProjSlots && k < 0; ++i) {
    std::unique_lock<std::mutex> t(l.project[i], std::try_to_lock);
    if (t.owns_lock()) { out->lk = std::move(t); k = i; }
  }
  if (k < 0) {
    k = (int)(l.next_project.fetch_add(1) % DeviceCtx::kProjSlots);
    out->lk = std::unique_lock<std::mutex>(l.project[k]);
  }
  out->ws = &c->proj[k];
  if (!out->ws->stream) HIP_TRY(hipStreamCreateWithFlags(&out->ws->stream, hipStreamNonBlocking));
  return LSPIV_OK;
}

// Host-pointer projection (what a project_hip dask block calls): a projection slot's own stream and buffers under the slot's own lock
// (round 6) -- not the PIV host entry points' workspaces and `host` lock, which a concurrent lspiv_piv_pairs holds from its first
// upload to its last download.  From the first queued copy on, every exit waits for the slot's stream: its DMAs read the caller's
// buffers and the pinned ring, which the next holder of the slot reuses.
template <typename Launch>
static int project_host(size_t ib, size_t ob, const void* frames, void* out, Launch&& launch) {
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  ProjSlot slot;
  LSPIV_TRY(take_proj_slot(c, &slot));
  DeviceCtx::ProjWs* w = slot.ws;
  LSPIV_TRY(ensure(&w->d_in, &w->in_cap, ib));
  LSPIV_TRY(ensure(&w->d_out, &w->out_cap, ob));
  for (int k = 0; k < 2; ++k) {
    if (!w->pin[k]) HIP_TRY(hipHostMalloc(&w->pin[k], DeviceCtx::kProjPinBytes, hipHostMallocDefault));
    if (!w->ev[k]) HIP_TRY(hipEventCreateWithFlags(&w->ev[k], hipEventDisableTiming));
  }
  const size_t slice = DeviceCtx::kProjPinBytes;
  const bool in_pinned = is_pinned(frames), out_pinned = is_pinned(out);
  TraceSpan span;   // (destroyed after the drain below: its events may be pending on the stream)
  struct Drain {
    hipStream_t s;
    ~Drain() { if (s && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError(); }
  } drain{w->stream};
  // up: staging threads copy slice k into one pinned buffer while the DMA of slice k - 1 drains the other
  if (in_pinned) {
    HIP_TRY(hipMemcpyAsync(w->d_in, frames, ib, hipMemcpyHostToDevice, w->stream));
  } else {
    int k = 0;
    for (size_t off = 0; off < ib; off += slice, ++k) {
      const size_t nb = std::min(slice, ib - off);
      if (k >= 2) HIP_TRY(hipEventSynchronize(w->ev[k & 1]));
      staged_copy(w->pin[k & 1], (const char*)frames + off, nb);
      HIP_TRY(hipMemcpyAsync((char*)w->d_in + off, w->pin[k & 1], nb, hipMemcpyHostToDevice, w->stream));
      HIP_TRY(hipEventRecord(w->ev[k & 1], w->stream));
    }
  }
  trace_begin(&span, LSPIV_TRACE_PROJECT_HOST, w->stream);
  LSPIV_TRY(launch(w->d_in, w->d_out, w->stream));
  trace_end(&span, w->stream);
  // down: the DMA of slice k fills one pinned buffer while the staging threads copy slice k - 1 out of the other
  if (out_pinned) {
    HIP_TRY(hipMemcpyAsync(out, w->d_out, ob, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    drain.s = nullptr;
    return LSPIV_OK;
  }
  const size_t n_slices = (ob + slice - 1) / slice;
  for (size_t k = 0; k <= n_slices; ++k) {
    if (k < n_slices) {
      const size_t off = k * slice, nb = std::min(slice, ob - off);
      HIP_TRY(hipMemcpyAsync(w->pin[k & 1], (const char*)w->d_out + off, nb, hipMemcpyDeviceToHost, w->stream));
      HIP_TRY(hipEventRecord(w->ev[k & 1], w->stream));
    }
    if (k >= 1) {
      const size_t off = (k - 1) * slice, nb = std::min(slice, ob - off);
      HIP_TRY(hipEventSynchronize(w->ev[(k - 1) & 1]));
      staged_copy((char*)out + off, w->pin[(k - 1) & 1], nb);
    }
  }
  drain.s = nullptr;   // the last event waited for follows the last copy
  return LSPIV_OK;
}

// ---- tiles of the orthoprojection plans (project.hip: project_tile_kernel, project_tile_f32_kernel) ------------------------------
// A wave owns a block of 64 quads of the ortho grid, 2^lg quads wide and 64 / 2^lg rows high (grids whose rows are not whole quads: 64
// consecutive quads of the flat index), and loads the sorted list of the aligned CHUNKS of the camera frame its cells read (8 bytes of a
// uint8 frame, four pixels of a float32 frame), one chunk per lane and list row.
struct TileShape {
  int lg = 6, rmax = 0;                                     // block width 2^lg quads; list rows of 64 chunks (1, 2 or 4)
  int64_t wq = 0, rows = 0;                                 // quads per grid row, grid rows (flat: all quads in one row)
  int64_t bqx() const { return (int64_t)1 << lg; }
  int64_t bqy() const { return 64 >> lg; }
  int64_t tiles_x() const { return (wq + bqx() - 1) / bqx(); }
  int64_t n_waves() const { return tiles_x() * ((rows + bqy() - 1) / bqy()); }
};

// the sorted chunk list of wave wv into lst; QC: bool(size_t quad, std::vector<int>& lst) appends the chunks a quad reads, false: the
// quad is not served by the tiles.  Returns whether the wave has a quad of its own.
template <class QC>
bool tile_wave_list(const TileShape& sh, int64_t wv, QC& quad_chunks, std::vector<int>& lst) {
  lst.clear();
  const int64_t ty = wv / sh.tiles_x(), tx = wv % sh.tiles_x();
  bool any = false;
  for (int64_t r = ty * sh.bqy(); r < std::min(sh.rows, (ty + 1) * sh.bqy()); ++r)
    for (int64_t c = tx * sh.bqx(); c < std::min(sh.wq, (tx + 1) * sh.bqx()); ++c) any = quad_chunks((size_t)(r * sh.wq + c), lst) || any;
  std::sort(lst.begin(), lst.end());
  lst.erase(std::unique(lst.begin(), lst.end()), lst.end());
  return any;
}

// One list row (64 chunks) when all but 1 in 100 waves fit, else two, else four (2 : 1 oversampling and beyond); among the shapes with
// the shortest lists the one with the fewest chunks wins; waves beyond the list hand their quads to a slow kernel; more than 1 in 100
// beyond four rows: no tiles.  *cap_limit: the list length beyond which a wave goes to the slow kernel (the LSPIV_PROJECT_TILE_CAP hook).
template <class QC>
bool tile_pick_shape(int64_t dst_h, int64_t dst_w, size_t nq, QC& quad_chunks, const char* what, TileShape* out, int* cap_limit) {
  std::vector<TileShape> shapes;
  auto shape = [&](int lg, int64_t wq, int64_t rows) { TileShape t; t.lg = lg; t.wq = wq; t.rows = rows; return t; };
  if (dst_w % 4 == 0) for (int lg : {5, 4, 6, 3}) shapes.push_back(shape(lg, dst_w / 4, dst_h));
  else shapes.push_back(shape(6, (int64_t)nq, 1));
  if (const char* f = getenv("LSPIV_PROJECT_TILE_LG")) {       // A/B: force a block width
    const int lg = atoi(f);
    if (dst_w % 4 == 0 && lg >= 0 && lg <= 6) { shapes.clear(); shapes.push_back(shape(lg, dst_w / 4, dst_h)); }
  }
  const bool say = getenv("LSPIV_PROJECT_DEBUG") != nullptr;
  std::vector<int> lst;
  int best = -1;
  int64_t best_total = 0;
  for (size_t i = 0; i < shapes.size(); ++i) {
    TileShape& sh = shapes[i];
    size_t over1 = 0, over2 = 0, over4 = 0;
    int64_t total = 0, seen = 0;
    // the shapes are compared on a sample of their waves (every k-th, about a thousand: a 1080p grid has 4 600 per shape and four shapes
    // per plan; the builder of the chosen shape then visits every wave and sends whatever does not fit to the slow kernel)
    const int64_t step = std::max<int64_t>(1, sh.n_waves() / 1024);
    for (int64_t wv = 0; wv < sh.n_waves(); wv += step, ++seen) {
      tile_wave_list(sh, wv, quad_chunks, lst);
      over1 += lst.size() > 64; over2 += lst.size() > 128; over4 += lst.size() > 256;
      total += (int64_t)lst.size();
    }
    const size_t few = (size_t)seen / 100;                    // waves a shape may leave to the slow kernel
    sh.rmax = over1 <= few ? 1 : over2 <= few ? 2 : over4 <= few ? 4 : 0;
    total = total * sh.n_waves() / std::max<int64_t>(seen, 1);   // (shapes differ in their number of waves: compare chunks per grid)
    if (say)
      fprintf(stderr, "lspiv projection (%s): blocks of %lld x %lld quads: %.1f chunks per wave, of %lld sampled waves (%lld in all) %zu need more than 64, %zu more than 128, %zu more than 256\n",
              what, (long long)sh.bqx(), (long long)sh.bqy(), (double)total / (double)sh.n_waves(), (long long)seen, (long long)sh.n_waves(), over1, over2, over4);
    if (!sh.rmax) continue;
    if (best < 0 || sh.rmax < shapes[(size_t)best].rmax || (sh.rmax == shapes[(size_t)best].rmax && total < best_total)) { best = (int)i; best_total = total; }
  }
  if (const char* f = getenv("LSPIV_PROJECT_TILE_RMAX"))       // A/B: more list rows than the plan needs
    if (best >= 0 && (atoi(f) == 2 || atoi(f) == 4)) shapes[(size_t)best].rmax = std::max(shapes[(size_t)best].rmax, atoi(f));
  *cap_limit = 256;
  if (const char* f = getenv("LSPIV_PROJECT_TILE_CAP")) {      // test hook: waves with longer lists go to the slow kernel, whatever their share
    *cap_limit = std::max(2, atoi(f));
    if (best < 0) { best = 0; shapes[0].rmax = 1; }
  }
  if (best < 0) return false;
  *out = shapes[(size_t)best];
  return true;
}

// n elements of a host array into a new device allocation (plain hipMemcpy: the project_cv plans)
template <class T>
int upload_new(T** d, const T* v, size_t n) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  *d = static_cast<T*>(p);
  if (n) HIP_TRY(hipMemcpy(p, v, n * sizeof(T), hipMemcpyHostToDevice));
  return LSPIV_OK;
}

}  // namespace lspiv_api

using namespace lspiv_api;

struct lspiv_projection {
  int64_t src_h, src_w, dst_h, dst_w;
  int device;
  int *d_nn, *d_grp_of, *d_grp_off, *d_grp_src;
  int *d_qlo1 = nullptr, *d_qlo2 = nullptr;   // quad-window plan for uint8 frames (project.hip), nullptr: not built
  uint32_t* d_qdesc = nullptr;
  int* d_slow_q = nullptr; int n_slow = 0;    // the quads that plan leaves to the per-cell kernel
  // mixed plan for uint8 frames when the plan has group means (round 6, project.hip: project_mix_kernel): per quad mix_nw 8-byte
  // windows, per cell one byte mask per window and the sample count; nullptr: not built
  int* d_mwin = nullptr; uint32_t* d_mcell = nullptr; int mix_nw = 0;
  int* d_mslow = nullptr; int n_mslow = 0;
  // tiled form of the mixed plan (project_tile_kernel): per wave -- a block of 2^tile_lg x 64 / 2^tile_lg quads -- the sorted list of
  // the 8-byte chunks of the camera frame its windows touch (64 * tile_rmax entries, lane l loads entry l), parked in LDS; the windows
  // of its quads as byte offsets into that tile; nullptr: not built
  int* d_wchunk = nullptr; int* d_twin = nullptr; int tile_rmax = 0, tile_lg = 6, tile_wq = 0, tile_rows = 0;
  int* d_tslow = nullptr; int n_tslow = 0;
  // tiles for float32 frames (project_tile_f32_kernel): chunk lists of four pixels, per cell f_dw descriptor words (tile positions of
  // its samples in the reference's order, count, group flag); nullptr: not built
  int* d_fchunk = nullptr; uint32_t* d_fdesc = nullptr; int f_dw = 0, f_rmax = 0, f_lg = 6, f_wq = 0, f_rows = 0;
  int* d_fslow = nullptr; int n_fslow = 0;
  int64_t n_groups = 0;                       // 0: nearest neighbour only -- uint8 frames may stay uint8 (lspiv_project_frames_u8)
};

struct lspiv_remap {
  int64_t src_h = 0, src_w = 0, dst_h = 0, dst_w = 0;
  bool undistort = false;
  int *d_mx1 = nullptr, *d_my1 = nullptr, *d_mx2 = nullptr, *d_my2 = nullptr;   // integer source coordinates of the undistortion map / of the warp map
  uint16_t *d_mf1 = nullptr, *d_mf2 = nullptr;   // 1/32-pixel fraction index fy * 32 + fx
  void* d_tmp = nullptr; size_t tmp_cap = 0;     // undistorted frames of one call (grow-only)
  // quad plans for uint8 frames (project.hip, remap_win_kernel), one per remap; nullptr: not built
  int *d_qb1 = nullptr, *d_qb2 = nullptr, *d_slow1 = nullptr, *d_slow2 = nullptr;
  uint64_t *d_qd1 = nullptr, *d_qd2 = nullptr;
  int n_slow1 = 0, n_slow2 = 0;
  // both remaps in one kernel for uint8 frames (project.hip, remap_fused_kernel): tiles' boxes, destination pixel descriptors, the
  // undistortion map's quads with the row step; nullptr: not built (the two passes run)
  void* d_ft = nullptr; uint32_t* d_fpx = nullptr; int* d_fqb = nullptr; uint64_t* d_fqd = nullptr;
  int f_tiles = 0, f_tiles_x = 0, f_cap = 0;
  std::mutex host_mu;                      // host-pointer calls on ONE handle queue: they share d_tmp (two handles run side by side)
};

extern "C" {

// ---- orthoprojection (N1) and int16 packing (N4) -------------------------------------------------
int lspiv_projection_create(int64_t src_h, int64_t src_w, int64_t dst_h, int64_t dst_w, const int64_t* idx_img,
                            const int64_t* idx_ortho, int64_t K, const int64_t* src_idx, const int64_t* norm_idx,
                            int64_t M, const int64_t* uidx, int64_t G, lspiv_projection** handle) {
  if (!handle) return fail(LSPIV_EINVAL, "handle is NULL");
  if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || K < 0 || M < 0 || G < 0)
    return fail(LSPIV_ESHAPE, "bad projection shape");
  const int64_t n_src = src_h * src_w, n_out = dst_h * dst_w;
  if (n_src >= (int64_t)1 << 31 || n_out >= (int64_t)1 << 31 || M >= (int64_t)1 << 31)
    return fail(LSPIV_EINVAL, "projection too large for 32-bit indices");
  if ((K > 0 && (!idx_img || !idx_ortho)) || (M > 0 && (!src_idx || !norm_idx)) || (G > 0 && !uidx))
    return fail(LSPIV_EINVAL, "NULL index array");
  if (M > 0 && G == 0) return fail(LSPIV_EINVAL, "group samples without groups");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  // host plan: nearest source per cell; CSR of group members in their ORIGINAL order (stable counting sort)
  std::vector<int> nn((size_t)n_out, -1), grp_of((size_t)n_out, -1), off((size_t)G + 1, 0), members((size_t)M);
  for (int64_t k = 0; k < K; ++k) {
    if (idx_ortho[k] < 0 || idx_ortho[k] >= n_out || idx_img[k] < 0 || idx_img[k] >= n_src)
      return fail(LSPIV_EINVAL, "nearest-neighbour index %lld out of range", (long long)k);
    nn[(size_t)idx_ortho[k]] = (int)idx_img[k];
  }
  for (int64_t g = 0; g < G; ++g) {
    if (uidx[g] < 0 || uidx[g] >= n_out) return fail(LSPIV_EINVAL, "uidx[%lld] out of range", (long long)g);
    grp_of[(size_t)uidx[g]] = (int)g;
  }
  for (int64_t i = 0; i < M; ++i) {
    if (norm_idx[i] < 0 || norm_idx[i] >= G || src_idx[i] < 0 || src_idx[i] >= n_src)
      return fail(LSPIV_EINVAL, "group sample %lld out of range", (long long)i);
    off[(size_t)norm_idx[i] + 1]++;
  }
  for (int64_t g = 0; g < G; ++g) off[(size_t)g + 1] += off[(size_t)g];
  {
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < M; ++i) members[(size_t)cur[(size_t)norm_idx[i]]++] = (int)src_idx[i];
  }
  // the samples of output cell o in the reference's order: its group's members, else its nearest neighbour, else none
  auto samples_of = [&](size_t o, const int** first, int* n) {
    const int g = grp_of[o];
    if (g >= 0) { *first = &members[(size_t)off[(size_t)g]]; *n = off[(size_t)g + 1] - off[(size_t)g]; }
    else if (nn[o] >= 0) { *first = &nn[o]; *n = 1; }
    else { *first = nullptr; *n = 0; }
  };
  lspiv_projection* h = new lspiv_projection();
  h->src_h = src_h; h->src_w = src_w; h->dst_h = dst_h; h->dst_w = dst_w;
  h->n_groups = G;
  h->d_nn = h->d_grp_of = h->d_grp_off = h->d_grp_src = nullptr;
  HIP_TRY(hipGetDevice(&h->device));
  auto up = [&](int** d, const std::vector<int>& v) -> hipError_t {
    const size_t b = std::max<size_t>(v.size(), 1) * sizeof(int);
    hipError_t e = hipMalloc((void**)d, b);
    if (e != hipSuccess) return e;
    // on the library's stream, then waited for: a null-stream hipMemcpy from pageable memory may return before the
    // DMA has landed, and the (non-blocking) stream the kernels run on does not synchronise with the null stream
    if (v.empty()) return hipSuccess;
    e = hipMemcpyAsync(*d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
  };
  hipError_t e = up(&h->d_nn, nn);
  if (e == hipSuccess) e = up(&h->d_grp_of, grp_of);
  if (e == hipSuccess) e = up(&h->d_grp_off, off);
  if (e == hipSuccess) e = up(&h->d_grp_src, members);
  // quad-window plan (uint8 frames): per four consecutive output cells two 8-byte source windows and, per cell, window +
  // byte.  Built when the grid has whole quads and most of them fit (a smooth homography: a few source bytes per quad,
  // one camera row or two); LSPIV_PROJECT_ONE_CELL=1 keeps the one-cell kernel for A/B.
  if (e == hipSuccess && n_out % 4 == 0 && n_src >= 8 && !getenv("LSPIV_PROJECT_ONE_CELL")) {
    const size_t nq = (size_t)n_out / 4;
    std::vector<int> qlo1(nq, 0), qlo2(nq, 0);
    std::vector<int> qdesc(nq, 0), slow;
    size_t fit = 0;
    for (size_t q = 0; q < nq; ++q) {
      const int* v = &nn[4 * q];
      bool ok = true;
      for (int k = 0; k < 4; ++k) ok = ok && grp_of[4 * q + k] < 0;
      int lo1 = -1, lo2 = -1;
      for (int k = 0; k < 4 && ok; ++k)
        if (v[k] >= 0 && (lo1 < 0 || v[k] < lo1)) lo1 = v[k];
      for (int k = 0; k < 4 && ok; ++k)
        if (v[k] >= 0 && v[k] - lo1 > 7 && (lo2 < 0 || v[k] < lo2)) lo2 = v[k];
      for (int k = 0; k < 4 && ok; ++k)
        if (v[k] >= 0 && v[k] - lo1 > 7 && v[k] - lo2 > 7) ok = false;
      if (!ok) { qdesc[q] = (int)0x80000000u; slow.push_back((int)q); continue; }
      if (lo1 < 0) lo1 = 0;
      if (lo2 < 0) lo2 = lo1;
      const int w1 = (int)std::min<int64_t>(lo1, n_src - 8), w2 = (int)std::min<int64_t>(lo2, n_src - 8);   // windows end inside the frame
      uint32_t d = 0;
      for (int k = 0; k < 4; ++k) {
        if (v[k] < 0) continue;
        const bool second = v[k] - lo1 > 7;
        d |= ((uint32_t)(v[k] - (second ? w2 : w1)) | (second ? 8u : 0u) | 16u) << (5 * k);
      }
      qlo1[q] = w1; qlo2[q] = w2; qdesc[q] = (int)d;
      ++fit;
    }
    if (fit * 10 >= nq * 9) {
      e = up(&h->d_qlo1, qlo1);
      if (e == hipSuccess) e = up(&h->d_qlo2, qlo2);
      int* dd = nullptr;
      if (e == hipSuccess) e = up(&dd, qdesc);
      h->d_qdesc = reinterpret_cast<uint32_t*>(dd);
      if (e == hipSuccess) e = up(&h->d_slow_q, slow);
      h->n_slow = (int)slow.size();
    }
  }
  // mixed plan (round 6): a plan with group means, uint8 frames.  Every cell is a set of samples (its group in the reference's
  // order, else its nearest-neighbour byte, else nothing); the samples of a quad are covered greedily with 8-byte windows over
  // the FLAT source index; a quad fits with at most NW windows and at most 255 samples per cell.
  // (nearest-neighbour-only plans too: a group of one sample -- their float32 output goes through the same tiled kernel)
  if (e == hipSuccess && n_out % 4 == 0 && n_src >= 16 && !getenv("LSPIV_PROJECT_ONE_CELL") && !getenv("LSPIV_PROJECT_NO_MIX")) {
    const size_t nq = (size_t)n_out / 4;
    std::vector<int> need(nq, 0);
    std::vector<int> px;
    auto windows_of = [&](size_t q, int* starts, int cap) -> int {     // greedy cover of the quad's sample set; returns the number of windows
      px.clear();
      for (int k = 0; k < 4; ++k) {
        const int* f; int n;
        samples_of(4 * q + k, &f, &n);
        px.insert(px.end(), f, f + n);
      }
      std::sort(px.begin(), px.end());
      int nw = 0;
      int64_t end = -1;
      for (int v : px) {
        if (v < end) continue;
        int64_t st = std::min<int64_t>(v, n_src - 8);
        // the kernel reads the three aligned dwords around a window in one 12-byte load: they must lie inside the frame
        if ((st & ~(int64_t)3) + 12 > n_src) st = std::min<int64_t>(st, (n_src - 12) & ~(int64_t)3);
        if (v >= st + 8) return cap + 1;                     // the frame's last bytes cannot be reached that way: the slow kernel's quad
        if (nw < cap) starts[nw] = (int)st;
        ++nw;
        end = st + 8;
      }
      return nw;
    };
    size_t over2 = 0, over4 = 0;
    int tmp[4];
    for (size_t q = 0; q < nq; ++q) {
      need[q] = windows_of(q, tmp, 4);
      over2 += need[q] > 2;
      over4 += need[q] > 4;
    }
    const int NW = over2 * 50 <= nq ? 2 : 4;                 // at most 2 % of the quads left to the slow kernel: two windows will do
    const size_t left = NW == 2 ? over2 : over4;
    if (getenv("LSPIV_PROJECT_DEBUG"))
      fprintf(stderr, "lspiv projection: %zu quads, %zu need more than two 8-byte windows, %zu more than four: %s\n", nq, over2, over4,
              left * 10 <= nq ? (NW == 2 ? "mixed plan, two windows" : "mixed plan, four windows") : "no mixed plan");
    if (left * 10 <= nq) {                                   // otherwise the geometry is too scattered for windows: the one-cell kernel
      const int CW = NW / 2;
      std::vector<int> mwin(nq * NW, 0), mslow;
      std::vector<int> mcell(nq * 4 * CW, 0);
      for (size_t q = 0; q < nq; ++q) {
        int st[4] = {0, 0, 0, 0};
        bool ok = need[q] <= NW;
        const int nw = ok ? windows_of(q, st, NW) : 0;
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 4 && ok; ++k) {
          const int* f; int n;
          samples_of(4 * q + k, &f, &n);
          if (n > 255) { ok = false; break; }            // the kernel's division-free quotient is checked for counts up to 255
          uint32_t masks = 0;
          for (int i = 0; i < n; ++i) {
            int wsel = -1;
            for (int j = 0; j < nw; ++j)
              if (f[i] >= st[j] && f[i] < st[j] + 8) { wsel = j; break; }
            if (wsel < 0) { ok = false; break; }
            masks |= 1u << (8 * wsel + (f[i] - st[wsel]));
          }
          const uint32_t cnt = (uint32_t)std::max(n, 1);     // a cell without samples: 0 / 1
          if (NW == 2) words[k] = masks | (cnt << 16);
          else { words[2 * k] = masks; words[2 * k + 1] = cnt; }
        }
        if (!ok) {
          mwin[q * NW] = -1;
          mslow.push_back((int)q);
          continue;
        }
        for (int j = 0; j < NW; ++j) mwin[q * NW + j] = st[j < nw ? j : 0];    // unused windows repeat the first (masks 0)
        if (nw == 0) for (int j = 0; j < NW; ++j) mwin[q * NW + j] = 0;
        for (int j = 0; j < 4 * CW; ++j) mcell[q * 4 * CW + j] = (int)words[j];
      }
      e = up(&h->d_mwin, mwin);
      int* dc = nullptr;
      if (e == hipSuccess) e = up(&dc, mcell);
      h->d_mcell = reinterpret_cast<uint32_t*>(dc);
      if (e == hipSuccess) e = up(&h->d_mslow, mslow);
      h->n_mslow = (int)mslow.size();
      h->mix_nw = NW;
      // tiled form (project_tile_kernel): chunks of 8 bytes; the three dwords around a window lie in chunk c0 = (start & ~3) >> 3 and
      // c0 + 1, neighbours in the wave's sorted list; a window becomes its byte offset into the wave's tile.
      if (e == hipSuccess && n_src % 8 == 0 && !getenv("LSPIV_PROJECT_NO_TILE")) {
        std::vector<int> qch(nq * NW, -1);                   // per quad and window: c0, or -1 (window unused / quad not served)
        for (size_t q = 0; q < nq; ++q) {
          if (mwin[q * NW] < 0) continue;
          for (int j = 0; j < NW; ++j) {
            uint32_t m = 0;                                  // window j's masks of the four cells: none set = the window is not read
            for (int k = 0; k < 4; ++k) m |= ((uint32_t)mcell[q * 4 * CW + (size_t)k * CW] >> (8 * j)) & 0xffu;
            if (m) qch[q * NW + j] = (mwin[q * NW + j] & ~3) >> 3;
          }
        }
        auto quad_chunks = [&](size_t q, std::vector<int>& l) {
          if (mwin[q * NW] < 0) return false;
          for (int j = 0; j < NW; ++j)
            if (qch[q * NW + j] >= 0) { l.push_back(qch[q * NW + j]); l.push_back(qch[q * NW + j] + 1); }
          return true;
        };
        TileShape sh;
        int cap_limit = 0;
        if (tile_pick_shape(dst_h, dst_w, nq, quad_chunks, "uint8", &sh, &cap_limit)) {
          const int cap = 64 * sh.rmax;
          size_t failed = 0;
          std::vector<int> lst, wchunk((size_t)sh.n_waves() * cap, -1), twin(mwin.size(), 0), tslow(mslow);
          for (size_t q = 0; q < nq; ++q) if (mwin[q * NW] < 0) twin[q * NW] = -1;
          for (int64_t wv = 0; wv < sh.n_waves(); ++wv) {
            if (!tile_wave_list(sh, wv, quad_chunks, lst)) continue;      // (all -1: the wave returns at once)
            const int64_t ty = wv / sh.tiles_x(), tx = wv % sh.tiles_x();
            const bool fits = (int)lst.size() <= std::min(cap, cap_limit);
            failed += !fits;
            if (fits) {
              if (lst.empty()) lst.push_back(0);             // cells without a source only: the wave still runs and writes their zeros
              for (int i = 0; i < cap; ++i) wchunk[(size_t)wv * cap + i] = lst[std::min<size_t>((size_t)i, lst.size() - 1)];
            }
            for (int64_t r = ty * sh.bqy(); r < std::min(sh.rows, (ty + 1) * sh.bqy()); ++r)
              for (int64_t c = tx * sh.bqx(); c < std::min(sh.wq, (tx + 1) * sh.bqx()); ++c) {
                const size_t q = (size_t)(r * sh.wq + c);
                if (mwin[q * NW] < 0) continue;
                if (!fits) { twin[q * NW] = -1; tslow.push_back((int)q); continue; }
                for (int j = 0; j < NW; ++j) {
                  const int c0 = qch[q * NW + j];
                  if (c0 < 0) continue;                       // (offset 0: any resident bytes do under a zero mask)
                  const int pos = (int)(std::lower_bound(lst.begin(), lst.end(), c0) - lst.begin());
                  twin[q * NW + j] = 8 * pos + (mwin[q * NW + j] - 8 * c0);
                }
              }
          }
          if (getenv("LSPIV_PROJECT_DEBUG"))
            fprintf(stderr, "lspiv projection (uint8): tiles of %lld x %lld quads, %d list row(s), %zu waves to the slow kernel (%zu slow quads in all)\n",
                    (long long)sh.bqx(), (long long)sh.bqy(), sh.rmax, failed, tslow.size());
          e = up(&h->d_wchunk, wchunk);
          if (e == hipSuccess) e = up(&h->d_twin, twin);
          if (e == hipSuccess) e = up(&h->d_tslow, tslow);
          h->n_tslow = (int)tslow.size();
          h->tile_rmax = sh.rmax; h->tile_lg = sh.lg; h->tile_wq = (int)sh.wq; h->tile_rows = (int)sh.rows;
        }
      }
    }
  }
  // float32 frames in tiles (project_tile_f32_kernel): chunks of four pixels; a cell = the tile positions of its samples in the
  // reference's order (the group's members, or the one nearest neighbour), at most 6 (two descriptor words per cell) or 9 (three).
  if (e == hipSuccess && n_out % 4 == 0 && n_src % 4 == 0 && !getenv("LSPIV_PROJECT_ONE_CELL") && !getenv("LSPIV_PROJECT_NO_TILE")) {
    const size_t nq = (size_t)n_out / 4;
    auto count_of = [&](size_t o) { const int g = grp_of[o]; return g >= 0 ? off[(size_t)g + 1] - off[(size_t)g] : nn[o] >= 0 ? 1 : 0; };
    size_t over6 = 0, over9 = 0;
    for (size_t q = 0; q < nq; ++q) {
      int m = 0;
      for (int k = 0; k < 4; ++k) m = std::max(m, count_of(4 * q + k));
      over6 += m > 6; over9 += m > 9;
    }
    const int DW = over6 * 100 <= nq ? 2 : 3, maxs = 3 * DW;
    if (getenv("LSPIV_PROJECT_DEBUG"))
      fprintf(stderr, "lspiv projection (float32): %zu quads, %zu with a cell of more than 6 samples, %zu of more than 9: %s\n", nq, over6, over9,
              (DW == 2 ? over6 : over9) * 10 <= nq ? (DW == 2 ? "two descriptor words per cell" : "three descriptor words per cell") : "no tiles");
    if ((DW == 2 ? over6 : over9) * 10 <= nq) {
      auto served = [&](size_t q) {
        for (int k = 0; k < 4; ++k) if (count_of(4 * q + k) > maxs) return false;
        return true;
      };
      auto quad_chunks = [&](size_t q, std::vector<int>& l) {
        if (!served(q)) return false;
        for (int k = 0; k < 4; ++k) {
          const int* f; int n;
          samples_of(4 * q + k, &f, &n);
          for (int i = 0; i < n; ++i) l.push_back(f[i] >> 2);
        }
        return true;
      };
      TileShape sh;
      int cap_limit = 0;
      if (tile_pick_shape(dst_h, dst_w, nq, quad_chunks, "float32", &sh, &cap_limit)) {
        const int cap = 64 * sh.rmax;
        size_t failed = 0;
        std::vector<int> lst, wchunk((size_t)sh.n_waves() * cap, -1), fdesc(nq * 4 * DW, 0), fslow;
        for (size_t q = 0; q < nq; ++q) if (!served(q)) { fdesc[q * 4 * DW] = -1; fslow.push_back((int)q); }
        for (int64_t wv = 0; wv < sh.n_waves(); ++wv) {
          if (!tile_wave_list(sh, wv, quad_chunks, lst)) continue;
          const int64_t ty = wv / sh.tiles_x(), tx = wv % sh.tiles_x();
          const bool fits = (int)lst.size() <= std::min(cap, cap_limit);
          failed += !fits;
          if (fits) {
            if (lst.empty()) lst.push_back(0);
            for (int i = 0; i < cap; ++i) wchunk[(size_t)wv * cap + i] = lst[std::min<size_t>((size_t)i, lst.size() - 1)];
          }
          for (int64_t r = ty * sh.bqy(); r < std::min(sh.rows, (ty + 1) * sh.bqy()); ++r)
            for (int64_t c = tx * sh.bqx(); c < std::min(sh.wq, (tx + 1) * sh.bqx()); ++c) {
              const size_t q = (size_t)(r * sh.wq + c);
              if (!served(q)) continue;
              if (!fits) { fdesc[q * 4 * DW] = -1; fslow.push_back((int)q); continue; }
              for (int k = 0; k < 4; ++k) {
                const int* f; int n;
                samples_of(4 * q + k, &f, &n);
                uint32_t w[3] = {0, 0, 0};
                for (int i = 0; i < n; ++i) {
                  const int pos = 4 * (int)(std::lower_bound(lst.begin(), lst.end(), f[i] >> 2) - lst.begin()) + (f[i] & 3);
                  w[i / 3] |= (uint32_t)pos << (10 * (i % 3));
                }
                const uint32_t grp = grp_of[4 * q + k] >= 0;
                w[0] |= ((uint32_t)n & 3u) << 30;
                if (DW == 2) w[1] |= (((uint32_t)n >> 2) & 1u) << 30 | grp << 31;
                else { w[1] |= (((uint32_t)n >> 2) & 3u) << 30; w[2] |= grp << 30; }
                for (int j = 0; j < DW; ++j) fdesc[(q * 4 + (size_t)k) * DW + j] = (int)w[j];
              }
            }
        }
        if (getenv("LSPIV_PROJECT_DEBUG"))
          fprintf(stderr, "lspiv projection (float32): tiles of %lld x %lld quads, %d list row(s), %zu waves to the slow kernel (%zu slow quads in all)\n",
                  (long long)sh.bqx(), (long long)sh.bqy(), sh.rmax, failed, fslow.size());
        e = up(&h->d_fchunk, wchunk);
        int* dd = nullptr;
        if (e == hipSuccess) e = up(&dd, fdesc);
        h->d_fdesc = reinterpret_cast<uint32_t*>(dd);
        if (e == hipSuccess) e = up(&h->d_fslow, fslow);
        h->n_fslow = (int)fslow.size();
        h->f_dw = DW; h->f_rmax = sh.rmax; h->f_lg = sh.lg; h->f_wq = (int)sh.wq; h->f_rows = (int)sh.rows;
      }
    }
  }
  if (e != hipSuccess) {
    lspiv_projection_destroy(h);
    return fail(e == hipErrorOutOfMemory ? LSPIV_ENOMEM : LSPIV_EHIP, "projection plan upload: %s", hipGetErrorString(e));
  }
  *handle = h;
  return LSPIV_OK;
}

int lspiv_project_frames_dev(lspiv_projection* h, const void* d_frames, int dtype, int64_t T, float* d_out, void* stream) {
  if (!h || !d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T < 0 || T >= (int64_t)1 << 28) return fail(LSPIV_ESHAPE, "bad frame count");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const bool tile = dtype == 0 && h->d_mcell && h->d_twin && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_frames) & 7) == 0;
  const bool win = dtype == 0 && !tile && h->d_qdesc && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
  const bool mix = dtype == 0 && !tile && !win && h->d_mcell && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
  const bool tile_f = dtype == 1 && h->d_fdesc && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_frames) & 15) == 0;
  hipError_t e = tile_f ? lspiv::launch_project_tile_f32((const float*)d_frames, h->src_h * h->src_w, (int)T, h->f_dw, h->f_rmax, h->d_fchunk, h->d_fdesc,
                                                          h->f_wq, h->f_rows, h->f_lg, h->d_fslow, h->n_fslow, h->d_nn, h->d_grp_of, h->d_grp_off, h->d_grp_src,
                                                          d_out, (int)(h->dst_h * h->dst_w), s)
               : tile ? lspiv::launch_project_tile((const uint8_t*)d_frames, h->src_h * h->src_w, (int)T, h->mix_nw, h->tile_rmax, h->d_wchunk, h->d_twin,
                                                    h->d_mcell, h->tile_wq, h->tile_rows, h->tile_lg, h->d_tslow, h->n_tslow, h->d_nn, h->d_grp_of, h->d_grp_off, h->d_grp_src, d_out,
                                                    (int)(h->dst_h * h->dst_w), s)
               : mix ? lspiv::launch_project_mix((const uint8_t*)d_frames, h->src_h * h->src_w, (int)T, h->mix_nw, h->d_mwin, h->d_mcell, h->d_mslow,
                                                  h->n_mslow, h->d_nn, h->d_grp_of, h->d_grp_off, h->d_grp_src, d_out, (int)(h->dst_h * h->dst_w), s)
               : win ? lspiv::launch_project_win((const uint8_t*)d_frames, h->src_h * h->src_w, (int)T, h->d_qlo1, h->d_qlo2, h->d_qdesc,
                                                  h->d_slow_q, h->n_slow, h->d_nn, h->d_grp_of, h->d_grp_off, h->d_grp_src, d_out, (int)(h->dst_h * h->dst_w), s)
                     : lspiv::launch_project(d_frames, dtype, h->src_h * h->src_w, (int)T, h->d_nn, h->d_grp_of, h->d_grp_off,
                                             h->d_grp_src, d_out, (int)(h->dst_h * h->dst_w), s);
  return launch_status(e);
}

int lspiv_project_frames(lspiv_projection* h, const void* frames, int dtype, int64_t T, float* out) {
  if (!h || !frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype < 0 || dtype > 2) return fail(LSPIV_EINVAL, "dtype %d not in {0:u8, 1:f32, 2:f64}", dtype);
  if (T <= 0) return LSPIV_OK;
  const size_t ib = (size_t)T * h->src_h * h->src_w * elem_size(dtype);
  const size_t ob = (size_t)T * h->dst_h * h->dst_w * sizeof(float);
  return project_host(ib, ob, frames, out, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_project_frames_dev(h, d_in, dtype, T, (float*)d_out, s);
  });
}

int lspiv_project_frames_u8_dev(lspiv_projection* h, const uint8_t* d_frames, int64_t T, uint8_t* d_out, void* stream) {
  if (!h || !d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (h->n_groups != 0)
    return fail(LSPIV_EINVAL, "the plan averages %lld cells (reducer \"mean\"): their values are no bytes, use lspiv_project_frames",
                (long long)h->n_groups);
  if (T < 0 || T >= (int64_t)1 << 28) return fail(LSPIV_ESHAPE, "bad frame count");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const bool tile = h->d_mcell && h->d_twin && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_frames) & 7) == 0;
  hipError_t e = tile ? lspiv::launch_project_tile_u8(d_frames, h->src_h * h->src_w, (int)T, h->mix_nw, h->tile_rmax, h->d_wchunk, h->d_twin, h->d_mcell,
                                                       h->tile_wq, h->tile_rows, h->tile_lg, h->d_tslow, h->n_tslow, h->d_nn, d_out,
                                                       (int)(h->dst_h * h->dst_w), s)
                      : lspiv::launch_project_u8(d_frames, h->src_h * h->src_w, (int)T, h->d_qlo1, h->d_qlo2, h->d_qdesc, h->d_nn, d_out,
                                                 (int)(h->dst_h * h->dst_w), s);
  return launch_status(e);
}

int lspiv_project_frames_u8(lspiv_projection* h, const uint8_t* frames, int64_t T, uint8_t* out) {
  if (!h || !frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (T <= 0) return LSPIV_OK;
  const size_t ib = (size_t)T * h->src_h * h->src_w, ob = (size_t)T * h->dst_h * h->dst_w;
  return project_host(ib, ob, frames, out, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_project_frames_u8_dev(h, (const uint8_t*)d_in, T, (uint8_t*)d_out, s);
  });
}

int lspiv_projection_destroy(lspiv_projection* h) {
  if (!h) return LSPIV_OK;
  for (void* p : {(void*)h->d_nn, (void*)h->d_grp_of, (void*)h->d_grp_off, (void*)h->d_grp_src, (void*)h->d_qlo1, (void*)h->d_qlo2,
                  (void*)h->d_qdesc, (void*)h->d_slow_q, (void*)h->d_mwin, (void*)h->d_mcell, (void*)h->d_mslow, (void*)h->d_wchunk,
                  (void*)h->d_twin, (void*)h->d_tslow, (void*)h->d_fchunk, (void*)h->d_fdesc, (void*)h->d_fslow})
    if (p) hipFree(p);
  delete h;
  return LSPIV_OK;
}

namespace {
// saturate_cast<int>(double): round half to even, saturating
int64_t cv_round(double v) {
  if (!(v == v)) return 0;
  if (v >= 2147483647.0) return 2147483647;
  if (v <= -2147483648.0) return -2147483648LL;
  return (int64_t)std::nearbyint(v);
}
bool invert3(const double* m, double* o) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  if (det == 0.0 || !(det == det)) return false;
  const double r = 1.0 / det;
  o[0] = (e * i - f * h) * r; o[1] = (c * h - b * i) * r; o[2] = (b * f - c * e) * r;
  o[3] = (f * g - d * i) * r; o[4] = (a * i - c * g) * r; o[5] = (c * d - a * f) * r;
  o[6] = (d * h - e * g) * r; o[7] = (b * g - a * h) * r; o[8] = (a * e - b * d) * r;
  return true;
}
int upload_map(const std::vector<int>& mx, const std::vector<int>& my, const std::vector<uint16_t>& mf, int** d_mx, int** d_my,
               uint16_t** d_mf) {
  const size_t n = mx.size();
  int rc = upload_new(d_mx, mx.data(), n);
  if (!rc) rc = upload_new(d_my, my.data(), n);
  return rc ? rc : upload_new(d_mf, mf.data(), n);
}
int clamp_short(int64_t v) { return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }   // OpenCV keeps the integer part as short

// Quad plan of a remap for uint8 frames: four consecutive destination pixels whose 2 x 2 source neighbourhoods are all
// interior, share the source row pair and fit 8 bytes (max ix - min ix <= 6) read two 8-byte windows instead of eight 2-byte
// pairs.  Built when the destination has whole quads and >= 80 % of them qualify; the others are listed for the per-pixel
// kernel.  LSPIV_PROJECT_ONE_CELL=1 skips it (A/B).
int build_remap_quads(const std::vector<int>& mx, const std::vector<int>& my, const std::vector<uint16_t>& mf, int64_t Hs, int64_t Ws,
                      int** d_qb, uint64_t** d_qd, int** d_slow, int* n_slow) {
  const size_t n = mx.size();
  if (n % 4 != 0 || Hs * Ws < 16 || getenv("LSPIV_PROJECT_ONE_CELL")) return LSPIV_OK;
  const size_t nq = n / 4;
  std::vector<int> qb(nq, 0), slow;
  std::vector<uint64_t> qd(nq, 0);
  for (size_t q = 0; q < nq; ++q) {
    const size_t o = 4 * q;
    bool ok = true, outside = true;
    int lo = mx[o], hi = mx[o];
    for (int k = 0; k < 4; ++k) {
      const int ix = mx[o + k], iy = my[o + k];
      ok = ok && ix >= 0 && ix + 1 < Ws && iy >= 0 && iy + 1 < Hs && iy == my[o];
      outside = outside && !((ix >= -1 && ix < Ws) && (iy >= -1 && iy < Hs));   // no neighbour of the 2 x 2 patch inside
      lo = std::min(lo, ix); hi = std::max(hi, ix);
    }
    if (outside) { qd[q] = (uint64_t)1 << 62; continue; }
    const int64_t base = ok ? (int64_t)my[o] * Ws + lo : 0;
    ok = ok && hi - lo <= 6 && base + Ws + 8 <= Hs * Ws;     // both windows end inside the frame
    if (!ok) { qd[q] = (uint64_t)1 << 63; slow.push_back((int)q); continue; }
    uint64_t d = 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t fr = mf[o + k], fx = fr & 31u, fy = fr >> 5;
      d |= (uint64_t)((uint32_t)(mx[o + k] - lo) | (fx << 3) | (fy << 8)) << (16 * k);
    }
    qb[q] = (int)base; qd[q] = d;
  }
  if (slow.size() * 5 > nq) return LSPIV_OK;                  // fewer than 80 % fit: the per-pixel kernel does everything
  int rc = upload_new(d_qb, qb.data(), nq);
  if (!rc) rc = upload_new(d_qd, qd.data(), nq);
  if (!rc) rc = upload_new(d_slow, slow.data(), slow.size());
  if (!rc) *n_slow = (int)slow.size();
  return rc;
}

// Plan of remap_fused_kernel (project.hip): undistortion and warp of uint8 frames in one kernel.  Built when both widths are multiples of
// four and every 64 x 16 destination tile's box of undistorted pixels fits 16 000 bytes; LSPIV_PROJECT_CV_TWO_PASS=1 skips it (A/B, tests).
int build_remap_fused(lspiv_remap* h, const std::vector<int>& mx1, const std::vector<int>& my1, const std::vector<uint16_t>& mf1,
                      const std::vector<int>& mx2, const std::vector<int>& my2, const std::vector<uint16_t>& mf2) {
  const int64_t Hs = h->src_h, Ws = h->src_w, Hd = h->dst_h, Wd = h->dst_w;
  if (Ws % 4 != 0 || Wd % 4 != 0 || Hs * Ws < 64 || Hs > 32767 || Ws > 32767 || Hd > 32767 || Wd > 32767 ||   // (24-bit index arithmetic in the kernel)
      getenv("LSPIV_PROJECT_CV_TWO_PASS")) return LSPIV_OK;
  // the undistortion map by quads: two or three 8-byte windows of the camera frame per four undistorted pixels
  const size_t nq = (size_t)(Hs * Ws / 4);
  std::vector<int> qb(nq, 0);
  std::vector<uint64_t> qd(nq, 0);
  size_t n_slow = 0;
  for (size_t q = 0; q < nq; ++q) {
    const size_t o = 4 * q;
    bool ok = true, outside = true;
    int lo = mx1[o], hi = mx1[o], ylo = my1[o], yhi = my1[o];
    for (int k = 0; k < 4; ++k) {
      const int ix = mx1[o + k], iy = my1[o + k];
      ok = ok && ix >= 0 && ix + 1 < Ws && iy >= 0 && iy + 1 < Hs;
      outside = outside && !((ix >= -1 && ix < Ws) && (iy >= -1 && iy < Hs));
      lo = std::min(lo, ix); hi = std::max(hi, ix); ylo = std::min(ylo, iy); yhi = std::max(yhi, iy);
    }
    if (outside) { qd[q] = (uint64_t)1 << 62; continue; }
    const int64_t base = ok ? (int64_t)ylo * Ws + lo : 0;
    ok = ok && hi - lo <= 6 && yhi - ylo <= 1 && (base & ~(int64_t)3) + (int64_t)(yhi - ylo + 1) * Ws + 12 <= Hs * Ws;   // every 12-byte load (from the dword below the window) ends inside the frame
    if (!ok) { qd[q] = (uint64_t)1 << 63; ++n_slow; continue; }
    uint64_t d = yhi > ylo ? (uint64_t)1 << 15 : 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t fr = mf1[o + k], fx = fr & 31u, fy = fr >> 5;
      d |= (uint64_t)((uint32_t)(mx1[o + k] - lo) | (fx << 3) | (fy << 8) | ((uint32_t)(my1[o + k] - ylo) << 13)) << (16 * k);
    }
    qb[q] = (int)base; qd[q] = d;
  }
  if (n_slow * 5 > nq) return LSPIV_OK;                       // a map this folded: the per-pixel path would pace every wave
  // the warp by tiles
  constexpr int TW = 64, TH = 16;
  const int tiles_x = (int)((Wd + TW - 1) / TW), tiles_y = (int)((Hd + TH - 1) / TH);
  std::vector<int> tiles((size_t)tiles_x * tiles_y * 4, 0);
  std::vector<uint32_t> pxd((size_t)(Hd * Wd), 0x80000000u);
  int cap = 16;
  auto inside = [&](int ix, int iy) { return (ix >= -1 && ix < Ws) && (iy >= -1 && iy < Hs); };
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      int xlo = INT_MAX, xhi = INT_MIN, ylo = INT_MAX, yhi = INT_MIN;
      const int64_t y1 = std::min<int64_t>(Hd, (int64_t)(ty + 1) * TH), x1 = std::min<int64_t>(Wd, (int64_t)(tx + 1) * TW);
      for (int64_t y = (int64_t)ty * TH; y < y1; ++y)
        for (int64_t x = (int64_t)tx * TW; x < x1; ++x) {
          const int ix = mx2[(size_t)(y * Wd + x)], iy = my2[(size_t)(y * Wd + x)];
          if (!inside(ix, iy)) continue;
          xlo = std::min(xlo, ix); xhi = std::max(xhi, ix + 1); ylo = std::min(ylo, iy); yhi = std::max(yhi, iy + 1);
        }
      if (xlo > xhi) continue;                                // nothing of the tile inside the image: an empty box
      const int bx0 = xlo >= 0 ? xlo / 4 * 4 : -4, bw = (xhi - bx0 + 1 + 3) / 4 * 4, bh = yhi - ylo + 1;
      if ((int64_t)bw * bh > 16000) return LSPIV_OK;          // this tile reads too wide a piece of the image (four boxes + 16 bytes must fit 64 KB of LDS): two passes
      cap = std::max(cap, bw * bh);
      int* t = &tiles[((size_t)ty * tiles_x + tx) * 4];
      t[0] = bx0; t[1] = ylo; t[2] = bw; t[3] = bh;
      for (int64_t y = (int64_t)ty * TH; y < y1; ++y)
        for (int64_t x = (int64_t)tx * TW; x < x1; ++x) {
          const size_t o = (size_t)(y * Wd + x);
          const int ix = mx2[o], iy = my2[o];
          if (!inside(ix, iy)) continue;
          const uint32_t fr = mf2[o], fx = fr & 31u, fy = fr >> 5;
          pxd[o] = (uint32_t)((iy - ylo) * bw + (ix - bx0)) | (fx << 16) | (fy << 21);
        }
    }
  cap = (cap + 15) / 16 * 16;
  if (getenv("LSPIV_PROJECT_DEBUG"))
    fprintf(stderr, "lspiv project_cv fused plan: %d x %d tiles, largest box %d bytes, %zu of %zu undistortion quads per pixel\n", tiles_x,
            tiles_y, cap, n_slow, nq);
  int* d_tiles = nullptr;
  int rc = upload_new(&h->d_fqb, qb.data(), nq);
  if (!rc) rc = upload_new(&h->d_fqd, qd.data(), nq);
  if (!rc) rc = upload_new(&h->d_fpx, pxd.data(), pxd.size());
  if (!rc) rc = upload_new(&d_tiles, tiles.data(), tiles.size());
  h->d_ft = d_tiles;
  if (rc) return rc;
  h->f_tiles = tiles_x * tiles_y; h->f_tiles_x = tiles_x; h->f_cap = cap;
  return LSPIV_OK;
}
}  // namespace

int lspiv_project_cv_create(int64_t src_h, int64_t src_w, int64_t dst_h, int64_t dst_w, const double* camera_matrix,
                            const double* dist_coeffs, int n_dist, const double* M, lspiv_remap** handle) {
  if (!handle || !M) return fail(LSPIV_EINVAL, "NULL argument");
  if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || src_h * src_w >= (int64_t)1 << 31 || dst_h * dst_w >= (int64_t)1 << 31)
    return fail(LSPIV_ESHAPE, "bad projection shape");
  if (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8)
    return fail(LSPIV_EINVAL, "dist_coeffs must hold 0, 4, 5 or 8 values (k1 k2 p1 p2 [k3 [k4 k5 k6]]), got %d", n_dist);
  if (n_dist > 0 && (!dist_coeffs || !camera_matrix)) return fail(LSPIV_EINVAL, "distortion coefficients need a camera matrix");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  lspiv_remap* h = new lspiv_remap();
  h->src_h = src_h; h->src_w = src_w; h->dst_h = dst_h; h->dst_w = dst_w;
  h->undistort = camera_matrix != nullptr;
  std::vector<int> mx1, my1;                 // the undistortion map, kept for the fused plan
  std::vector<uint16_t> mf1;
  if (h->undistort) {
    // initUndistortRectifyMap(K, dist, R = I, newK = K, size, CV_16SC2): the row walk _x += ir[0] included
    double ir[9];
    if (!invert3(camera_matrix, ir)) { delete h; return fail(LSPIV_EINVAL, "camera matrix is singular"); }
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n_dist; ++i) k[i] = dist_coeffs[i];
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double fx = camera_matrix[0], fy = camera_matrix[4], u0 = camera_matrix[2], v0 = camera_matrix[5];
    const size_t n = (size_t)(src_h * src_w);
    std::vector<int> mx(n), my(n);
    std::vector<uint16_t> mf(n);
    for (int64_t i = 0; i < src_h; ++i) {
      double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
      for (int64_t j = 0; j < src_w; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double w = 1.0 / _w, x = _x * w, y = _y * w;
        const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2), yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
        const int64_t iu = cv_round((fx * xd + u0) * 32.0), iv = cv_round((fy * yd + v0) * 32.0);
        const size_t o = (size_t)(i * src_w + j);
        mx[o] = clamp_short(iu >> 5); my[o] = clamp_short(iv >> 5);
        mf[o] = (uint16_t)((iv & 31) * 32 + (iu & 31));
      }
    }
    int rc = upload_map(mx, my, mf, &h->d_mx1, &h->d_my1, &h->d_mf1);
    if (!rc) rc = build_remap_quads(mx, my, mf, src_h, src_w, &h->d_qb1, &h->d_qd1, &h->d_slow1, &h->n_slow1);
    if (rc) { lspiv_project_cv_destroy(h); return rc; }
    mx1.swap(mx); my1.swap(my); mf1.swap(mf);
  }
  {
    // cv2.warpPerspective(src, M, (dst_w, dst_h), INTER_AREA -> INTER_LINEAR): M is inverted, 64-pixel column blocks
    double Mi[9];
    if (!invert3(M, Mi)) { lspiv_project_cv_destroy(h); return fail(LSPIV_EINVAL, "homography is singular"); }
    const size_t n = (size_t)(dst_h * dst_w);
    std::vector<int> mx(n), my(n);
    std::vector<uint16_t> mf(n);
    for (int64_t y = 0; y < dst_h; ++y)
      for (int64_t xb = 0; xb < dst_w; xb += 64) {
        const double X0 = Mi[0] * xb + Mi[1] * y + Mi[2], Y0 = Mi[3] * xb + Mi[4] * y + Mi[5], W0 = Mi[6] * xb + Mi[7] * y + Mi[8];
        for (int64_t x1 = 0; x1 < 64 && xb + x1 < dst_w; ++x1) {
          double W = W0 + Mi[6] * x1;
          W = W != 0.0 ? 32.0 / W : 0.0;
          const double fX = std::max(-2147483648.0, std::min(2147483647.0, (X0 + Mi[0] * x1) * W));
          const double fY = std::max(-2147483648.0, std::min(2147483647.0, (Y0 + Mi[3] * x1) * W));
          const int64_t X = cv_round(fX), Y = cv_round(fY);
          const size_t o = (size_t)(y * dst_w + xb + x1);
          mx[o] = clamp_short(X >> 5); my[o] = clamp_short(Y >> 5);
          mf[o] = (uint16_t)((Y & 31) * 32 + (X & 31));
        }
      }
    int rc = upload_map(mx, my, mf, &h->d_mx2, &h->d_my2, &h->d_mf2);
    if (!rc) rc = build_remap_quads(mx, my, mf, src_h, src_w, &h->d_qb2, &h->d_qd2, &h->d_slow2, &h->n_slow2);
    if (!rc && h->undistort) rc = build_remap_fused(h, mx1, my1, mf1, mx, my, mf);
    if (rc) { lspiv_project_cv_destroy(h); return rc; }
  }
  *handle = h;
  return LSPIV_OK;
}

int lspiv_project_cv_frames_dev(lspiv_remap* h, const void* d_frames, int dtype, int64_t T, void* d_out, void* stream) {
  if (!h || !d_frames || !d_out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype != LSPIV_U8 && dtype != LSPIV_F32) return fail(LSPIV_EINVAL, "project_cv takes uint8 or float32 frames (cv2 keeps the frame dtype)");
  if (T < 0 || T >= (int64_t)1 << 28) return fail(LSPIV_ESHAPE, "bad frame count");
  DeviceCtx* c;
  LSPIV_TRY(get_ctx(&c));
  hipStream_t s = on_stream(c, stream);
  const int64_t n_src = h->src_h * h->src_w, n_dst = h->dst_h * h->dst_w;
  const void* src = d_frames;
  hipError_t e;
  if (dtype == LSPIV_U8 && h->undistort && h->d_ft && ((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_frames)) & 3) == 0) {   // both remaps in one kernel
    e = lspiv::launch_remap_fused((const uint8_t*)d_frames, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_ft, h->f_tiles, h->f_tiles_x,
                                  h->f_cap, h->d_fpx, h->d_fqb, h->d_fqd, h->d_mx1, h->d_my1, h->d_mf1, (uint8_t*)d_out, (int)h->dst_h,
                                  (int)h->dst_w, s);
    return launch_status(e);
  }
  if (dtype == LSPIV_F32 && h->undistort && h->d_ft && ((reinterpret_cast<uintptr_t>(d_out) & 15) | (reinterpret_cast<uintptr_t>(d_frames) & 3)) == 0) {
    e = lspiv::launch_remap_fused_f32((const float*)d_frames, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_ft, h->f_tiles, h->f_tiles_x,
                                      h->f_cap, h->d_fpx, h->d_mx1, h->d_my1, h->d_mf1, (float*)d_out, (int)h->dst_h, (int)h->dst_w, s);
    return launch_status(e);
  }
  if (h->undistort) {
    LSPIV_TRY(ensure(&h->d_tmp, &h->tmp_cap, (size_t)T * n_src * elem_size(dtype)));
    if (dtype == LSPIV_U8 && h->d_qd1)
      e = lspiv::launch_remap_win((const uint8_t*)d_frames, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_qb1, h->d_qd1, h->d_slow1,
                                  h->n_slow1, h->d_mx1, h->d_my1, h->d_mf1, (uint8_t*)h->d_tmp, (int)n_src, s);
    else
      e = lspiv::launch_remap(d_frames, dtype, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_mx1, h->d_my1, h->d_mf1, h->d_tmp, (int)n_src, s);
    LSPIV_TRY(launch_status(e));
    src = h->d_tmp;
  }
  if (dtype == LSPIV_U8 && h->d_qd2 && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0)
    e = lspiv::launch_remap_win((const uint8_t*)src, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_qb2, h->d_qd2, h->d_slow2, h->n_slow2,
                                h->d_mx2, h->d_my2, h->d_mf2, (uint8_t*)d_out, (int)n_dst, s);
  else
    e = lspiv::launch_remap(src, dtype, n_src, (int)h->src_h, (int)h->src_w, (int)T, h->d_mx2, h->d_my2, h->d_mf2, d_out, (int)n_dst, s);
  return launch_status(e);
}

int lspiv_project_cv_frames(lspiv_remap* h, const void* frames, int dtype, int64_t T, void* out) {
  if (!h || !frames || !out) return fail(LSPIV_EINVAL, "NULL argument");
  if (dtype != LSPIV_U8 && dtype != LSPIV_F32) return fail(LSPIV_EINVAL, "project_cv takes uint8 or float32 frames (cv2 keeps the frame dtype)");
  if (T <= 0) return LSPIV_OK;
  const size_t fb = (size_t)T * h->src_h * h->src_w * elem_size(dtype), ob = (size_t)T * h->dst_h * h->dst_w * elem_size(dtype);
  std::lock_guard<std::mutex> handle_lock(h->host_mu);
  return project_host(fb, ob, frames, out, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_project_cv_frames_dev(h, d_in, dtype, T, d_out, s);
  });
}

int lspiv_project_cv_destroy(lspiv_remap* h) {
  if (!h) return LSPIV_OK;
  for (void* p : {(void*)h->d_mx1, (void*)h->d_my1, (void*)h->d_mf1, (void*)h->d_mx2, (void*)h->d_my2, (void*)h->d_mf2, h->d_tmp,
                  (void*)h->d_qb1, (void*)h->d_qb2, (void*)h->d_qd1, (void*)h->d_qd2, (void*)h->d_slow1, (void*)h->d_slow2,
                  h->d_ft, (void*)h->d_fpx, (void*)h->d_fqb, (void*)h->d_fqd})
    if (p) hipFree(p);
  delete h;
  return LSPIV_OK;
}

int lspiv_pack_int16_dev(const float* d_values, int64_t n, float scale, int fill, int16_t* d_packed, void* stream) {
  if (!d_values || !d_packed) return fail(LSPIV_EINVAL, "NULL argument");
  if (n < 0 || !(scale > 0.0f) || fill < -32768 || fill > 32767) return fail(LSPIV_EINVAL, "bad argument");
  return launch_on(stream, [&](hipStream_t s) { return lspiv::launch_pack_int16(d_values, n, scale, fill, d_packed, s); });
}

int lspiv_pack_int16(const float* values, int64_t n, float scale, int fill, int16_t* packed) {
  if (!values || !packed) return fail(LSPIV_EINVAL, "NULL argument");
  if (n <= 0) return n == 0 ? LSPIV_OK : fail(LSPIV_EINVAL, "bad n");
  return host_roundtrip(__func__, {values, (size_t)n * sizeof(float)}, {packed, (size_t)n * sizeof(int16_t)}, [&](void* d_in, void* d_out, hipStream_t s) {
    return lspiv_pack_int16_dev((const float*)d_in, n, scale, fill, (int16_t*)d_out, s);
  });
}

}  // extern "C"
