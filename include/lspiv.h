/*
 * lspiv.h -- C ABI of liblspiv_hip.so, the MI355X (gfx950) LSPIV cross-correlation engine.
 *
 * This is the drop-in boundary for the hot path behind pyorc's Frames.get_piv().  The
 * reference has no native boundary at all: the seam is the Python-level `engine` string
 * (pyorc/api/frames.py:118,176-177) that is forwarded to pyorc/velocimetry/ffpiv.py and
 * from there to six symbols of the third-party `ffpiv` package.  Every entry point below
 * names the reference call it replaces.  INTEGRATION.md shows the ctypes binding and the
 * five-line patch a pyorc maintainer would add.
 *
 * Conventions
 *   - plain C types only; all arrays are C-contiguous, caller-allocated, never retained;
 *   - frames are (T, H, W) of dtype LSPIV_U8 / LSPIV_F32 / LSPIV_F64; a stack of T frames
 *     holds P = T-1 pairs (pair p = frames p and p+1, labelled with frame p+1's time stamp,
 *     pyorc/velocimetry/ffpiv.py:403);
 *   - window index is row-major k*n_cols+m (pyorc/velocimetry/ffpiv.py:469);
 *   - every function returns LSPIV_OK (0) or a negative status; lspiv_last_error() returns
 *     the thread-local message of the last failure on this thread;
 *   - "_dev" variants take DEVICE pointers (HBM-resident stacks, multi-GPU shards) and a
 *     stream handle (NULL = the library's own per-device stream); host variants stage
 *     through pinned buffers and synchronise before returning.  The library's stream is
 *     NON-BLOCKING (it does not synchronise with the NULL stream): device data handed to a
 *     "_dev" call must already be complete, or the call must be given the stream that
 *     produces it; lspiv_memcpy_h2d / _d2h / lspiv_memset_dev run on the library's stream and
 *     wait for it.  "_dev" calls that need temporaries (normalize) share one scratch buffer
 *     per device: calls that overlap in time must be issued on one stream;
 *   - NaN conventions follow the reference: skipped / invalid windows yield NaN, never an
 *     error (pyorc/velocimetry/ffpiv.py:93-97,465-466).
 */
#ifndef LSPIV_H
#define LSPIV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSPIV_ABI_VERSION 5   /* (additions since, nothing existing moved, no version change: the search-area entry points lspiv_piv_search_pairs_at /
                               * lspiv_piv_search_pairs_dev_at and lspiv_search_supported; the sliding ensemble, lspiv_ensemble_set_sliding /
                               * lspiv_ensemble_sliding_reserve / lspiv_ensemble_sliding_finish; the multi-pass ensemble, lspiv_ensemble_set_shift /
                               * _set_shift_dev / _get_shift; multi-pass PIV, lspiv_shift_supported /
                               * lspiv_piv_shift_pairs_dev_at / lspiv_piv_predict_shift_dev / lspiv_piv_multipass_dev_at / lspiv_piv_multipass_at; window deformation passes,
                               * lspiv_deform_supported / lspiv_deform_required_bytes / lspiv_piv_predict_deform_dev /
                               * lspiv_piv_deform_pairs_dev_at / lspiv_piv_multipass_deform_dev_at / lspiv_piv_multipass_deform_at; SPOF phase-filtered
                               * correlation, lspiv_spof_supported / lspiv_piv_spof_pairs_dev_at / lspiv_piv_spof_pairs_at /
                               * lspiv_ensemble_set_spectral_filter / _get_spectral_filter; the image mask, lspiv_mask_supported /
                               * lspiv_piv_masked_pairs_dev_at / lspiv_piv_masked_pairs_at; the second correlation peak, lspiv_peak2_supported /
                               * lspiv_piv_peak2_pairs_dev_at / lspiv_piv_peak2_pairs_at / lspiv_second_peak_dev / lspiv_second_peak; vector validation,
                               * lspiv_validate_dev / lspiv_validate; the per-window frame lag, lspiv_lag_supported /
                               * lspiv_piv_lag_pairs_dev_at / lspiv_piv_lag_pairs_at / lspiv_lag_predict_dev / lspiv_lag_predict; frame stabilisation,
                               * lspiv_stabilize_fit[_dev] / lspiv_stabilize_chain[_dev] / lspiv_warp_affine[_dev]; space-time image
                               * velocimetry, lspiv_sti_gather[_dev] / lspiv_sti_orientation[_dev]; pyramidal Lucas-Kanade point tracking,
                               * lspiv_pyr_down[_dev] / lspiv_lk_track[_dev])
                               * 5 (round 6): lspiv_chunk_alignment(wy, wx) without a grid now returns the alignment that is right on EVERY grid (75
                               * where it returned 25: callers that cut chunks on it stay bit-reproducible on large grids); additions:
                               * lspiv_upload_frames, lspiv_trace / lspiv_trace_read; the host-pointer projection entry points no longer
                               * share the PIV host entry points' lock and workspaces.
                               * (round 5 added lspiv_chunk_alignment_grid, lspiv_piv_velocity_at, lspiv_ensemble_flag_digest, lspiv_kernel_times + the "time_kernel" option and the test hook lspiv_debug_hold_lock; no version change: nothing existing moved)
                               * 4 (round 4, additions only): lspiv_build_info, the float64 rescue of the ensemble's final fit
                               * (lspiv_ensemble_set_retain / _stats / _flag / _partials / _finish_partials), lspiv_stream_release,
                               * lspiv_stream_create_priority; 3: lspiv_rescue_stats,
                               * lspiv_project_frames_u8[_dev], the rescue / v_sign / norm_clip / std_ddof / round_odd options */

/* status codes (mapped by the Python shim onto the reference's exception types) */
#define LSPIV_OK            0
#define LSPIV_EINVAL       -1  /* bad argument                      -> ValueError    */
#define LSPIV_ESHAPE       -2  /* frame smaller than window, T < 2  -> ValueError    */
#define LSPIV_ENOMEM       -3  /* HBM / pinned allocation failed    -> MemoryError   */
#define LSPIV_EHIP         -4  /* HIP runtime error                 -> RuntimeError  */
#define LSPIV_ENODEV       -5  /* no gfx950 device visible          -> RuntimeError  */
#define LSPIV_EUNSUPPORTED -6  /* window size outside kernel range  -> ValueError    */

/* frame dtypes (pyorc frame stacks are uint8 after normalize/project_cv, float32 after
 * edge_detect/smooth/time_diff, float64 out of project_numpy) */
#define LSPIV_U8  0
#define LSPIV_F32 1
#define LSPIV_F64 2

/* largest interrogation window side the kernels accept (ffpiv.cross_corr itself has no upper bound).  2..64:
 * register-resident kernels; above 64 (any parity, square or not, e.g. 96 x 96 and 128 x 128 for 4K footage): the
 * LDS-resident DFT kernel, as long as 2 wy wx floats fit the 160 KB of a CU -- 128 x 128 does; anything larger up to this
 * limit runs the same transforms on slots of HBM scratch: correct, an order of magnitude slower per sample. */
#define LSPIV_MAX_WINDOW 512

/* ---------------------------------------------------------------- library / device ------- */
int         lspiv_abi_version(void);
const char* lspiv_version(void);                        /* "lspiv-hip <version> (gfx950) src <source hash>" */
/* Provenance of the loaded binary (csrc/Makefile compiles both in): LSPIV_BUILD_KERNEL_HASH = first 16 hex digits of the
 * sha256 over csrc/{piv_fft_impl.h, fft_regs.h, common.h, piv_rescue.hip} (the fused PIV kernels; the committed profile
 * summaries are keyed to it), LSPIV_BUILD_SOURCE_HASH = the same over every .hip, .h and .cpp file of csrc/ (sorted by name) and this
 * header.  pyorc_amd._lib.load() recomputes the second from the tree and refuses a stale binary.  "unknown": not built by
 * csrc/Makefile; "": unknown selector. */
#define LSPIV_BUILD_KERNEL_HASH 0
#define LSPIV_BUILD_SOURCE_HASH 1
const char* lspiv_build_info(int what);
const char* lspiv_last_error(void);
int         lspiv_device_count(int* n);                 /* 0 devices is LSPIV_OK with *n = 0 */
int         lspiv_set_device(int device);               /* per calling thread               */
int         lspiv_get_device(int* device);
int         lspiv_device_name(int device, char* buf, size_t len);
int         lspiv_synchronize(void);                    /* hipDeviceSynchronize             */
/* run-time options: "walk" = 1 the default time-walking kernels (segments anchored every lspiv_chunk_alignment pairs of
 * the absolute pair index: results do not depend on the chunking as long as chunks start on such anchors), 0 per-pair
 * kernels (independent of any chunking, ~23 % slower), n > 1 anchor length n, -1 back to the LSPIV_WALK environment
 * variable.
 * Three engine semantics could not be pinned on a real ffpiv run (ffpiv is absent from /root/reference, SURVEY.md
 * section 8c A5 / A7); each is an option whose default is the oracle's reading, so that matching a real ffpiv is a
 * one-line default flip (environment presets: LSPIV_BORDER_PEAK, LSPIV_SIGNAL_MODE, LSPIV_SIGNAL_POSITIVE):
 *   "border_peak"      arg-max of a correlation plane on the plane border (no 3-point fit possible): 0 u = v = NaN
 *                      (default), 1 the plane centre, i.e. zero displacement (OpenPIV's scalar routine), 2 the integer peak;
 *   "signal_mode"      signal_threshold (pyorc/velocimetry/ffpiv.py:93-97) scores 0 each window PAIR: both windows need
 *                      the fraction (default; CHANGELOG 0.9.5 "any of the 2 interrogation window in a window pair"), 1 each
 *                      window POSITION over all frames of the chunk ("fraction of non-zero pixels in the window stack");
 *   "signal_positive"  the score counts 0 samples != 0 ("non-zero pixels", default), 1 samples > 0 ("above zero"). */
/* Four more readings became switches in round 3 (environment presets LSPIV_V_SIGN, LSPIV_NORM_CLIP, LSPIV_STD_DDOF,
 * LSPIV_ROUND_ODD), so that a run of the real ffpiv (tests/golden/regen_from_ffpiv.py) can only end in "combination X matches":
 *   "v_sign"           0 v = row shift of the correlation peak, positive down the image (default; pyorc/api/plot.py:548,576-583
 *                      flips it for plotting only), 1 negated inside the engine;
 *   "norm_clip"        1 the normalised window is clipped at zero (default, A3), 0 plain (a - mean) / std -- served by the
 *                      block-per-window kernels (kinds 3 / 9 / 10), not by the fused FFT kernels;
 *   "std_ddof"         0 population standard deviation in the window normalisation (default), 1 sample (n - 1);
 *   "round_odd"        ffpiv.window.round_to_even for odd sizes (pyorc/api/frames.py:167): 0 half-even of x / 2 (25 -> 24, 27 -> 28;
 *                      default), 1 up (25 -> 26), 2 down (27 -> 26); host side -- pyorc_amd.window.round_to_even reads it. */
/* Float64 rescue pass (round 3): the reference fits EVERY correlation plane in its engine's precision
 * (pyorc/velocimetry/ffpiv.py:465-471); a float32 plane carries ~1e-7 of noise, which the 3-point log fit amplifies beyond
 * 1e-4 on ill-conditioned peaks (a neighbour that is exactly zero, a flat ridge, a tie for the maximum).  The kernels flag
 * those windows and a second kernel re-evaluates them from the frames in float64, overwriting u and v:
 *   "rescue"           1 (default; environment LSPIV_RESCUE) | 0 float32 results as they are;
 *   "rescue_kappa"     plane noise the flag model assumes, in 1e-9 of the plane maximum (default 500);
 *   "rescue_tau"       relative gap between the two largest samples below which the arg-max counts as ambiguous and the whole
 *                      plane is re-evaluated, in 1e-9 (default 4000);
 *   "rescue_generic"   0 (default; environment LSPIV_RESCUE_GENERIC) square 16 / 32 / 64 px windows without a search area take fit
 *                      kernels with the window size known at compile time | 1 every launch takes the run-time-geometry
 *                      kernel.  The results are the same bit for bit; 1 is the reference of that claim
 *                      (tests/test_gpu_rescue_fixed_size.py);
 *   "rescue_fit_size"  read-only (lspiv_get_option): the compile-time window size of the fit kernel the last rescue pass of the
 *                      process launched, 0 the run-time-geometry kernel, -1 no pass yet.  For tests of the dispatch.
 * Planes with no frames behind them -- lspiv_u_v_displacement, and lspiv_ensemble_finish / lspiv_ensemble_sliding_finish on a sum whose
 * frames are not all at hand (an imported state, a chunk that could not be retained) -- have nothing to be re-evaluated from and need
 * nothing: their float32 samples are the input, only the float32 arithmetic of the fit errs.  With "rescue" = 1 the windows the flag
 * model marks get the 3-point fit of their five samples in float64 instead; the others keep the bits of the float32 fit.
 * lspiv_ensemble_stats still counts them as flagged and left without a re-evaluation from the frames.
 *   "peaks_refitted"   read-only: the planes the last lspiv_u_v_displacement of the process fitted in float64.
 * Batched sub-pixel fit of the 32 x 32 time-walking kernels:
 *   "defer_fit"        1 (default; environment LSPIV_DEFER_FIT) an iteration stops after the arg-max search and the peak's samples, and
 *                      after every 16th iteration each lane of a window's lane group fits one of the 32 staged planes | 0 every plane is
 *                      fitted inside its own iteration.  The same expressions on the same operands: results and rescue records are
 *                      the same bit for bit (tests/test_gpu_walk_defer.py); float64 frames with a signal threshold run the 0 form
 *                      either way.
 * Un-packing of the 32 x 32 time-walking kernels (per frame pair):
 *   "unpack_dpp"       1 (default; environment LSPIV_UNPACK_DPP_OPT) between its two transposes an iteration keeps the columns kx and -kx
 *                      in adjacent lanes and exchanges them through DPP | 0 columns in natural order, exchanged through LDS
 *                      (ds_bpermute).  The same expressions on the same operands: results and rescue records are the same bit for
 *                      bit (tests/test_gpu_unpack_dpp.py).
 * Cross-row reductions and un-pack lane masks of the 32 x 32 time-walking kernels (per frame pair):
 *   "lds_light"        1 (default; environment LSPIV_LDS_LIGHT) the 32-lane reductions of an iteration join their two 16-lane rows with
 *                      v_permlane16_swap, the integer ones that come in pairs in one chain | 0 the rows are joined through LDS
 *                      (ds_swizzle).  Only on top of "unpack_dpp" = 1 and
 *                      "defer_fit" = 1; ignored otherwise.  Results and rescue records are the same bit for bit
 *                      (tests/test_gpu_lds_light.py).
 * Group-uniform work of the peak search of the 32 x 32 time-walking kernels (per frame pair):
 *   "scalar_epilogue"  1 (default; environment LSPIV_SCALAR_EPILOGUE) the first-match searches for the peak's row and column, the
 *                      near-tie test, the wrapped neighbour indices and the record word of a plane are taken from ballots on the
 *                      scalar unit, one value per 32-lane group | 0 they are computed 64 lanes wide in vector registers.  Only on
 *                      top of "lds_light" = 1 where that applies; ignored otherwise.  Integer first-match and index arithmetic:
 *                      results and rescue records are the same bit for bit (tests/test_gpu_scalar_epilogue.py).
 * float64 HOST stacks are narrowed to float32 while they are staged (the kernels compute in float32).  A frame that rides on a
 * DC offset far above its contrast would lose the low bits of its texture in that conversion, where the reference normalises
 * every window in float64; the per-window normalisation does not see a constant added to a frame, so:
 *   "narrow_offset"    smallest magnitude of a frame's DC offset (the mean of 4096 strided samples, rounded to an integer: a
 *                      function of the frame alone) that is subtracted while narrowing; default 1024 (never triggers on 8-bit-like
 *                      imagery, whose results stay bit-identical to a float32 copy of the stack), -1 never; environment
 *                      LSPIV_NARROW_OFFSET.  lspiv_piv_pairs / lspiv_ensemble_accumulate only, and only without a signal
 *                      threshold (which counts samples != 0).  float64 stacks already in HBM ("_dev") are converted as they are, except by the
 *                      search-area kernels, which take a float64 sample of the window off before they convert. */
int         lspiv_set_option(const char* name, int value);
int         lspiv_get_option(const char* name, int* value);
/* counters of the rescue pass on `stream` (NULL: the library's own stream), after synchronising with it: stats[0..4] =
 * "fit" / "amb" windows of the last launch, the same two summed over all launches, windows processed by all launches */
int         lspiv_rescue_stats(void* stream, int64_t* stats);
/* which kernel a window size dispatches to: 1 = FFT 32x32, 2 = FFT 64x64, 6 = FFT 8x8 / 16x16, 8 = prime-factor FFT
 * kernels (every other even square window 6..62), 7 / 4 / 5 = odd square windows (and 4x4) 4..7 / 9..15 / 21..31
 * embedded in the 16- / 32- / 64-point FFT kernels, 3 = direct spatial correlation (non-square and odd 17 / 19 / 33..63
 * windows of fewer than 1500 samples), 9 = LDS-resident 2-D transform (any window with a side above 64, and the non-square /
 * odd ones from 1500 samples on), 10 = the same transforms on HBM scratch (windows that outgrow the LDS of a CU: a side
 * above 128); <0 = unsupported.  Host-only. */
int         lspiv_kernel_kind(int wy, int wx);

/* ---------------------------------------------------------------- window grid (host) ----- */
/* replaces ffpiv.window.get_rect_coordinates (pyorc/api/frames.py:85-90) and the implied
 * ffpiv.window.get_axis_shape: n = (dim - win)//(win - overlap) + 1, centres
 * arange(n)*(win-overlap) + win/2 as integer pixel indices. */
int lspiv_grid_shape(int64_t H, int64_t W, int wy, int wx, int oy, int ox, int64_t* n_rows, int64_t* n_cols);
int lspiv_grid_coords(int64_t H, int64_t W, int wy, int wx, int oy, int ox,
                      int64_t* rows /* n_rows */, int64_t* cols /* n_cols */);

/* ---------------------------------------------------------------- memory planner --------- */
/* replaces ffpiv.window.required_memory / available_memory (pyorc/velocimetry/ffpiv.py:120-129):
 * device bytes one call on T frames needs (frames + results [+ planes]); free/total HBM. */
int64_t lspiv_required_bytes(int64_t T, int64_t H, int64_t W, int dtype, int wy, int wx, int oy, int ox,
                             int with_planes);
int     lspiv_available_bytes(int64_t* free_bytes, int64_t* total_bytes);

/* ---------------------------------------------------------------- the hot path ----------- */
/* One fused call per frame chunk: replaces ffpiv.cross_corr + the corr_max / s2n reductions +
 * ffpiv.u_v_displacement of pyorc/velocimetry/ffpiv.py:446-474 (_get_uv_timestep).
 *   u, v          displacement in PIXELS (u = column shift, v = row shift, no sign flip)
 *   corr_max      nanmax of the clipped correlation plane
 *   s2n           corr_max / nanmean(plane)
 *   each (T-1) * n_rows * n_cols float32.
 *   corr_planes   NULL, or (T-1) * n_win * wy * wx float32: the fft-shifted, clipped planes that
 *                 ffpiv.cross_corr returns (NaN planes for windows below signal_threshold).
 *   signal_threshold < 0 disables the pre-mask (reference: None).                           */
int lspiv_piv_pairs(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                    int wy, int wx, int oy, int ox, float signal_threshold,
                    float* u, float* v, float* corr_max, float* s2n, float* corr_planes);

/* same on device-resident data.  d_out is 4 planes [u | v | corr_max | s2n], each
 * (T-1)*n_win float32, contiguous (so one all-gather moves a rank's whole result block).    */
int lspiv_piv_pairs_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                        int wy, int wx, int oy, int ox, float signal_threshold,
                        float* d_out, float* d_corr_planes, void* stream);

/* Chunked callers (the time-chunk loop of pyorc/velocimetry/ffpiv.py:140,399-442; multi-GPU time blocks): the same two
 * calls on a chunk whose first pair has index `pair_offset` in the caller's whole stack.  The reference computes every
 * window independently, so its results cannot depend on the chunking; the default kernels here share transforms between
 * consecutive pairs of a window in runs that start at multiples of lspiv_chunk_alignment() of the ABSOLUTE pair index.
 * Chunks that start on such a multiple therefore reproduce, bit for bit, what one call over the whole stack returns
 * (tested); a chunk that starts elsewhere is still correct but its first (alignment - offset % alignment) pairs may
 * differ from the whole-stack run in the last float32 bit.  lspiv_piv_pairs[_dev] == these with pair_offset 0.
 * lspiv_chunk_alignment: pairs; 1 for window sizes served by per-pair kernels and with option "walk" = 0.  Host-only.
 * Round 5: the run length depends on the window GRID as well -- 25 pairs, or 75 on grids with at least as many windows as the chip
 * has lane groups for that window family (1080p 32 x 32 @ 50 %, 64 x 64 @ 75 %, 4K: less per-segment overhead, csrc/common.h
 * walk_anchor).  lspiv_chunk_alignment_grid(H, W, ...) is the figure to cut chunks on for frames of that shape; negative status for
 * a bad shape.  lspiv_chunk_alignment(wy, wx), without a grid, is the alignment that is right for EVERY frame shape (ABI 5: the
 * longest run length of the family, a multiple of every grid's; ABI 4 returned the run length of small grids). */
int lspiv_chunk_alignment(int wy, int wx);
int lspiv_chunk_alignment_grid(int64_t H, int64_t W, int wy, int wx, int oy, int ox);
int lspiv_piv_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                       int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                       float* u, float* v, float* corr_max, float* s2n, float* corr_planes);
int lspiv_piv_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                           int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                           float* d_out, float* d_corr_planes, void* stream);
/* lspiv_piv_pairs_at with the per-chunk scaling of _get_ffpiv_timestep (pyorc/velocimetry/ffpiv.py:418-419) applied on the device
 * before the results cross PCIe (round 5): v_x = (u * res_x / dt[pair]).astype(float32), v_y likewise -- the product in float32 (what
 * numpy computes for a float32 array times a Python float), the division in float64, one rounding; dt: seconds per pair, T - 1
 * doubles.  The Python mirror uses it when the resolutions are Python floats (pyorc: camera_config.resolution) and keeps numpy's own
 * arithmetic for anything else. */
int lspiv_piv_velocity_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                          int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                          double res_x, double res_y, const double* dt,
                          float* v_x, float* v_y, float* corr_max, float* s2n);

/* Extended search area: an interrogation window wy x wx of frame t searched inside a LARGER search area say x sax of frame t+1
 * (ffpiv.cross_corr's search_area_size != window_size).  This project's reading (ffpiv's own is unknown: unpinned like the rest of
 * the PIV path): the grid is that of the search area -- tiles of say x sax anchored top-left, step search area -
 * overlap, so oy, ox are relative to the search area --; per tile and pair B = the tile of frame t+1 normalised over its say sax
 * samples, a = the central wy x wx block of the tile of frame t (offset (say - wy) / 2) normalised over its own samples and placed
 * at that offset in a tile of zeros; plane = clip(fftshift(irfft2(conj(rfft2 A) rfft2 B)) / (wy wx), 0, 1), say x sax samples, zero
 * displacement at its centre; corr_max, s2n, u, v from that plane as in lspiv_piv_pairs.  corr_planes: (T-1) * n_win * say * sax.  The
 * signal threshold scores a over wy wx samples and B over say sax.  Supported (lspiv_search_supported == 1, host-only): square search
 * areas 16, 32, 64 with a square even window 4 .. search area - 2; anything else, and option "norm_clip" = 0, is LSPIV_EUNSUPPORTED.
 * Per-pair kernels: results do not depend on the chunking (chunk alignment 1).  lspiv_required_bytes with the SEARCH AREA as its
 * window is the memory these calls need.  A displacement up to (search area - window) / 2 is measured without aliasing. */
int lspiv_search_supported(int say, int sax, int wy, int wx);
int lspiv_piv_search_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                              int say, int sax, int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                              float* u, float* v, float* corr_max, float* s2n, float* corr_planes);
int lspiv_piv_search_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                  int say, int sax, int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                                  float* d_out, float* d_corr_planes, void* stream);

/* Multi-pass PIV: a chain of passes (wy_k, wx_k, oy_k, ox_k), k = 0 .. K, square even windows, non-increasing; a coarse pass predicts the
 * displacement, each finer pass cuts its window of frame t+1 at an INTEGER offset from that prediction and measures the residual, the
 * full window against a full window (the project's own semantics, unpinned like the search area).  All
 * pass-to-pass arithmetic is in the kernels' orientation (u column shift, v row shift, rows downward); option "v_sign" is applied once,
 * to the final result.  Option "norm_clip" = 0 and "signal_mode" = 1 are LSPIV_EUNSUPPORTED in every entry point below.
 *
 * lspiv_shift_supported: 1 for wy = wx in {16, 32, 64} (the windows of passes k >= 1), else 0.  Host-only.
 *
 * lspiv_piv_shift_pairs_dev_at: ONE shifted pass.  d_shift: (T-1) * n_win * 2 int16 {dy, dx} per (pair, window) on the device, or NULL
 * (all zero).  Per window and pair: A = the window of frame t at its grid origin (y0, x0), B = the window of frame t+1 at (y0 + dy,
 * x0 + dx), the offset CLAMPED by the kernel to dy in [-y0, H - wy - y0], dx in [-x0, W - wx - x0] (no offset array reads outside the
 * stack); plane, corr_max, s2n as lspiv_piv_pairs computes them for the pair (A, B), the signal threshold scoring A and the shifted B;
 * u = clamped dx + residual u, v = clamped dy + residual v (float32 sums, a NaN residual stays NaN).  d_out, d_corr_planes as
 * lspiv_piv_pairs_dev_at.  Per-pair kernels, one window per job: a window's result depends on its own samples and offset alone, so
 * results do not depend on the chunking (pair_offset is accepted for symmetry).  Unsupported windows: LSPIV_EUNSUPPORTED.
 *
 * lspiv_piv_predict_shift_dev: the predictor between two passes.  d_u, d_v: n_pairs * coarse windows float32 (kernel orientation);
 * d_shift: n_pairs * fine windows * 2 int16 {dy, dx}.  Per pair: q = rint (half to even, float32) of every vector, clamped to the int16
 * range [-32768, 32767] (no displacement a frame can hold is touched), valid when u and v are finite (any finite float32); M2 = twice the median of q over the valid vectors of the 3 x 3 neighbourhood clipped at the grid's edges (even count: the
 * sum of the two middle values; none: 0), u and v separately; bilinear interpolation between the coarse window centres origin + w / 2 at
 * the fine centres, integer weights w1 = clamp(cf - cc[i0], 0, s), w0 = s - w1, i0 = clamp(floor((cf - cc[0]) / s), 0, count - 2)
 * (constant outside the outermost centres; a one-entry axis has w1 = 0); d = floor((2 num + den) / (2 den)), den = 2 s_y s_x; then the
 * frame clamp above.  Exact integer arithmetic after the rint.  Windows must be even; a frame side above 32767 is LSPIV_EINVAL.
 *
 * lspiv_piv_multipass_dev_at: the chain.  passes: n_passes * 4 ints {wy, wx, oy, ox} on the HOST, coarsest first; the last one is the
 * grid of the result.  Pass 0 is lspiv_piv_pairs_dev_at of its window (any window that serves; bit for bit, at the same pair_offset);
 * passes k >= 1 need lspiv_shift_supported.  d_out: 4 * (T-1) * n_win floats of the LAST pass's grid, [u | v | corr_max | s2n];
 * d_corr_planes: NULL or the last pass's planes; d_shift_out: NULL or the last pass's CLAMPED offsets, (T-1) * n_win * 2 int16.
 * n_passes = 1 is lspiv_piv_pairs_dev_at (d_shift_out: zeros).  Chunks cut on lspiv_chunk_alignment_grid of PASS 0 reproduce one
 * call bit for bit: every later pass is pair-local.  Intermediates live in a per-device workspace: one stream at a time.
 * lspiv_piv_multipass_at: the host-fed twin -- the chunk is staged like lspiv_piv_pairs_at stages it (float64 narrowed to float32),
 * the chain runs on it, results come back; shift_out: NULL or host int16. */
int lspiv_shift_supported(int wy, int wx);
int lspiv_piv_shift_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                 int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                                 const int16_t* d_shift, float* d_out, float* d_corr_planes, void* stream);
int lspiv_piv_predict_shift_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t H, int64_t W,
                                int cwy, int cwx, int coy, int cox, int fwy, int fwx, int foy, int fox,
                                int16_t* d_shift, void* stream);
int lspiv_piv_multipass_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                               int n_passes, const int* passes, float signal_threshold, int64_t pair_offset,
                               float* d_out, float* d_corr_planes, int16_t* d_shift_out, void* stream);
int lspiv_piv_multipass_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                           int n_passes, const int* passes, float signal_threshold, int64_t pair_offset,
                           float* u, float* v, float* corr_max, float* s2n, float* corr_planes, int16_t* shift_out);

/* Per-window frame lag, multi-frame PIV for slow flow (the project's own semantics, unpinned): pair t, window w
 * is correlated against frame t + k[t, w], k in 1 .. 16, and the displacement is divided by k -- the absolute error of a correlation peak
 * does not shrink with the displacement, so a window that moves 0.2 px per frame interval is measured four times better over four
 * intervals.  A = the window of frame t at its grid origin (y0, x0); B = the window of frame t + k at (y0 + dy, x0 + dx), the int16
 * offset clamped exactly as lspiv_piv_shift_pairs_dev_at clamps it; plane, corr_max, s2n, the first maximum, the three-point fit,
 * "border_peak" and the signal threshold are that entry point's.  u = (clamped dx + residual u) / k, v = (clamped dy + residual v) / k:
 * the float32 sum, then ONE correctly rounded float32 division by (float)k; a NaN stays NaN; "v_sign" last.  Velocities stay in px per
 * frame interval.  Kernel orientation throughout.  Option "norm_clip" = 0 and "signal_mode" = 1 are LSPIV_EUNSUPPORTED.
 *
 * lspiv_lag_supported: 1 for wy = wx in {16, 32, 64}, else 0.  Host-only.
 *
 * lspiv_piv_lag_pairs_dev_at: d_frames points at T frames AVAILABLE to this call; pairs 0 .. n_pairs - 1 of that pointer are computed,
 * 1 <= n_pairs <= T - 1.  The lag of pair t is clipped to T - 1 - t OF THIS CALL, so a caller that cuts a stack into chunks must hand
 * over, with every chunk, the frames up to min(last pair of the chunk + 16, end of the stack): then the clip is the one of the absolute
 * frame count and no chunking changes a result.  No lag reads past frame T - 1: the library writes the table the kernels read.
 * lag_form selects where the lags come from:
 *   LSPIV_LAG_UNIFORM   k[t, w] = min(k, T - 1 - t), k in 1 .. 16;
 *   LSPIV_LAG_WINDOW    d_lag: n_win bytes, one lag per window, values clamped to 1 .. 16, the same clip;
 *   LSPIV_LAG_TABLE     d_lag: n_pairs * n_win bytes, one lag per (pair, window), clamped and clipped likewise;
 *   LSPIV_LAG_ADAPTIVE  pass 0 is lspiv_piv_pairs_dev_at on the same grid at lag 1 (its bits, at the same pair_offset), then
 *                       lspiv_lag_predict_dev with k_max = k and target128 turns pair t's field into (k, dy, dx) per window; d_lag and
 *                       d_shift must be NULL.
 * d_shift: NULL (zero offsets) or n_pairs * n_win * 2 int16 {dy, dx}.  d_out: 4 * n_pairs * n_win floats [u | v | corr_max | s2n], laid
 * out as lspiv_piv_pairs_dev_at lays them out for n_pairs pairs; d_corr_planes: NULL or n_pairs * n_win * wy * wx floats; d_lag_out:
 * n_pairs * n_win bytes, REQUIRED -- the effective lags, and the table the kernels read; d_shift_out: NULL or n_pairs * n_win * 2 int16,
 * the clamped offsets (may be d_shift itself).  With every lag 1 and no offsets the result is lspiv_piv_shift_pairs_dev_at's without
 * offsets bit for bit (not lspiv_piv_pairs_dev_at's: that is another kernel).  One window per job: a window's result depends on its own
 * samples, lag and offset alone.  The adaptive form uses a per-device workspace: one stream at a time.
 * lspiv_piv_lag_pairs_at: the host-fed twin -- all T frames are staged like lspiv_piv_pairs_at stages them (float64 narrowed to
 * float32), lag / shift / lag_out / shift_out are host arrays of the same sizes (lag_out required, shift_out may be NULL).
 *
 * lspiv_lag_predict_dev: the lag predictor alone.  d_u, d_v: n_pairs * n_win float32 of a lag-1 pass on the grid (kernel orientation).
 * Per pair t and window: valid = u and v finite; q = rint(64 x) (float32: the product is exact, the rint half to even) clamped to
 * +-32767 * 64, for u and v; M2 = twice the median of q over the valid vectors of the 3 x 3 neighbourhood clipped at the grid's edges,
 * centre included (even count: the sum of the two middle values; none: 0), in 1 / 128 px; mag = max(|M2u|, |M2v|); k = clamp(floor(
 * target128 / max(mag, 1)), 1, k_max), then k = min(k, T - 1 - t); dx = floor((k M2u + 64) / 128), dy likewise; the frame clamp above.
 * target128 = rint(128 * target in px), 1 .. 64 * window.  Exact integer arithmetic after the rint.  d_lag: n_pairs * n_win bytes,
 * d_shift: n_pairs * n_win * 2 int16.  lspiv_lag_predict: the host-fed twin. */
#define LSPIV_LAG_UNIFORM 0
#define LSPIV_LAG_WINDOW 1
#define LSPIV_LAG_TABLE 2
#define LSPIV_LAG_ADAPTIVE 3
int lspiv_lag_supported(int wy, int wx);
int lspiv_piv_lag_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t n_pairs, int64_t H, int64_t W,
                               int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                               int lag_form, int k, int target128, const uint8_t* d_lag, const int16_t* d_shift,
                               float* d_out, float* d_corr_planes, uint8_t* d_lag_out, int16_t* d_shift_out, void* stream);
int lspiv_piv_lag_pairs_at(const void* frames, int dtype, int64_t T, int64_t n_pairs, int64_t H, int64_t W,
                           int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                           int lag_form, int k, int target128, const uint8_t* lag, const int16_t* shift,
                           float* u, float* v, float* corr_max, float* s2n, float* corr_planes, uint8_t* lag_out, int16_t* shift_out);
int lspiv_lag_predict_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t T, int64_t H, int64_t W,
                          int wy, int wx, int oy, int ox, int k_max, int target128, uint8_t* d_lag, int16_t* d_shift, void* stream);
int lspiv_lag_predict(const float* u, const float* v, int64_t n_pairs, int64_t T, int64_t H, int64_t W,
                      int wy, int wx, int oy, int ox, int k_max, int target128, uint8_t* lag, int16_t* shift);

/* Window deformation passes (the project's own semantics, unpinned): after a chain, D passes on the FINAL grid,
 * each between frame t and frame t+1 WARPED by the field of the pass before it at 1 / 64 px, so that the pass measures a residual of
 * sub-pixel size on windows whose inner velocity gradient is taken out.  Kernel orientation throughout; "v_sign" once, at the end.
 * Option "norm_clip" = 0 and "signal_mode" = 1 are LSPIV_EUNSUPPORTED.  Window: square, 16 / 32 / 64, the same overlap on both axes.
 *
 * lspiv_deform_supported: 1 for wy = wx in {16, 32, 64}, else 0.  Host-only.
 * lspiv_deform_required_bytes: the HBM a pass takes next to the frames and results: the warped frames of one batch of pairs + the nodes.
 *
 * lspiv_piv_predict_deform_dev: d_u, d_v n_pairs * n_rows * n_cols float32 -> d_nodes n_pairs * n_rows * n_cols * 2 int32 {v, u} in
 * 1 / 128 px on the same grid: q = rint(64 x) (float32, half to even) clamped to +-32767 * 64, valid when u and v are finite; node =
 * twice the median of q over the valid vectors of the 3 x 3 neighbourhood (the median of lspiv_piv_predict_shift_dev; none valid: 0).
 *
 * lspiv_piv_deform_pairs_dev_at: ONE pass.  Dense field at pixel (y, x), per component, exact integers on doubled coordinates: per axis
 * node i at c2[i] = 2 i s + n - 1, p2 = 2 y, S2 = 2 s, i0 = clamp(floor((p2 - c2[0]) / S2), 0, count - 2), w1 = clamp(p2 - c2[i0], 0, S2),
 * w0 = S2 - w1 (constant outside the outermost nodes; one node: w1 = 0); d64 = floor((num + den) / (2 den)), num = the four corners'
 * wy wx node, den = S2y S2x.  Warp: Y64 = clamp(64 y + dv64, 0, 64 (H - 1)), iy = Y64 >> 6, fy = Y64 & 63 (iy = H - 1: iy = H - 2, fy = 64),
 * x likewise; B'(y, x) = the four neighbours of frame t+1 weighted (64 - fy | fy) (64 - fx | fx) / 4096 -- exact in float32 for uint8
 * frames, a fixed order of unfused float32 products and sums otherwise (float64 samples narrowed first).  No field makes a read leave
 * the frame.  Then the plain per-pair result of (window of frame t, the same window of B'): plane, corr_max, s2n, the signal threshold
 * scoring both; u = float32(node.u) / 128 + residual u, v likewise (a NaN residual stays NaN).  d_nodes: (T-1) * n_win * 2 int32; d_out,
 * d_corr_planes as lspiv_piv_pairs_dev_at.  Pair-local: pair_offset is accepted for symmetry.  The pairs run in batches through a
 * per-device workspace: one stream at a time.
 *
 * lspiv_piv_multipass_deform_dev_at / _at: lspiv_piv_multipass_dev_at / _at followed by n_deform (0 .. 4) deformation passes on the last
 * pass's grid, each fed with the (u, v) of the pass before it through lspiv_piv_predict_deform_dev.  n_deform = 0 is the plain chain, bit
 * for bit; n_passes = 1 is allowed.  corr_max, s2n and planes are those of the last deformation pass; shift: the last CHAIN pass's. */
int lspiv_deform_supported(int wy, int wx);
int64_t lspiv_deform_required_bytes(int64_t T, int64_t H, int64_t W, int wy, int wx, int oy, int ox);
int lspiv_piv_predict_deform_dev(const float* d_u, const float* d_v, int64_t n_pairs, int64_t n_rows, int64_t n_cols,
                                 int32_t* d_nodes, void* stream);
int lspiv_piv_deform_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                  int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                                  const int32_t* d_nodes, float* d_out, float* d_corr_planes, void* stream);
int lspiv_piv_multipass_deform_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                      int n_passes, const int* passes, int n_deform, float signal_threshold, int64_t pair_offset,
                                      float* d_out, float* d_corr_planes, int16_t* d_shift_out, void* stream);
int lspiv_piv_multipass_deform_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                                  int n_passes, const int* passes, int n_deform, float signal_threshold, int64_t pair_offset,
                                  float* u, float* v, float* corr_max, float* s2n, float* corr_planes, int16_t* shift_out);

/* SPOF phase-filtered correlation (the project's own semantics, unpinned): the per-pair result with the
 * symmetric phase-only filter ("robust phase correlation") as the weighting of the cross spectrum, for imagery whose static or slow
 * background -- bed texture, standing ripples, glare -- carries more spectral energy than the tracers.  Replaces ffpiv.cross_corr +
 * the corr_max / s2n reductions + ffpiv.u_v_displacement (pyorc/velocimetry/ffpiv.py:446-474) with, per pair of N x N windows A, B
 * (N = wy = wx in {16, 32, 64}): a^ = normalize_intensity(A), b^ likewise ("std_ddof" and the zero clip as everywhere);
 * Rn = conj(fft2 a^) fft2 b^ / N^2; R' = Rn / sqrt(|Rn|), 0 where Rn = 0; plane = clip(fftshift(ifft2(R').real), 0, 1), where the lower
 * bound removes true negative lobes; corr_max = max of the plane; s2n = max / mean of the CLIPPED plane; u, v = the first maximum in
 * row-major order and the three-point log-Gaussian fit on plane + 1e-7 ("border_peak", "v_sign" as everywhere).  signal_threshold
 * scores A and B as lspiv_piv_pairs_dev_at does: a failing pair, or one with a non-finite sample, gives NaN u, v, corr_max, s2n and a
 * NaN plane; a zero-variance window an exactly zero plane.  float32 arithmetic WITHOUT a float64 rescue pass (a filtered plane is no
 * sum of lag products the rescue kernels could re-evaluate): the "rescue" option has no effect here.  Options "norm_clip" = 0 and
 * "signal_mode" = 1 and every other window are LSPIV_EUNSUPPORTED.
 *
 * lspiv_spof_supported: 1 for wy = wx in {16, 32, 64}, else 0.  Host-only.
 * lspiv_piv_spof_pairs_dev_at: d_out, d_corr_planes as lspiv_piv_pairs_dev_at lays them out.  One window per job, one plane per inverse
 * transform: a window's result depends on its own samples alone, so every chunking gives the same bits; pair_offset is accepted for
 * symmetry.  No workspace next to the frames and results.
 * lspiv_piv_spof_pairs_at: the host-fed twin -- the chunk is staged like lspiv_piv_pairs_at stages it (float64 narrowed to float32). */
#define LSPIV_FILTER_NONE 0
#define LSPIV_FILTER_SPOF 1
int lspiv_spof_supported(int wy, int wx);
int lspiv_piv_spof_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                                float* d_out, float* d_corr_planes, void* stream);
int lspiv_piv_spof_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                            int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset,
                            float* u, float* v, float* corr_max, float* s2n, float* corr_planes);

/* Image mask (the project's own semantics, unpinned): the per-pair result over the VALID samples of each
 * window, for windows that straddle banks, piers, vegetation or the edge of the orthoprojected area.  Replaces ffpiv.cross_corr + the
 * corr_max / s2n reductions + ffpiv.u_v_displacement (pyorc/velocimetry/ffpiv.py:446-474) with, per pair of N x N windows A, B
 * (N = wy = wx in {16, 32, 64}) under the window M of the mask (H x W bytes, non-zero = valid, one mask for every frame), k = sum M:
 * mean = sum M A / k, std = sqrt(sum M (A - mean)^2 / k) ("std_ddof": k - 1), a^ = max((A - mean) / std, 0) on valid samples, 0 where
 * std = 0 and EXACTLY 0 on excluded samples, b^ likewise under the same M; plane = clip(fftshift(irfft2(conj(rfft2 a^) rfft2 b^)) / k,
 * 0, 1); corr_max = max of the plane; s2n = max / mean of the plane over all N^2 samples; u, v = the first maximum in row-major order
 * and the three-point log-Gaussian fit on plane + 1e-7 ("border_peak", "v_sign" as everywhere).  An excluded sample never enters the
 * arithmetic: a NaN, Inf or any value there changes no bit of any result.  k < k_min (the caller's max(2, ceil(coverage * N^2)), formed
 * in float64 on the host), a valid non-finite sample, or a pair failing signal_threshold -- the share of signal samples AMONG THE VALID
 * ones, count / k, of A and of B -- gives NaN u, v, corr_max, s2n and a NaN plane.  A window with k = N^2 gives the plane of
 * lspiv_piv_pairs_dev_at.  The float64 rescue pass follows as on the other per-pair paths ("rescue"), with the mask.  Options
 * "norm_clip" = 0 and "signal_mode" = 1 and every other window are LSPIV_EUNSUPPORTED; k_min outside 2 .. N^2 is LSPIV_EINVAL.
 *
 * lspiv_mask_supported: 1 for wy = wx in {16, 32, 64}, else 0.  Host-only.
 * lspiv_piv_masked_pairs_dev_at: d_mask is H x W bytes on the device; the kernels read the caller's bytes as they are (a lane folds its
 * row of them into one bit per sample), no copy is made.  d_out, d_corr_planes as lspiv_piv_pairs_dev_at lays them out.  One window per
 * job, one plane per inverse transform: a window's result depends on its own samples and its own mask alone, so every chunking gives
 * the same bits; pair_offset is accepted for symmetry.
 * lspiv_piv_masked_pairs_at: the host-fed twin -- the chunk is staged like lspiv_piv_pairs_at stages it (float64 narrowed to float32),
 * `mask` (H x W bytes of host memory) goes up once per call into memory the library owns. */
int lspiv_mask_supported(int wy, int wx);
int lspiv_piv_masked_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                  int wy, int wx, int oy, int ox, const uint8_t* d_mask, int64_t k_min,
                                  float signal_threshold, int64_t pair_offset, float* d_out, float* d_corr_planes, void* stream);
int lspiv_piv_masked_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                              int wy, int wx, int oy, int ox, const uint8_t* mask, int64_t k_min,
                              float signal_threshold, int64_t pair_offset,
                              float* u, float* v, float* corr_max, float* s2n, float* corr_planes);

/* ---- Second correlation peak (additions, no ABI version change) ------------------------------------------
 * How far a vector can be trusted: the height of the second highest correlation peak, the PEAK RATIO p1 / corr2 PIV practice validates
 * with, and the runner-up vector that replaces a rejected one -- per window and pair, without the planes leaving the device.
 * On the fft-shifted plane (the orientation of lspiv_u_v_displacement), with (ip, jp) the primary peak (first maximum in row-major order),
 * p1 its height and r = peak_exclusion, 1 <= r <= N / 4: a sample s at (i, j) is a CANDIDATE when (1) s >= 1e-5 (five times the plane
 * gate of 2e-6: float32 noise around an isolated peak is no peak), (2) (i, j) lies outside the box |i - ip| <= r and |j - jp| <= r, which
 * is clipped at the plane edge and does not wrap, and (3) s >= each of its existing 4-neighbours -- a neighbour outside the plane does
 * not exist, one inside the box counts; this is what takes out the flank of the primary peak.  The second peak is the candidate with the
 * largest value, the first in row-major order among equals.  Per window the block peak2 holds four consecutive floats
 *   {u2, v2, corr2, peak_ratio}: corr2 its height, peak_ratio = p1 / corr2, (u2, v2) its displacement by the primary's rule -- the
 *   three-point log-Gaussian fit on plane + 1e-7 inside, "border_peak" on the plane border, "v_sign" on v2.
 * No candidate: corr2 = 0, peak_ratio = +inf, u2 = v2 = NaN.  A skipped window (signal_threshold, non-finite input; a NaN plane) is NaN
 * in all four.  The second peak is taken on the float32 plane at the float32 arg-max: the float64 rescue pass ("rescue") corrects u, v as
 * after every per-pair kernel and leaves the four alone.
 *
 * lspiv_peak2_supported: 1 for wy = wx in {16, 32, 64}, else 0.  Host-only.
 * lspiv_piv_peak2_pairs_dev_at: lspiv_piv_shift_pairs_dev_at without offsets -- d_out, d_corr_planes as lspiv_piv_pairs_dev_at lays them
 * out, the same bits as that call with d_shift = NULL -- plus d_peak2: (T - 1) * n_win * 4 floats, 16-byte aligned.  One window per job,
 * pair-local: every chunking gives the same bits; pair_offset is accepted for symmetry.  Options "norm_clip" = 0 and "signal_mode" = 1
 * and every other window are LSPIV_EUNSUPPORTED; peak_exclusion outside 1 .. N / 4 is LSPIV_EINVAL.
 * lspiv_piv_peak2_pairs_at: the host-fed twin, staged like lspiv_piv_pairs_at.
 * lspiv_second_peak_dev / lspiv_second_peak: the same rule and the same fit on planes that already exist -- n_planes (P * n_win)
 * fft-shifted float32 planes of wy x wx, 4 .. 4096 px per side, any shape, 1 <= peak_exclusion <= min(wy, wx) / 4 -- lspiv_piv_pairs'
 * corr_planes, an ensemble's mean planes; p1 is the plane's first maximum.  On the planes lspiv_piv_peak2_pairs_dev_at returns, the four
 * outputs are that call's bits. */
int lspiv_peak2_supported(int wy, int wx);
int lspiv_piv_peak2_pairs_dev_at(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W,
                                 int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset, int peak_exclusion,
                                 float* d_out, float* d_peak2, float* d_corr_planes, void* stream);
int lspiv_piv_peak2_pairs_at(const void* frames, int dtype, int64_t T, int64_t H, int64_t W,
                             int wy, int wx, int oy, int ox, float signal_threshold, int64_t pair_offset, int peak_exclusion,
                             float* u, float* v, float* corr_max, float* s2n, float* peak2, float* corr_planes);
int lspiv_second_peak_dev(const float* d_planes, int64_t n_planes, int wy, int wx, int peak_exclusion, float* d_peak2, void* stream);
int lspiv_second_peak(const float* corr_planes, int64_t P, int64_t n_win, int wy, int wx, int peak_exclusion, float* peak2);

/* Host frames into a slice of an HBM-resident stack, the way lspiv_piv_pairs brings them in -- pinned ring, staging threads,
 * float64 narrowed to float32 with the "narrow_offset" guard (so d_dst receives n_frames * H * W samples of LSPIV_F32 for LSPIV_F64
 * input, of `dtype` otherwise) -- without launching anything: what lets the chunk loop of pyorc/velocimetry/ffpiv.py:399-440 keep a
 * LAZY stack resident in HBM, filled in whatever pieces dask delivers (its own blocks: no frame is decoded twice) and launched on
 * the kernels' anchors (pyorc_amd/resident.py).  signal_threshold: that of the PIV call which will read the frames (it decides the
 * guard exactly as there).  Blocking; waits for the library's stream before the first DMA. */
int lspiv_upload_frames(void* d_dst, const void* frames, int dtype, int64_t n_frames, int64_t H, int64_t W,
                        float signal_threshold);

/* replaces ffpiv.u_v_displacement on an existing plane volume (pyorc/velocimetry/ffpiv.py:324,471):
 * planes (P, n_win, wy, wx) float32 -> u, v (P * n_win) float32 in pixels.                   */
int lspiv_u_v_displacement(const float* corr_planes, int64_t P, int64_t n_win, int wy, int wx,
                           float* u, float* v);

/* ---------------------------------------------------------------- ensemble correlation --- */
/* replaces _get_ffpiv_mean (pyorc/velocimetry/ffpiv.py:182-376): corr_sum / corr_count stay in
 * HBM across chunks; per-pair corr_max / s2n (masked to 0 like ffpiv.py:238-241) are returned per
 * chunk for the time averages of ffpiv.py:284-286.  The handle counts the pairs it has seen: chunks are
 * consecutive, and chunkings whose boundaries are multiples of lspiv_chunk_alignment() give the same bits. */
typedef struct lspiv_ensemble lspiv_ensemble;
int lspiv_ensemble_begin(int64_t H, int64_t W, int wy, int wx, int oy, int ox, lspiv_ensemble** handle);
int lspiv_ensemble_accumulate(lspiv_ensemble* handle, const void* frames, int dtype, int64_t T,
                              float corr_min, float s2n_min, float signal_threshold,
                              float* corr_max /* (T-1)*n_win */, float* s2n /* (T-1)*n_win */);
/* same on a device-resident chunk: d_corr_s2n = [corr_max | s2n], 2*(T-1)*n_win float32 in HBM; asynchronous on
 * `stream` (NULL = the library's stream). */
int lspiv_ensemble_accumulate_dev(lspiv_ensemble* handle, const void* d_frames, int dtype, int64_t T,
                                  float corr_min, float s2n_min, float signal_threshold,
                                  float* d_corr_s2n, void* stream);
/* count filter (count < count_min * n_frames -> NaN), mean plane, sub-pixel peak.
 * u, v (n_win) in pixels; corr_count (n_win) float32; corr_mean NULL or n_win*wy*wx float32.  */
int lspiv_ensemble_finish(lspiv_ensemble* handle, float count_min, float n_frames,
                          float* u, float* v, float* corr_count, float* corr_mean);
/* running state out of / into HBM: corr_sum (n_win*wy*wx, fft-shifted planes) and corr_count (n_win).  Multi-GPU
 * ensemble = every rank accumulates its own time block, the states are summed (one all-reduce) and
 * imported on the rank that calls lspiv_ensemble_finish.  `add` != 0 adds to the current state instead of replacing. */
/* Float64 rescue of the FINAL fit (round 4).  lspiv_ensemble_finish fits the mean plane; where that float32 fit is
 * ill-conditioned (same flag model as the per-pair "rescue" option: a neighbour of the peak near zero, a flat ridge, samples tying
 * for the maximum -- rare, and mostly in ensembles of a few pairs) the samples the fit reads are re-evaluated in float64 from the
 * FRAMES, over the pairs that were added to the sum, and u, v are overwritten.  The frames therefore have to be reachable at
 * finish:
 *   - lspiv_ensemble_accumulate (host frames) keeps its upload buffers in HBM until finish / destroy, as long as they fit
 *     LSPIV_ENSEMBLE_RETAIN_BYTES (default: a quarter of the device memory); beyond that nothing is re-evaluated from frames;
 *   - lspiv_ensemble_accumulate_dev keeps nothing by default (LSPIV_RETAIN_NONE: no re-evaluation from frames);
 *     LSPIV_RETAIN_COPY makes the handle copy every chunk (same budget), LSPIV_RETAIN_BORROW only records the caller's pointer --
 *     the caller then guarantees that every chunk handed to accumulate_dev stays valid and unchanged until finish;
 *   - a state brought in with lspiv_ensemble_import holds pairs whose frames this handle never saw: lspiv_ensemble_finish
 *     re-evaluates nothing from frames then (the staged finish below is the multi-GPU way).
 * Without the frames the flagged windows get the float64 fit of the five samples of the float32 mean plane (the 3-point fit's own
 * arithmetic, not the plane, is then exact; "peaks_refitted" above).
 * Set the mode before the first accumulate call.  lspiv_ensemble_stats after finish: stats[0..5] = windows flagged, windows
 * re-evaluated from the frames, windows left without that (no frames / more than four arg-max candidates / list limit), chunks kept,
 * bytes kept, 1 if every chunk could be kept. */
#define LSPIV_RETAIN_NONE   0
#define LSPIV_RETAIN_COPY   1
#define LSPIV_RETAIN_BORROW 2
int lspiv_ensemble_set_retain(lspiv_ensemble* handle, int mode);
int lspiv_ensemble_stats(lspiv_ensemble* handle, int64_t* stats);
/* The same rescue when the sum is spread over several handles (multi-GPU: every rank accumulated its own time block, the
 * states were all-reduced and imported -- replaced, `add` = 0 -- on every rank, so all hold the same sums).  lspiv_ensemble_finish
 * in three stages:
 *   lspiv_ensemble_flag            mean planes, float32 fits, the flagged windows sorted by index: the same *n_records and the
 *                                  same list on every rank;
 *   lspiv_ensemble_partials        this handle's float64 sums over ITS retained chunks, partials[n_records][LSPIV_ENS_PARTIAL_DOUBLES];
 *                                  *complete = 0 (and zeros) if some chunk of this handle could not be kept -- the ranks then agree
 *                                  (one more all-reduce) to call plain lspiv_ensemble_finish instead;
 *   [the caller sums `partials` over the ranks: one float64 all-reduce]
 *   lspiv_ensemble_finish_partials the fits of the flagged windows from the totals, then the outputs of lspiv_ensemble_finish. */
#define LSPIV_ENS_PARTIAL_DOUBLES 20
int lspiv_ensemble_flag(lspiv_ensemble* handle, float count_min, float n_frames, int64_t* n_records);
/* 64-bit digest (FNV-1a) of the last lspiv_ensemble_flag's sorted records -- window, number of candidates, candidate positions --,
 * 0 without records: ranks compare it (one MAX all-reduce) before they add their partials POSITIONALLY; the same count of
 * flagged windows does not prove the same windows (round 5). */
int lspiv_ensemble_flag_digest(lspiv_ensemble* handle, uint64_t* digest);
int lspiv_ensemble_partials(lspiv_ensemble* handle, double* partials, int* complete);
int lspiv_ensemble_finish_partials(lspiv_ensemble* handle, const double* partials, float* u, float* v, float* corr_count,
                                   float* corr_mean);
int lspiv_ensemble_export(lspiv_ensemble* handle, float* corr_sum, float* corr_count);
int lspiv_ensemble_import(lspiv_ensemble* handle, const float* corr_sum, const float* corr_count, int add);
/* corr_sum / corr_count of n handles (same geometry, any devices; n <= 64) summed in handle order, ((s0 + s1) + s2) + ..., and
 * written back to EVERY handle as its replaced state -- what an all-reduce followed by lspiv_ensemble_import(add = 0) on each handle
 * leaves, bit for bit (adds only, one float32 rounding each: a float32 sum in the same order matches).  The sum runs on handles[0]'s
 * device; other devices' buffers are read over the fabric where peer access is possible, else copied there first; the total goes back
 * with peer copies.  Every handle is marked as holding a foreign state, so the staged finish below (flag / partials / finish_partials)
 * keeps the float64 rescue.  Waits for every handle's accumulations; takes the host locks of the devices involved in ascending order;
 * the calling thread's device is unchanged afterwards. */
int lspiv_ensemble_allreduce(lspiv_ensemble** handles, int n);
/* Sliding ensemble: time-resolved fields from a moving window of pairs (the project's own mode).  The
 * pairs of the run, by absolute index, form blocks of `stride_pairs` = s; output j is fitted on the mean plane of the
 * `window_pairs` = M pairs of blocks j .. j + M / s - 1 (1 <= s <= M, M % s == 0, else LSPIV_EINVAL).  Call before the first
 * accumulate only.  The handle then keeps a BLOCK STORE in HBM -- one plane sum and one count per (block, window) for the whole run,
 * n_win * (wy * wx + 1) * 4 bytes per block, grown geometrically, LSPIV_ENOMEM with the bytes it needed when that fails -- and leaves
 * corr_sum / corr_count untouched.  Every pair is correlated once.  A block sum is a fixed sequence of float32 additions in pair
 * order and an output a fixed sequence of block sums: the results are bit-identical for every chunking whose boundaries are
 * multiples of s.  Every accumulate call must hold a multiple of s pairs unless it is the last one (LSPIV_EINVAL otherwise); the
 * pairs after the last whole block are correlated -- their corr_max / s2n are returned -- and enter no output.  The even square
 * windows 6 .. 64 run the time-walking ensemble kernel once per call with one segment per block; every other window size, and
 * LSPIV_WALK=0, take one launch of the one-owner ensemble kernel per block: correct for every size the ensemble mode supports, and
 * slower.  The first accumulate records the slot layout of the store; a later call that would write another one (LSPIV_WALK changed
 * in between, 64 x 64 windows) returns LSPIV_EINVAL, and lspiv_ensemble_sliding_finish decodes the recorded layout.  On such a handle lspiv_ensemble_finish, _flag, _partials, _finish_partials, _export, _import and _allreduce return
 * LSPIV_EINVAL. */
int lspiv_ensemble_set_sliding(lspiv_ensemble* handle, int64_t window_pairs, int64_t stride_pairs);
/* Room in the block store of a sliding handle for a run of `n_pairs` pairs in all, allocated once: a caller that knows the length of
 * its run calls this before the first accumulate, and the store is then neither grown nor moved (growing doubles the store and copies
 * the blocks written so far, with the old and the new store alive together).  LSPIV_ENOMEM with the bytes it needed; never shrinks. */
int lspiv_ensemble_sliding_reserve(lspiv_ensemble* handle, int64_t n_pairs);
/* Outputs [first_out, first_out + n_out) of a sliding handle, of the (pairs accumulated / s) - M / s + 1 there are (LSPIV_EINVAL
 * outside that range; may be called more than once): per output and window the block sums and counts added in block order, NaN plane
 * and NaN u, v where the count is < count_min * M, else the mean plane and its sub-pixel peak as in lspiv_ensemble_finish.
 * u, v, corr_count: (n_out, n_win) float32; corr_mean NULL or (n_out, n_win, wy, wx).  Works through the outputs in tiles sized to
 * the plane workspace.  The float64 rescue re-evaluates an output's ill-conditioned fits over ITS pairs from the retained frames,
 * under the retention rules of lspiv_ensemble_finish; lspiv_ensemble_stats then reports the totals over the outputs of this call. */
int lspiv_ensemble_sliding_finish(lspiv_ensemble* handle, float count_min, int64_t first_out, int64_t n_out,
                                  float* u, float* v, float* corr_count, float* corr_mean);
/* Multi-pass ensemble: a SHIFTED handle (the project's own mode).  `shift`: n_win x {dy, dx} int16, the
 * integer offset of every window's cut of frame t+1 from its cut of frame t, the SAME for every pair of the run; it is copied into the
 * handle and clamped there so that the shifted window stays inside the frame (lspiv_ensemble_get_shift returns the clamped values, n_win
 * x {dy, dx}; LSPIV_EINVAL on a handle without offsets).  NULL clears the offsets: the plain ensemble again.  Before the first
 * accumulate only, and not on a sliding handle (LSPIV_EINVAL); the window must satisfy lspiv_shift_supported and the option norm_clip
 * be 1 (LSPIV_EUNSUPPORTED).  "_dev": the same from a device array; the copy runs on `stream` (NULL: the library's) and has completed
 * on return.  On a shifted handle lspiv_ensemble_accumulate / _accumulate_dev run the shifted ensemble kernel -- one owner per window,
 * one plane per inverse transform, float32 additions in pair order: the same bits for every chunking -- and return LSPIV_EUNSUPPORTED
 * under the option signal_mode = 1, as multi-pass PIV does; lspiv_ensemble_finish / _finish_partials fit the mean plane, rescue that
 * fit in float64 at the clamped offsets, and return the TOTAL displacement u = dx + residual, v = dy + residual (float32 sums; a NaN
 * residual stays NaN, a zero offset leaves the residual's bits; "v_sign" applied last).  lspiv_ensemble_export / _import carry the
 * sums as before; lspiv_ensemble_allreduce returns LSPIV_EINVAL unless every handle holds the same clamped offsets (or none). */
int lspiv_ensemble_set_shift(lspiv_ensemble* handle, const int16_t* shift);
int lspiv_ensemble_set_shift_dev(lspiv_ensemble* handle, const int16_t* d_shift, void* stream);
int lspiv_ensemble_get_shift(lspiv_ensemble* handle, int16_t* shift);
/* SPOF phase-filtered ensemble: filter = LSPIV_FILTER_SPOF makes the handle sum the planes of
 * lspiv_piv_spof_pairs_dev_at in place of ffpiv.cross_corr's (pyorc/velocimetry/ffpiv.py:222-241): a plane failing corr_min / s2n_min
 * / finite counts as zero, corr_sum += plane, corr_count += (corr_max > 1e-6), the returned per-pair corr_max / s2n are the masked values
 * of the FILTERED planes -- corr_min / s2n_min keep their meaning, their useful values are lower (filtered peaks are lower).
 * LSPIV_FILTER_NONE: the plain ensemble again.  Before the first accumulate only (LSPIV_EINVAL); not on a sliding or a shifted handle,
 * and a filtered handle refuses lspiv_ensemble_set_sliding / _set_shift (LSPIV_EINVAL); the window must satisfy lspiv_spof_supported
 * and the options be as for the per-pair entry point (LSPIV_EUNSUPPORTED).  lspiv_ensemble_accumulate / _accumulate_dev then run the
 * filtered ensemble kernel -- one owner per window, one plane per inverse transform, float32 additions in pair order: the same bits for
 * every chunking.  lspiv_ensemble_finish / _finish_partials form the mean plane, the count filter and the fit as before, WITHOUT the
 * float64 rescue (lspiv_ensemble_flag reports no records, nothing is retained for it).  lspiv_ensemble_export / _import carry the
 * sums and leave the handle's filter as it is; lspiv_ensemble_allreduce returns LSPIV_EINVAL unless every handle has the same filter. */
int lspiv_ensemble_set_spectral_filter(lspiv_ensemble* handle, int filter);
int lspiv_ensemble_get_spectral_filter(lspiv_ensemble* handle, int* filter);
int lspiv_ensemble_destroy(lspiv_ensemble* handle);

/* ---------------------------------------------------------------- next rows */
/* N1 -- orthoprojection: replaces pyorc.project.img_to_ortho applied per frame by project_numpy
 * (pyorc/project.py:123-230), the numba group average (:19-53) and Frames.project's fillna(0.0)
 * (pyorc/api/frames.py:265).  The index maps are the outputs of CameraConfig.map_idx_img_ortho /
 * map_mean_idx_img_ortho (pyorc/api/cameraconfig.py:739-860):
 *   idx_img[K], idx_ortho[K]   nearest neighbour: out[idx_ortho[k]] = img[idx_img[k]] (flat indices; later k wins)
 *   src_idx[M], norm_idx[M]    group means: sample img[src_idx[i]] belongs to group norm_idx[i] (0..G-1)
 *   uidx[G]                    flat output index of every group; M = 0 disables the mean step (reducer != "mean")
 * Output: (T, dst_h, dst_w) float32, the values the reference returns (widened to float64 there).            */
typedef struct lspiv_projection lspiv_projection;
int lspiv_projection_create(int64_t src_h, int64_t src_w, int64_t dst_h, int64_t dst_w,
                            const int64_t* idx_img, const int64_t* idx_ortho, int64_t K,
                            const int64_t* src_idx, const int64_t* norm_idx, int64_t M,
                            const int64_t* uidx, int64_t G, lspiv_projection** handle);
int lspiv_project_frames(lspiv_projection* handle, const void* frames, int dtype, int64_t T, float* out);
int lspiv_project_frames_dev(lspiv_projection* handle, const void* d_frames, int dtype, int64_t T, float* d_out,
                             void* stream);
/* A plan without group means (G = 0, Frames.project with a reducer other than "mean": pyorc/project.py:196-199) gives every
 * cell a source byte or 0, so a uint8 stack may stay uint8: (T, dst_h, dst_w) uint8 holding the values lspiv_project_frames
 * returns as float32 -- a quarter of the bytes, and get_piv runs its uint8 kernels on them.  LSPIV_EINVAL for a plan
 * with group means.                                                                                            */
int lspiv_project_frames_u8(lspiv_projection* handle, const uint8_t* frames, int64_t T, uint8_t* out);
int lspiv_project_frames_u8_dev(lspiv_projection* handle, const uint8_t* d_frames, int64_t T, uint8_t* d_out, void* stream);
int lspiv_projection_destroy(lspiv_projection* handle);

/* N1, method "cv" -- replaces pyorc.project.project_cv (pyorc/project.py:56-120): cv2.undistort(img, camera_matrix,
 * dist_coeffs) (pyorc/cv.py:1392-1413) followed by cv2.warpPerspective(img, M, (dst_w, dst_h), flags=INTER_AREA)
 * (pyorc/cv.py:993-1013; OpenCV turns INTER_AREA into INTER_LINEAR there).  OpenCV's published algorithm is restated --
 * initUndistortRectifyMap / the inverted homography evaluated in double, source coordinates quantised to 1/32 pixel,
 * fixed-point bilinear blend (2^15 weights, round half up) for uint8 and the float32 weight table for float32 frames,
 * BORDER_CONSTANT 0 -- NOT pinned against a real cv2 (absent here).  camera_matrix 3x3 row-major or NULL (no
 * undistortion step); dist_coeffs k1 k2 p1 p2 [k3 [k4 k5 k6]] (n_dist 0, 4, 5 or 8); M the 3x3 source-to-destination
 * homography of cv2.getPerspectiveTransform (pyorc/cv.py:769-795).  Frames uint8 or float32; the output has the dtype
 * of the input, (T, dst_h, dst_w), like the reference (pyorc/project.py:112). */
typedef struct lspiv_remap lspiv_remap;
int lspiv_project_cv_create(int64_t src_h, int64_t src_w, int64_t dst_h, int64_t dst_w, const double* camera_matrix,
                            const double* dist_coeffs, int n_dist, const double* M, lspiv_remap** handle);
int lspiv_project_cv_frames(lspiv_remap* handle, const void* frames, int dtype, int64_t T, void* out);
int lspiv_project_cv_frames_dev(lspiv_remap* handle, const void* d_frames, int dtype, int64_t T, void* d_out, void* stream);
int lspiv_project_cv_destroy(lspiv_remap* handle);

/* N2 -- element-wise pre-processing filters the reference writes in plain numpy (bit-reproducible):
 *   lspiv_time_diff   Frames.time_diff (pyorc/api/frames.py:409-436): out (T-1,H,W) float32 = f32(frame t+1) - f32(frame t),
 *                     values <= thres and NaN -> 0, |.| if use_abs
 *   lspiv_minmax      Frames.minmax (:344-362) on float32 frames: maximum(minimum(x, hi), lo), NaN propagates
 *   lspiv_reduce_rolling  Frames.reduce_rolling (:381-407) on uint8 frames, float64 arithmetic: trailing rolling mean over
 *                     `samples` frames removed, clipped at 0, per-frame (x * 255 / max) -> uint8, 0 where the rolling mean is 0;
 *                     frames without a complete window and frames whose maximum is 0 come out 0 (NaN.astype(uint8) on x86)
 *   lspiv_time_range  Frames.range (:364-379): out (H,W) in the frames' dtype = max over time - min over time (NaN skipped
 *                     for float frames, an all-NaN pixel stays NaN)
 *   lspiv_normalize   Frames.normalize (:279-306) on uint8 frames: float32 mean of frames [::round(T/samples)] removed,
 *                     per-frame ((x - min) / (max - min) * 255) -> uint8
 *   lspiv_gaussian_blur / lspiv_edge_detect   Frames.smooth (:438-467) / Frames.edge_detect (:308-342): pyorc calls
 *                     cv2.GaussianBlur(float32, (k, k), 0) (pyorc/cv.py:142-183); OpenCV's published algorithm is
 *                     restated (coefficient tables for k <= 7, separable, BORDER_REFLECT_101): NOT bit-pinned, ~1e-6.
 *                     out (T,H,W) float32; ksize odd, 1..31; edge = blur(ksize_2) - blur(ksize_1).
 * Host pointers; *_dev take device pointers. */
int lspiv_gaussian_blur(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize, float* out);
int lspiv_gaussian_blur_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize, float* d_out,
                            void* stream);
int lspiv_edge_detect(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2, float* out);
int lspiv_edge_detect_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2,
                          float* d_out, void* stream);
/* Frames.edge_detect followed by Frames.minmax (the reference's recipe order, examples/ngwerere/ngwerere.yml:6-11; pyorc/api/frames.py:308-362)
 * in one pass: np.maximum(np.minimum(x, hi), lo) applied as the band-filtered value is stored -- the bits of lspiv_edge_detect_dev +
 * lspiv_minmax_dev without the second trip over the float32 stack.  -INFINITY / INFINITY switch a limit off. */
int lspiv_edge_detect_clip_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, int ksize_1, int ksize_2, float lo,
                               float hi, float* d_out, void* stream);
int lspiv_time_diff(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, float thres, int use_abs, float* out);
int lspiv_time_diff_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, float thres, int use_abs,
                        float* d_out, void* stream);
int lspiv_time_range(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, void* out);
int lspiv_time_range_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, void* d_out, void* stream);
int lspiv_minmax(const float* frames, int64_t n, float lo, float hi, float* out);
int lspiv_minmax_dev(const float* d_frames, int64_t n, float lo, float hi, float* d_out, void* stream);
int lspiv_normalize(const uint8_t* frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* out);
int lspiv_normalize_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* d_out, void* stream);
/* The two halves of lspiv_normalize_dev, for a stack that arrives in pieces (pyorc_amd/pipeline.py streams the camera frames
 * in while earlier ones are processed): the float32 mean plane (H,W) of frames [::round(T/samples)] of a T-frame stack of
 * which only those frames need to be resident yet, and the per-frame stretch of any run of frames against a given mean plane.
 * mean + apply over the whole stack == lspiv_normalize_dev bit for bit (the stretch uses per-frame statistics only). */
int lspiv_normalize_mean_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, float* d_mean, void* stream);
int lspiv_normalize_apply_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, const float* d_mean, uint8_t* d_out,
                              void* stream);
int lspiv_reduce_rolling(const uint8_t* frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* out);
int lspiv_reduce_rolling_dev(const uint8_t* d_frames, int64_t T, int64_t H, int64_t W, int samples, uint8_t* d_out, void* stream);

/* N3 -- post-PIV masks, ds.velocimetry.mask.* (pyorc/api/mask.py:147-403), on the result block
 * fields = [v_x | v_y | corr | s2n], each (T, R, C) float32 (lspiv_piv_pairs_dev's d_out after
 * lspiv_scale_velocity_dev).  mask: uint8, 1 = keep; (T, R, C), or (R, C) for the time-reducing kinds.
 * xarray's expressions are restated through the numpy calls they dispatch to (oracle/mask_oracle.py; unpinned
 * against a real xarray).  Reference quirks kept: stack_window's y range excludes +wdw (helpers.py:672-679),
 * variance's np.maximum(mean, 1e30), rolling's NaN edges.
 *   kind                     params (doubles)                                         mask shape
 *   LSPIV_MASK_MINMAX      0 s_min, s_max                                 :147-160    (T,R,C)
 *   LSPIV_MASK_ANGLE       1 angle_expected, angle_tolerance              :162-185    (T,R,C)
 *   LSPIV_MASK_COUNT       2 tolerance                                    :187-201    (R,C)
 *   LSPIV_MASK_CORR        3 tolerance                                    :203-213    (T,R,C)
 *   LSPIV_MASK_S2N         4 tolerance                                    :215-225    (T,R,C)
 *   LSPIV_MASK_OUTLIERS    5 tolerance, mode (0 "or", 1 "and")            :227-252    (T,R,C)
 *   LSPIV_MASK_VARIANCE    6 tolerance, mode                              :254-284    (R,C)
 *   LSPIV_MASK_ROLLING     7 wdw, tolerance                               :286-303    (T,R,C)
 *   LSPIV_MASK_WINDOW_NAN  8 tolerance, x_min, x_max, y_min, y_max        :305-340    (T,R,C)
 *   LSPIV_MASK_WINDOW_MEAN 9 tolerance, mode, x_min, x_max, y_min, y_max  :342-383    (T,R,C)
 * lspiv_mask_apply    ds[var].where(mask) on all four variables (:132-145); mask_has_time 0 for an (R,C) mask.
 * lspiv_time_mean     ds.mean(dim="time") -- the reduce_time=True pre-step (:51-52); out (4, R, C).
 * lspiv_window_replace  fillna with the neighbourhood nanmean, iter times (:385-403), in place.
 * lspiv_scale_velocity_dev  px/frame -> m/s in place on the first two planes: (u * res / dt).astype(float32),
 *                     pyorc/velocimetry/ffpiv.py:418-419; dt: HOST array, one entry per time step. */
#define LSPIV_MASK_MINMAX 0
#define LSPIV_MASK_ANGLE 1
#define LSPIV_MASK_COUNT 2
#define LSPIV_MASK_CORR 3
#define LSPIV_MASK_S2N 4
#define LSPIV_MASK_OUTLIERS 5
#define LSPIV_MASK_VARIANCE 6
#define LSPIV_MASK_ROLLING 7
#define LSPIV_MASK_WINDOW_NAN 8
#define LSPIV_MASK_WINDOW_MEAN 9
int lspiv_mask(const float* fields, int64_t T, int64_t R, int64_t C, int kind, const double* params, int n_params,
               uint8_t* mask);
int lspiv_mask_dev(const float* d_fields, int64_t T, int64_t R, int64_t C, int kind, const double* params, int n_params,
                   uint8_t* d_mask, void* stream);
int lspiv_mask_apply(float* fields, int64_t T, int64_t R, int64_t C, const uint8_t* mask, int mask_has_time);
int lspiv_mask_apply_dev(float* d_fields, int64_t T, int64_t R, int64_t C, const uint8_t* d_mask, int mask_has_time,
                         void* stream);
int lspiv_time_mean(const float* fields, int64_t T, int64_t R, int64_t C, float* out);
int lspiv_time_mean_dev(const float* d_fields, int64_t T, int64_t R, int64_t C, float* d_out, void* stream);
int lspiv_window_replace(float* fields, int64_t T, int64_t R, int64_t C, int x_min, int x_max, int y_min, int y_max,
                         int iter);
int lspiv_window_replace_dev(float* d_fields, int64_t T, int64_t R, int64_t C, int x_min, int x_max, int y_min,
                             int y_max, int iter, void* stream);
int lspiv_scale_velocity_dev(float* d_fields, int64_t T, int64_t n_vec, double res_x, double res_y, const double* dt,
                             void* stream);

/* ---- Vector validation (additions, no ABI version change) ------------------------------------------------
 * The normalised median test (Westerweel & Scarano 2005) on the fields u, v (T, R, C) float32 while they are still in HBM, with the
 * runner-up vector of the second correlation peak as the first substitute for a rejected one.  Every iteration reads the field of the
 * iteration before it only (Jacobi): the result does not depend on the order in which vectors are visited.  For every (t, i, j):
 *   neighbours  the up to eight positions (i + di, j + dj) of the same t inside the grid whose u AND v are finite (no wrap across row
 *               ends or time steps); n their count
 *   med(x)      of n values sorted ascending: the middle one for odd n, 0.5f * (x[n/2-1] + x[n/2]) for even n
 *   limits      um = med(u_k), vm = med(v_k); ru = med(|u_k - um|), rv = med(|v_k - vm|); lu = threshold * (ru + epsilon), lv alike --
 *               every operation one correctly rounded float32 operation
 *   judged      a vector that is finite in both components and has n >= min_neighbours; anything else keeps value and flag (NaN is
 *               never filled: lspiv_window_replace does that)
 *   outlier     |u0 - um| > lu or |v0 - vm| > lv
 *   action      (1) with peak2, a vector that is still the primary one (flag 0) whose (u2, v2) are finite and no outlier against the same
 *               um, vm, lu, lv becomes (u2, v2), flag 2; else (2) replace = LSPIV_VALIDATE_NAN: NaN / NaN, flag 1; (3) replace =
 *               LSPIV_VALIDATE_MEDIAN: (um, vm), flag 3.  A flag-2 or flag-3 vector is judged again by a later iteration like any other and
 *               can only fall to (2) or (3); the flag is the last action taken.
 * flag: uint8 (T, R, C): 0 kept or unjudged, 1 rejected, 2 substituted, 3 median.  Units: those of the fields (epsilon 0.1 is meant for
 * pixels: validate before lspiv_scale_velocity_dev).  peak2: (T, R, C, 4) = {u2, v2, corr2, ratio} as lspiv_piv_peak2_pairs_dev_at writes
 * it, read only.  threshold > 0, epsilon >= 0, min_neighbours 1 .. 8, iterations 1 .. 8; a parameter outside its range, or T, R or C < 1,
 * is LSPIV_EINVAL.  Both calls work in place on u, v; d_peak2 / peak2 and d_flag / flag may be NULL.  One kernel launch per iteration;
 * the ping-pong workspace (8 bytes per vector) is the library's, grow-only.  lspiv_validate_dev is asynchronous on `stream`.
 * lspiv_validate: the host twin -- upload, the same kernels, download. */
#define LSPIV_VALIDATE_NAN 0
#define LSPIV_VALIDATE_MEDIAN 1
int lspiv_validate_dev(float* d_u, float* d_v, const float* d_peak2, int64_t T, int64_t R, int64_t C,
                       float threshold, float epsilon, int min_neighbours, int replace, int iterations,
                       uint8_t* d_flag, void* stream);
int lspiv_validate(float* u, float* v, const float* peak2, int64_t T, int64_t R, int64_t C,
                   float threshold, float epsilon, int min_neighbours, int replace, int iterations, uint8_t* flag);

/* ---- Frame stabilisation (additions, no ABI version change) -------------------------------------------------
 * Replaces pyorc/cv.py's stabilisation behind Video(stabilize=...) -- feature tracks on the banks, one transform per frame -- and the
 * cv2.warpAffine it applies to every frame on the CPU.  The semantics are this project's own (unpinned against pyorc and OpenCV):
 *   vectors  those of lspiv_piv_masked_pairs_dev_at under a static mask (non-zero = does not move in the world), window n x n; u column
 *            shift, v row shift, rows downward (a caller under the "v_sign" option = 1 negates v first); a window's position is its
 *            centre xc = col (n - ox) + (n - 1) / 2, yc = row (n - oy) + (n - 1) / 2.
 *   fit      lspiv_stabilize_fit*: P_t (2 x 3, float64) of every pair with x_{t+1} = P_t (x_t, y_t, 1) for a static point, i.e.
 *            (u, v) = (P - I)(x, y, 1), by least squares through the normal equations with float64 sums, coordinates relative to
 *            ((W - 1) / 2, (H - 1) / 2) inside the fit.  model: translation (2 unknowns), similarity (4: u = a x - b y + c, v = b x + a y + d)
 *            or affine (6).  Three rounds, each over a subset of the FINITE vectors: all; those within reject0 px of round 1's prediction;
 *            those within reject1 px of round 2's.  A round with fewer than min_vectors vectors or a singular normal matrix (determinant
 *            <= 1e-9 x the product of the matrix's diagonal) makes the pair's P the identity and n_used 0; else n_used = round 3's count.
 *            u, v: (pairs, rows, cols) float32; (rows, cols) must be the grid of (H, W, n, oy, ox); n 16, 32 or 64; reject0 > reject1 > 0.
 *            One launch for all pairs and all three rounds; the reduction order depends on the grid alone.
 *   chain    lspiv_stabilize_chain*: A_0 = carry_in (NULL: the identity), [A_{t+1}; 0 0 1] = [P_t; 0 0 1] [A_t; 0 0 1], sequentially, every
 *            product and sum a separately rounded float64 operation.  A: (pairs + 1, 2, 3); carry_out (may be NULL) = A_pairs.  A_t maps a
 *            pixel of the reference frame (frame 0 of the run) to its position in frame t: the map the warp needs, nothing is inverted.
 *            Cutting a run anywhere with a one-frame halo and carry_in = the pose at the chunk's first frame gives the same bits.
 *   warp     lspiv_warp_affine*: out[t](y, x) = the bilinear sample of frames[t] at A_t (x, y, 1), OpenCV's fixed-point walk: with
 *            xb = 64 (x / 64), x1 = x - xb: fX = ((A00 xb + A01 y + A02) + A00 x1) 32, every operation rounded on its own; NaN -> 0,
 *            clipped to int32, round half to even; integer part X >> 5, fraction X & 31; Y alike.  LSPIV_U8: integer weights,
 *            (acc + 2^14) >> 15; LSPIV_F32: the float32 weight table, added left to right.  A neighbour outside the frame counts as 0.
 *            frames, out: (T, H, W), different buffers, sides up to 32767; A: (T, 2, 3) float64 (for the "_dev" call in HBM).
 * "_dev" calls take device pointers and are asynchronous on `stream`: fit -> chain -> warp queue up without a host round trip.  The
 * host twins upload, run the same kernels and download.  A bad argument is LSPIV_EINVAL with a message. */
#define LSPIV_STABILIZE_TRANSLATION 0
#define LSPIV_STABILIZE_SIMILARITY 1
#define LSPIV_STABILIZE_AFFINE 2
int lspiv_stabilize_fit_dev(const float* d_u, const float* d_v, int64_t pairs, int64_t rows, int64_t cols, int n, int oy, int ox,
                            int64_t H, int64_t W, int model, double reject0, double reject1, int min_vectors,
                            double* d_P, int32_t* d_n_used, void* stream);
int lspiv_stabilize_fit(const float* u, const float* v, int64_t pairs, int64_t rows, int64_t cols, int n, int oy, int ox,
                        int64_t H, int64_t W, int model, double reject0, double reject1, int min_vectors,
                        double* P, int32_t* n_used);
int lspiv_stabilize_chain_dev(const double* d_P, int64_t pairs, const double* d_carry_in, double* d_A, double* d_carry_out,
                              void* stream);
int lspiv_stabilize_chain(const double* P, int64_t pairs, const double* carry_in, double* A, double* carry_out);
int lspiv_warp_affine_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* d_A, void* d_out,
                          void* stream);
int lspiv_warp_affine(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* A, void* out);

/* ---- Space-time image velocimetry, STIV (additions, no ABI version change) ----------------------------------
 * The other standard method of image-based river gauging next to PIV (Fujita et al.; Fudaa-LSPIV, Hydro-STIV and RIVeR offer it; pyorc
 * has none, so nothing is replaced and the semantics are this project's own, stated in float64 / float32 numpy by tests/stiv_ref.py):
 * the brightness along a search line laid along the flow, sampled in every frame, is stacked into a space-time image, and the speed
 * along the line is the orientation of the streaks in that image.
 *   gather   lspiv_sti_gather*: sti[s, t_offset + t, i] (float32, (S, T_total, L)) = the bilinear sample of frame t at point (s, i).
 *            points: (S, L, 2) float64 (x, y) in pixels, a HOST pointer in both forms (the entry point checks every point and prepares
 *            the sample table once per call); L >= 3; every point finite with 0 <= x <= W - 1, 0 <= y <= H - 1, else LSPIV_EINVAL with
 *            a message that names the point and its line.  ix = min(floor(x), W - 2), fx = float32(x - ix), y alike (x = W - 1 has
 *            fx = 1: nothing outside the frame is read); with the neighbours a, b (row iy) and c, d (row iy + 1) as float32:
 *            top = a + fx (b - a), bot = c + fx (d - c), value = top + fy (bot - top), every operation one correctly rounded float32
 *            operation.  A NaN sample propagates.  frames: (T, H, W), LSPIV_U8 or LSPIV_F32, sides 2 .. 32767.  Only rows
 *            [t_offset, t_offset + T) of sti are written: a video that goes through in chunks fills one space-time image, the same bits
 *            as one call.  The host twin stages the frames in chunks (at most 256 MiB; LSPIV_HOST_CHUNK_BYTES, a test hook, overrides
 *            it).  The "_dev" form keeps its sample table in the context's scratch buffer: calls that overlap in time share one
 *            stream (as with lspiv_normalize_dev).
 *   orientation  lspiv_sti_orientation*: per line s and time window k = 0 .. K - 1, K = (T - time_window) / time_stride + 1, rows
 *            k time_stride .. k time_stride + time_window - 1 of sti (S, T, L).  All arithmetic in float64 on the float32 samples.
 *            detrend != 0: every column's mean over the window (summed with t ascending, divided by time_window) is taken off it.
 *            Gradients by integer-tap separable filters, smooth = k in 0 .. 3 (k passes of the 3 x 3 binomial before a Sobel pair, the
 *            common scale dropped): Gx = dx_k(i) (x) b_{2k+2}(t), Gt = b_{2k+2}(i) (x) dx_k(t), b_m the binomial row of order m,
 *            dx_k = [-1, 0, 1] * b_{2k}; only positions whose whole (2k + 3) x (2k + 3) stencil lies inside the window count; L or
 *            time_window below 2k + 3 is LSPIV_EINVAL.  tensor (S, K, 3) = (Jxx, Jtt, Jxt) = (sum Gx^2, sum Gt^2, sum Gx Gt), float64
 *            sums in an order that depends on the shape alone.  With d = Jxx - Jtt, r = sqrt(d^2 + 4 Jxt^2): slope (S, K) =
 *            -2 Jxt / (d + r), in samples per frame, positive from point 0 towards point L - 1 (the total-least-squares orientation in
 *            its half-angle form); coherency (S, K) = r / (Jxx + Jtt).  A constant window or one with a NaN gives NaN for both.
 * "_dev" calls take device pointers (except points) and are asynchronous on `stream`: gather -> orientation queue up without a host
 * round trip.  The host twins upload, run the same kernels and download.  A bad argument is LSPIV_EINVAL with a message; nothing is
 * launched then. */
int lspiv_sti_gather_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t S, int64_t L,
                         float* d_sti, int64_t t_offset, int64_t T_total, void* stream);
int lspiv_sti_gather(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t S, int64_t L,
                     float* sti, int64_t t_offset, int64_t T_total);
int lspiv_sti_orientation_dev(const float* d_sti, int64_t S, int64_t T, int64_t L, int64_t time_window, int64_t time_stride, int smooth,
                              int detrend, double* d_tensor, double* d_slope, double* d_coherency, void* stream);
int lspiv_sti_orientation(const float* sti, int64_t S, int64_t T, int64_t L, int64_t time_window, int64_t time_stride, int smooth,
                          int detrend, double* tensor, double* slope, double* coherency);

/* ---- Pyramidal Lucas-Kanade point tracking (additions, no ABI version change) ----------------------------------
 * The third family of image-based river gauging next to PIV and STIV (KLT-IV, OTV, every OpenCV-based LSPTV script): the displacement
 * of a small window around a point between two frames, refined from the coarsest level of a Gaussian pyramid down to the frame (Lucas &
 * Kanade; the forward additive iteration of Bouguet).  Unpinned against OpenCV: the semantics are this project's own, stated in float32 /
 * float64 numpy by tests/track_ref.py.
 *   pyramid  lspiv_pyr_down*: out (T, (H + 1) / 2, (W + 1) / 2) float32 from frames (T, H, W), LSPIV_U8 or LSPIV_F32, sides 3 .. 32767.
 *            Taps [1, 4, 6, 4, 1] along x on every source row, then along y; source index 2 x + j - 2 reflected without repeating the
 *            edge (-1 -> 1, n -> n - 2); each pass ((a0 + a4) + 4 (a1 + a3)) + 6 a2, the result times 2^-8; every operation one correctly
 *            rounded float32 operation.  NaN propagates.  Level 0 of a tracker's pyramid is the frame as float32, level l is pyr_down of
 *            level l - 1; a level that pyr_down reads needs both sides >= 3, every level both >= 2.
 *   tracker  lspiv_lk_track*: pairs (t, t + 1), t = 0 .. T - 2, of frames (T >= 2, H, W); N points (x, y) float64 per pair: points
 *            (N, 2) for every pair (points_per_pair = 0) or (T - 1, N, 2) (points_per_pair != 0); guess: NULL (start at 0), or initial
 *            (u, v) in pixels of the frame, shaped like points by guess_per_pair.  window: odd, 5 .. 31 (w, r = (w - 1) / 2); levels:
 *            1 .. 5 (L; a stack too small for it is LSPIV_EINVAL with the level that fails); max_iter: 1 .. 100; eps >= 0; min_eig >= 0.
 *            Sampling at level l: a position q = (qx, qy) (float64; the point is p 2^-l) has ix = floor(qx), fx = float32(qx - ix), y
 *            alike; the sample at integer offset (i, j) has the neighbours at columns clamp(ix + j, 0, W_l - 1), clamp(ix + j + 1, 0,
 *            W_l - 1) and rows alike (the level is edge replicated: nothing outside it is read); top = a + fx (b - a), bot = c + fx (d - c),
 *            value = top + fy (bot - top), single float32 operations.
 *            Per level, from L - 1 down to 0: the template I on the (w + 2)^2 patch around the point, Ix = 0.5f (I[i, j + 1] - I[i, j - 1]),
 *            Iy alike; Gxx = sum Ix^2, Gyy = sum Iy^2, Gxy = sum Ix Iy over the w^2 window, exact float64 products, float64 sums in an
 *            order that depends on w alone.  det = Gxx Gyy - Gxy Gxy, lambda = (Gxx + Gyy - sqrt((Gxx - Gyy)^2 + 4 Gxy^2)) / (2 w^2).  The
 *            point is lost (status 2) unless det > 1e-9 Gxx Gyy and lambda >= min_eig.  Iterations: d starts at guess 2^-(L - 1) (or 0);
 *            J on the window at q = p 2^-l + d, e = I - J (float32), bx = sum e Ix, by = sum e Iy, delta = ((Gyy bx - Gxy by) / det,
 *            (Gxx by - Gxy bx) / det), every operation rounded on its own; d += delta; q outside [0, W_l - 1] x [0, H_l - 1] after the
 *            update is status 3; stop when |delta|^2 < eps^2 or after max_iter iterations at this level; between levels d <- 2 d.
 *            Outputs, (T - 1, N) each: u, v = d at level 0 (float64, pixels per frame); err = sum |I - J| / w^2 at the final d; min_eig =
 *            lambda of level 0 (NaN if the point never got there); n_iter (int32): the iterations of all levels; status (uint8): 0
 *            converged, 1 level 0 ended on max_iter (still a vector), 2 lost (see above), 3 walked out, 4 a sum that is not finite (a NaN
 *            sample), 5 the point itself is not finite.  Status 2 .. 5 have NaN in u, v, err.
 *            chain != 0 (a trajectory): points is (N, 2), the positions in frame 0, and xy (T, N, 2) is written: row 0 = points, row
 *            t + 1 = row t + (u, v) of pair t, which is tracked from row t -- pair after pair in stream order inside the call, nothing
 *            goes through the host; NaN once a point is lost.  The bits of T - 1 one-pair calls.
 *            Levels >= 1 live in a workspace the library owns (at most 1 GiB; LSPIV_TRACK_WS_BYTES, a test hook, overrides the cap):
 *            a longer run goes through it in batches of pairs with one frame of halo, the same bits.
 * "_dev" calls take device pointers throughout (the points, the guess and xy as well) and are asynchronous on `stream`; calls that
 * overlap in time share one stream (the workspace).  The host twins upload (the frames in chunks of at most 256 MiB with one frame of halo;
 * LSPIV_HOST_CHUNK_BYTES, a test hook, overrides the size), run the same kernels and download.  A bad argument is LSPIV_EINVAL with a message; nothing is launched then. */
int lspiv_pyr_down_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, float* d_out, void* stream);
int lspiv_pyr_down(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, float* out);
int lspiv_lk_track_dev(const void* d_frames, int dtype, int64_t T, int64_t H, int64_t W, const double* d_points, int64_t N,
                       int points_per_pair, const double* d_guess, int guess_per_pair, int window, int levels, int max_iter, double eps,
                       double min_eig, int chain, double* d_u, double* d_v, double* d_err, double* d_min_eig, int32_t* d_n_iter,
                       uint8_t* d_status, double* d_xy, void* stream);
int lspiv_lk_track(const void* frames, int dtype, int64_t T, int64_t H, int64_t W, const double* points, int64_t N, int points_per_pair,
                   const double* guess, int guess_per_pair, int window, int levels, int max_iter, double eps, double min_eig, int chain,
                   double* u, double* v, double* err, double* min_eig_out, int32_t* n_iter, uint8_t* status, double* xy);

/* N4 -- on-disk packing of the result variables (pyorc/const.py:80-83: int16, scale_factor 0.01,
 * _FillValue -9999; arithmetic of xarray's encoder: float32 x / float32 scale, NaN -> fill, round half even). */
int lspiv_pack_int16(const float* values, int64_t n, float scale, int fill, int16_t* packed);
int lspiv_pack_int16_dev(const float* d_values, int64_t n, float scale, int fill, int16_t* d_packed, void* stream);

/* ---------------------------------------------------------------- multi-GPU exchange ------ */
/* One process per GPU.  The reference is a single process: nothing is replaced here; frame
 * pairs are independent (docs/user-guide/velocimetry/index.rst:12-13) and the time axis is already cut into chunks
 * with a one-frame halo (pyorc/velocimetry/ffpiv.py:140), so rank r owns a contiguous block of pairs and the only
 * exchange is ONE all-gather of the packed (4, t, y, x) result block -- or, in ensemble mode, one sum all-reduce of
 * corr_sum / corr_count (ffpiv.py:361-363) before lspiv_ensemble_finish.
 *   transport LSPIV_COMM_RCCL  RCCL over xGMI; librccl.so is loaded on first use; the communicator binds to the
 *                              calling thread's current device (lspiv_set_device first);
 *   transport LSPIV_COMM_SHM   POSIX shared memory on the node, staged through host memory: plumbing tests only
 *                              (RCCL refuses two ranks on one GPU and needs a GPU; this one needs neither).
 * Rendezvous: rank 0 calls lspiv_comm_unique_id and hands the LSPIV_COMM_ID_BYTES to the other ranks (file, pipe,
 * environment); every rank then calls lspiv_comm_init.  "_dev" collectives take device pointers and are asynchronous
 * on `stream` with RCCL; the others take host pointers and block.  count = elements PER RANK; recv of an all-gather
 * holds world * count elements in rank order.  dtype LSPIV_F32 / LSPIV_F64; op LSPIV_COMM_SUM / LSPIV_COMM_MAX. */
#define LSPIV_COMM_RCCL 0
#define LSPIV_COMM_SHM 1
#define LSPIV_COMM_SUM 0
#define LSPIV_COMM_MAX 1
#define LSPIV_COMM_ID_BYTES 128
typedef struct lspiv_comm lspiv_comm;
int lspiv_comm_unique_id(int transport, void* id /* LSPIV_COMM_ID_BYTES */);
int lspiv_comm_init(int rank, int world, const void* id, int transport, lspiv_comm** comm);
/* backend_ranks: the rank count the transport itself reports (ncclCommCount / attached shm ranks) */
int lspiv_comm_info(lspiv_comm* comm, int* rank, int* world, int* transport, int* backend_ranks);
int lspiv_comm_allgather_dev(lspiv_comm* comm, const void* d_send, void* d_recv, int64_t count, int dtype, void* stream);
int lspiv_comm_allreduce_dev(lspiv_comm* comm, const void* d_send, void* d_recv, int64_t count, int dtype, int op,
                             void* stream);
int lspiv_comm_allgather(lspiv_comm* comm, const void* send, void* recv, int64_t count, int dtype);
int lspiv_comm_allreduce(lspiv_comm* comm, const void* send, void* recv, int64_t count, int dtype, int op);
int lspiv_comm_barrier(lspiv_comm* comm);
int lspiv_comm_destroy(lspiv_comm* comm);

/* ---------------------------------------------------------------- device-resident helpers  */
/* For hosts that keep stacks in HBM (bench.py, one-process-per-GPU shards).                 */
int lspiv_dev_malloc(void** d_ptr, size_t bytes);
int lspiv_dev_free(void* d_ptr);
/* pinned host memory: a uint8 / float32 stack that lives in it is DMA'd in place by lspiv_piv_pairs (no staging copy). */
int lspiv_host_alloc(void** h_ptr, size_t bytes);
int lspiv_host_free(void* h_ptr);
int lspiv_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int lspiv_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int lspiv_memset_dev(void* d_ptr, int value, size_t bytes);
/* HIP events recorded on the library's launch stream (bench.py's live kernel timing). */
int lspiv_event_create(void** ev);
int lspiv_event_record(void* ev);
int lspiv_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises ev_stop */
int lspiv_event_destroy(void* ev);
/* extra HIP streams for hosts that overlap the result exchange with the next launch (bench.py --gpus N): every "_dev"
 * entry point takes such a handle; events recorded on one stream can be waited for on another. */
int lspiv_stream_create(void** stream);
/* the same with a scheduling priority: > 0 the device's highest, < 0 its lowest, 0 = lspiv_stream_create.  pyorc_amd.shard puts the
 * result exchange on a HIGH-priority stream: RCCL's few workgroups must find a compute unit while a PIV kernel of ~80 000
 * workgroups is draining through all of them on the other stream. */
int lspiv_stream_create_priority(void** stream, int priority);
int lspiv_stream_destroy(void* stream);
/* a stream the CALLER created (hipStreamCreate) and passed to "_dev" entry points: free what the library keeps for it (the
 * rescue lists and their counters); NULL = the library's own stream.  lspiv_stream_destroy does this for its own streams. */
int lspiv_stream_release(void* stream);
int lspiv_stream_synchronize(void* stream);             /* NULL = the library's launch stream */
int lspiv_event_record_on(void* ev, void* stream);      /* NULL = the library's launch stream */
int lspiv_stream_wait_event(void* stream, void* ev);    /* NULL = the library's launch stream */

/* Synthetic particle-image stack rendered directly into HBM (SURVEY.md section 8d workload; test and
 * bench utility, not on the PIV path): N_p = density*H*W Gaussian particles (sigma 1.2 px)
 * advected by u = 3 + 2 sin(2 pi y/H), v = 1.5 cos(2 pi x/W) px/frame.  d_frames (T,H,W) uint8. */
int lspiv_synth_particles_dev(void* d_frames, int64_t T, int64_t H, int64_t W, uint64_t seed, float density);
/* test hook, host only: the float64 -> float32 conversion the host entry points apply while staging (csrc/host_stage.cpp), with
 * the DC-offset rule of the "narrow_offset" option at threshold min_abs (-1: plain conversion); offsets (nullable) receives the
 * offset taken off every frame; returns the number of staging threads. */
int lspiv_debug_narrow(const double* frames, int64_t frame_elems, int64_t n_frames, int min_abs, float* out, double* offsets);

/* Test hook: `count` independent length-n complex FFTs with the kernels' own register transforms (fft_regs.h), numpy
 * conventions (forward exp(-2 pi i jk/n), inverse exp(+...), both unnormalised); in / out: host arrays of count*n
 * interleaved (re, im) float pairs; n = 8, 16, 32, 64 or any even length 6..62 (the sizes lspiv_kernel_kind maps to 6 / 8). */
int lspiv_debug_fft(int n, int inverse, const float* in, float* out, int64_t count);
/* The same with the twiddle path of n = 16, 32, 64 chosen by name: form 0 = what the kernels use (lspiv_debug_fft), 1 = twiddles as
 * separate complex multiplies, 2 = twiddle scales folded into the next butterfly level, 4 = conjugate-pair split radix (fft_regs.h;
 * one bit per form, so 3 is none).  Other n with form 1 / 2 / 4, or another form: LSPIV_EUNSUPPORTED. */
int lspiv_debug_fft_form(int n, int form, int inverse, const float* in, float* out, int64_t count);
/* Test hook: the 32-lane reductions of the kernels (csrc/common.h) on `count` whole waves of 64 lanes; in / out: host arrays of count * 64
 * 32-bit words, out[l] = what lane l holds after the reduction over its 32-lane half.  op 0 = float sum (bits), 1 = integer sum, 2 =
 * signed minimum, 3 = signed maximum (what the maxima of the clipped planes are taken with); form 0 = the two 16-lane rows joined through
 * ds_swizzle, 1 = through v_permlane16_swap ("lds_light"), 2 / 3 (integer ops) = the paired reduction of "lds_light" on (the lane's value,
 * the value of the same lane of the other half): 2 returns the first result, 3 the second -- which is what the other half's lanes hold
 * after forms 0 and 1.  Another op or form: LSPIV_EUNSUPPORTED. */
int lspiv_debug_half_reduce(int op, int form, const uint32_t* in, uint32_t* out, int64_t count);
/* Test hook: the first-match search of the 32 x 32 peak search on `count` whole waves; in: count * 64 flags (non-zero = the lane matches),
 * out[l] = the smallest shifted index (lane + 16) & 31 among the matching lanes of lane l's 32-lane half, 1 << 12 where there is none.
 * form 0 = DPP arg-min, 1 = ballot and bit scan ("scalar_epilogue"), 2 = the paired DPP chain of "lds_light".  Another form:
 * LSPIV_EUNSUPPORTED. */
int lspiv_debug_first_match(int form, const uint32_t* in, uint32_t* out, int64_t count);
/* Test hook (host only): how the time-walking kernels cut a chunk of n_pairs pairs that starts at absolute pair index
 * pair_offset into segments of seg_len pairs anchored at multiples of seg_len: pairs in the first segment, segment count. */
int lspiv_debug_segments(int64_t n_pairs, int64_t pair_offset, int seg_len, int64_t* seg_first, int64_t* n_seg);
/* Test hook: the rescue lists the LAST per-timestep launch on `stream` (NULL: the library's own) left behind, after synchronising with it.
 * counts[0 .. 1] = "fit" / "amb" records of that launch; the first min(count, cap) of them are copied: a "fit" record is four words
 * (result index inside the launch, ip << 16 | jp, the other arg-max candidate or ~0, 0), an "amb" record the result index.  The order of
 * a list is whatever the kernel's waves made it. */
int lspiv_debug_rescue_lists(void* stream, uint32_t* fit, int64_t cap_fit, uint32_t* amb, int64_t cap_amb, int64_t* counts);
/* Test hook (host only): the column-to-lane map of the 32 x 32 walking kernels under "unpack_dpp", as the kernels compile it.  For
 * 0 <= i < 32: *col = the column lane i holds (compile-time form), *col_rt = the same from the branch-free run-time form the second
 * transpose uses, *lane = the lane that holds column i.  LSPIV_EINVAL outside the range. */
int lspiv_debug_unpack_map(int i, int* col, int* col_rt, int* lane);

/* Measurement (round 5): with lspiv_set_option("time_kernel", 1) every launch records HIP events on its own stream right before and
 * right after its PIV kernel(s) -- not around the rescue kernels that follow.  lspiv_kernel_times returns the durations [ms] of the
 * last *n <= min(cap, 16) launches of the calling thread's device, oldest first, and empties the ring: the dominant kernel's time
 * inside the launch as a caller issues it, which is what `rocprofv3 --kernel-trace` reports for that kernel (bench.py:
 * roofline.achieved). */
int lspiv_kernel_times(float* ms, int cap, int* n);

/* Measurement / tests (round 6): lspiv_trace(1) makes the library record HIP event pairs -- on the streams the work runs on --
 * around the spans below, lspiv_trace(0) stops and forgets them; lspiv_trace_read returns up to `cap` of the *n recorded spans of the
 * calling thread's device, in recording order, as milliseconds since lspiv_trace(1) (it synchronises the device first).
 *   LSPIV_TRACE_PIV_HOST      one host-pointer PIV call (lspiv_piv_pairs[_at], lspiv_piv_velocity_at): from before its first kernel
 *                             to after its last download;
 *   LSPIV_TRACE_PROJECT_HOST  the projection kernel(s) of one host-pointer projection call (lspiv_project_frames[_u8],
 *                             lspiv_project_cv_frames), between its upload and its download.
 * A projection span that starts inside a PIV span shows what a wall clock cannot: the two calls, issued by two host threads on one
 * device, overlapped on the GPU (they share neither lock, nor stream, nor workspaces since round 6). */
#define LSPIV_TRACE_PIV_HOST 0
#define LSPIV_TRACE_PROJECT_HOST 1
int lspiv_trace(int enable);
int lspiv_trace_read(int64_t cap, int32_t* kind, double* start_ms, double* end_ms, int64_t* n);

/* Test hook (round 6): the orthoprojection kernel for plans with group means computes float(sum) / float(count) as q = RN(s y),
 * q' = RN(q + (s - q c) y) with y = RN(1 / c) instead of the division sequence; *mismatches = the number of (s, c), 0 <= s <= 255 c,
 * 1 <= c <= 255 -- every sum of c uint8 samples --, for which that differs from s / c on the device (must be 0). */
int lspiv_debug_project_division(int* mismatches);

/* Test hook (host only, no HIP call): hold one of device `device`'s locks -- 0 the host-pointer PIV entry points' workspaces, 1 a launch
 * and its rescue kernels, 2 the rescue lists, 3 / 4 the two slots of the host-pointer projection entry points -- for `milliseconds`.  The locks are per device (round 5; process-wide before): two
 * threads holding the same lock of two devices overlap, of one device queue.  tests/test_host.py times exactly that. */
int lspiv_debug_hold_lock(int device, int which, int milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* LSPIV_H */
