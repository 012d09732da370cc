"""Float64 numpy reference of the per-window frame lag, multi-frame PIV: the lagged pass, the clip at the end
of the stack, the integer lag predictor and the adaptive form, plus the inputs the host and GPU tests share.  Composed of the oracle's own
pieces (sliding_window_stack, ncc, signal_mask, u_v_displacement) exactly as tests/multipass_ref.py composes its shifted pass: the lagged
pass IS ``multipass_ref.shifted_piv`` with window B cut from ``imgs[t + k]`` and the displacement divided by k.  Like the rest of the PIV
path it is this project's reading: unpinned against a real ffpiv.

Kernel orientation throughout (u column shift, v row shift, rows downward); SEMANTICS["v_sign"] is applied once, to the result."""
import functools
import warnings

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd import synth
from tests import ensemble_multipass_ref as emp
from tests import multipass_ref as mp

LAG_WINDOWS = (16, 32, 64)
MAX_LAG = 16


def clip_lags(lag, n_frames):
    """``lag`` (P, rows, cols) clamped to 1 .. 16 and clipped to the end of a stack of ``n_frames`` frames: k[t] <= n_frames - 1 - t."""
    lag = np.clip(np.asarray(lag, dtype=np.int64), 1, MAX_LAG)
    left = n_frames - 1 - np.arange(lag.shape[0])
    return np.minimum(lag, np.maximum(left, 1)[:, None, None])


def table(pair_step, n_frames, n_pairs, grid):
    """The effective lags (n_pairs, rows, cols) of a whole number or of a per-window array."""
    k = np.asarray(pair_step, dtype=np.int64)
    return clip_lags(np.broadcast_to(k if k.ndim == 0 else k[None], (n_pairs, *grid)), n_frames)


def lagged_piv(imgs, n, overlap, lag, shift=None, signal_threshold=None, n_pairs=None):
    """One lagged pass over the first ``n_pairs`` pairs (default: all T - 1) of ``imgs``.  ``lag`` (n_pairs, rows, cols): the lags, clipped
    here to the frames left; ``shift`` (n_pairs, rows, cols, 2) {dy, dx} or None.  dict(u, v, corr, s2n (P, rows, cols), planes (P, n_win,
    n, n), tie, lag = the EFFECTIVE lags, shift = the CLAMPED offsets).  A = window of frame t at (y0, x0), B = window of frame t + k at
    (y0 + dy, x0 + dx); u = (dx + residual) / k, v = (dy + residual) / k."""
    imgs = np.asarray(imgs)
    T, H, W = imgs.shape
    P = T - 1 if n_pairs is None else int(n_pairs)
    if po.SEMANTICS["signal_mode"] == 1 or not po.SEMANTICS["norm_clip"]:
        raise NotImplementedError("a frame lag: signal_mode = 1 and norm_clip = 0 are not supported")
    ov = mp.overlap_pair(overlap)
    y0, x0 = mp.grid_origins((H, W), n, overlap)
    rows, cols = len(y0), len(x0)
    k = clip_lags(np.asarray(lag).reshape(P, rows, cols), T)
    if shift is None:
        shift = np.zeros((P, rows, cols, 2), dtype=np.int64)
    sh = mp.clamp_shift(np.asarray(shift).reshape(P, rows, cols, 2), (H, W), n, overlap)
    stack = po.sliding_window_stack(imgs, (n, n), ov)                                      # (T, n_win, n, n)
    planes = np.full((P, rows * cols, n, n), np.nan)
    ar = np.arange(n)
    for t in range(P):
        by = (y0[:, None] + sh[t, :, :, 0]).reshape(-1)                                    # (n_win,)
        bx = (x0[None, :] + sh[t, :, :, 1]).reshape(-1)
        fr = t + k[t].reshape(-1)                                                          # the frame of every window's B
        B = imgs[fr[:, None, None], (by[:, None] + ar[None, :])[:, :, None], (bx[:, None] + ar[None, :])[:, None, :]]
        A = stack[t]
        keep = po.signal_mask(A, B, signal_threshold)
        if keep.any():
            planes[t, keep] = po.ncc(A[keep], B[keep])
    with po.semantics(v_sign=0):
        u, v = po.u_v_displacement(planes, rows, cols)
    u = (u + sh[..., 1]) / k
    v = (v + sh[..., 0]) / k
    if po.SEMANTICS["v_sign"]:
        v = -v
    shape = (P, rows, cols)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN planes (windows below the signal threshold)
        cm = np.nanmax(planes, axis=(-2, -1))
        s2n = cm / np.nanmean(planes, axis=(-2, -1))
    top = np.sort(planes.reshape(planes.shape[:2] + (-1,)), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        tie = ((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (cm > 0)
    return dict(u=u, v=v, corr=cm.reshape(shape), s2n=s2n.reshape(shape), planes=planes, tie=tie.reshape(shape), lag=k, shift=sh)


def target128(n, target=None):
    """rint(128 * target); the default target is the quarter rule, n / 4 px."""
    return int(np.rint(128.0 * (n / 4 if target is None else float(target))))


def predict_lag(u, v, dim_size, n, overlap, n_frames, k_max=4, target=None, clamp=True):
    """The integer lag predictor: (u, v) (P, rows, cols) of a lag-1 pass (kernel orientation) of a stack of ``n_frames`` frames ->
    (lag (P, rows, cols) uint8, shift (P, rows, cols, 2) int16 {dy, dx}, clamped to the frame unless ``clamp`` is off: int64 then).  Exact
    integers after the rint."""
    H, W = dim_size
    y0, x0 = mp.grid_origins(dim_size, n, overlap)
    u = np.asarray(u, dtype=np.float32).reshape(-1, len(y0), len(x0))
    v = np.asarray(v, dtype=np.float32).reshape(-1, len(y0), len(x0))
    t128 = target128(n, target)
    lim = 32767 * 64
    lag = np.empty(u.shape, dtype=np.int64)
    out = np.empty(u.shape + (2,), dtype=np.int64)
    for p in range(u.shape[0]):
        valid = np.isfinite(u[p]) & np.isfinite(v[p])
        with np.errstate(invalid="ignore", over="ignore"):
            # rint: half to even, in float32 (the product by 64 is exact, or infinite); clamped to +-32767 * 64
            qu = np.clip(np.where(valid, np.rint(np.float32(64) * u[p]), 0), -lim, lim).astype(np.int64)
            qv = np.clip(np.where(valid, np.rint(np.float32(64) * v[p]), 0), -lim, lim).astype(np.int64)
        m2u, m2v = mp._median2(qu, valid), mp._median2(qv, valid)                          # 1 / 128 px
        mag = np.maximum(np.abs(m2u), np.abs(m2v))
        k = np.clip(t128 // np.maximum(mag, 1), 1, k_max)
        k = np.minimum(k, max(n_frames - 1 - p, 1))
        lag[p] = k
        out[p, :, :, 1] = np.floor_divide(k * m2u + 64, 128)
        out[p, :, :, 0] = np.floor_divide(k * m2v + 64, 128)
    return lag.astype(np.uint8), mp.clamp_shift(out, dim_size, n, overlap).astype(np.int16) if clamp else out


def adaptive(imgs, n, overlap, k_max=4, target=None, signal_threshold=None, n_pairs=None):
    """``pair_step="adaptive"``: pass 0 (the plain pass at lag 1, kernel orientation), the predictor, the lagged pass.  The lagged pass's
    dict plus ``pass0``."""
    imgs = np.asarray(imgs)
    P = imgs.shape[0] - 1 if n_pairs is None else int(n_pairs)
    with po.semantics(v_sign=0):
        p0 = mp.shifted_piv(imgs[:P + 1], n, overlap, None, signal_threshold)
    lag, shift = predict_lag(p0["u"], p0["v"], imgs.shape[1:], n, overlap, imgs.shape[0], k_max, target)
    return dict(lagged_piv(imgs, n, overlap, lag, shift, signal_threshold, P), pass0=p0)


# ---- the parity inputs (tests/test_lag_host.py checks them on the CPU, tests/test_gpu_lag.py runs them) ---------------------------------------
# the pass stacks of the multi-pass tests at 7 frames: 16 @ 8 on 48 x 53, 32 @ 16 on 96 x 131, 64 @ 32 on 160 x 200, a uniform (3, -2) px/frame
PASS_CASES = emp.PASS_CASES
PASS_T = 7
PASS_DTYPES = (np.uint8, np.float32, np.float64)
INT_LAG = 3
SIGNAL_THR = emp.SIGNAL_THR
# adaptive form per window size: (pair_step_max, pair_step_target).  The stacks move 3 px per frame, so the targets are chosen above the
# quarter rule where that would leave every lag at 1 (16 px: n / 2 = 8 px, the largest the keyword takes).  32 px: at K = 4 one window's
# median v of -1.875 px/frame puts 4 v on a rounding boundary of the offset, within the GPU's 1e-4 of its lag-1 field (found by
# tests/test_lag_host.py); at K = 3 no window is that close
ADAPTIVE = {16: (4, 8.0), 32: (3, 16.0), 64: (4, None)}


def pass_stack(n, dtype=np.uint8):
    return emp.pass_stack(n, PASS_T, dtype)


def grid_shape(n):
    return emp.grid_shape(n)


@functools.lru_cache(maxsize=None)
def window_lags(n):
    """A per-window array with the lags 1 .. 4, every one of them present."""
    rows, cols = grid_shape(n)
    rng = np.random.default_rng(700 + n)
    a = rng.integers(1, 5, (rows, cols)).astype(np.int64)
    a.reshape(-1)[:4] = (1, 2, 3, 4)
    return a


@functools.lru_cache(maxsize=None)
def parity_ref(n, form, dtype=np.uint8, signal=False):
    """The reference of one parity input: form "int" (a lag of 3), "array" (window_lags) or "adaptive" (ADAPTIVE[n])."""
    m, ov, dim = PASS_CASES[n]
    a = (signal_stack(n) if signal else pass_stack(n, dtype)).astype(np.float64)
    thr = SIGNAL_THR if signal else None
    if form == "adaptive":
        return adaptive(a, m, ov, *ADAPTIVE[n], signal_threshold=thr)
    lag = table(INT_LAG if form == "int" else window_lags(n), PASS_T, PASS_T - 1, grid_shape(n))
    return lagged_piv(a, m, ov, lag, None, thr)


def parity_kw(n, form):
    """The keywords of ``piv.piv_pairs_lagged`` for a parity input."""
    if form == "adaptive":
        return dict(pair_step="adaptive", pair_step_max=ADAPTIVE[n][0], pair_step_target=ADAPTIVE[n][1])
    return dict(pair_step=INT_LAG if form == "int" else window_lags(n))


@functools.lru_cache(maxsize=None)
def signal_stack(n):
    """Samples below 40 set to zero, the upper left quarter of every frame and the right third of frame 4 empty: the threshold takes out
    some windows, and whether a window of pair t is kept depends on WHICH frame its window B is cut from."""
    a = pass_stack(n).copy()
    a[a < 40] = 0
    a[:, :a.shape[1] // 2, :a.shape[2] // 2] = 0
    a[4, :, 2 * a.shape[2] // 3:] = 0
    return a


# ---- a caller's table and offsets (LSPIV_LAG_TABLE with d_shift: reachable from C only) ----------------------------------------------------
TABLE_PAIRS = 4          # of the 6 pairs of a 7-frame pass stack: the frames behind them are the call's halo


@functools.lru_cache(maxsize=None)
def table_case(n):
    """(raw table (4, rows, cols) uint8 -- lags 1 .. 3, and a 0 and a 200 the library clamps to 1 and to the frames left --, raw offsets (4,
    rows, cols, 2) int16 {dy, dx}: lag times the stack's displacement plus a scatter of +-1 px, and a few that point out of the frame)."""
    rows, cols = grid_shape(n)
    rng = np.random.default_rng(900 + n)
    lag = rng.integers(1, 4, (TABLE_PAIRS, rows, cols)).astype(np.uint8)
    sh = np.empty((TABLE_PAIRS, rows, cols, 2), dtype=np.int16)
    sh[..., 0] = lag.astype(np.int64) * emp.PASS_SHIFT[1] + rng.integers(-1, 2, lag.shape)
    sh[..., 1] = lag.astype(np.int64) * emp.PASS_SHIFT[0] + rng.integers(-1, 2, lag.shape)
    lag[0, 0, 0], lag[1, -1, -1] = 0, 200
    sh[2, 0, :, 0] = -300
    sh[3, :, -1, 1] = 32767
    return lag, sh


@functools.lru_cache(maxsize=None)
def table_ref(n):
    m, ov, _ = PASS_CASES[n]
    lag, sh = table_case(n)
    return lagged_piv(pass_stack(n).astype(np.float64), m, ov, lag, sh, None, TABLE_PAIRS)


# ---- small and odd grids: a job count that is no multiple of the jobs per block (4 x 5 windows x 5 pairs at 32 px: 100 jobs, 8 per block),
# one row, one window ----------------------------------------------------------------------------------------------------------------------
SMALL_GRIDS = {"odd job count": (32, 16, (80, 99)), "one row": (16, 8, (20, 131)), "one window": (64, 32, (70, 75)), "one window 16": (16, 8, (16, 16))}
SMALL_T, SMALL_K = 6, 5


@functools.lru_cache(maxsize=None)
def small_stack(name):
    n, _, dim = SMALL_GRIDS[name]
    return synth.particle_stack(SMALL_T, dim[0], dim[1], seed=31 + n, density=0.05, uniform_shift=(0.8, -0.5))


def small_lags(name):
    """A per-window array of lags 1 .. 4 in window order."""
    n, ov, dim = SMALL_GRIDS[name]
    rows, cols = (len(q) for q in mp.grid_origins(dim, n, ov))
    return (np.arange(rows * cols).reshape(rows, cols) % 4 + 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def small_ref(name, form):
    n, ov, dim = SMALL_GRIDS[name]
    a = small_stack(name).astype(np.float64)
    if form == "adaptive":
        return adaptive(a, n, ov, SMALL_K)
    arr = small_lags(name)
    return lagged_piv(a, n, ov, table(arr, SMALL_T, SMALL_T - 1, arr.shape))


# ---- the predictor on hand-made fields ---------------------------------------------------------------------------------------------------
HAND_DIM, HAND_N, HAND_OV, HAND_T = (96, 131), 16, 8, 6          # an 11 x 15 grid, 5 pairs: the last pairs are clipped


@functools.lru_cache(maxsize=None)
def hand_fields():
    """(u, v) (5, 11, 15) float32: a slow-to-fast profile with scatter; a NaN neighbourhood (a whole 3 x 3 block, and isolated NaN / inf
    entries in u or in v alone); exact zeros (mag = 0); vectors on .5 / 64 px (rint half to even); large vectors at the grid's edges, where
    the frame clamp changes the offset; a huge finite vector (the clamp of q)."""
    rows, cols = (len(q) for q in mp.grid_origins(HAND_DIM, HAND_N, HAND_OV))
    rng = np.random.default_rng(77)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    u = np.empty((HAND_T - 1, rows, cols), dtype=np.float32)
    v = np.empty_like(u)
    for p in range(HAND_T - 1):
        u[p] = 0.1 + 3.0 * (rr / (rows - 1)) ** 2 + rng.normal(0, 0.05, (rows, cols))
        v[p] = -0.6 * np.sin(np.pi * cc / cols) + rng.normal(0, 0.05, (rows, cols))
    u[0, 3:6, 4:7] = np.nan                    # an empty neighbourhood at (4, 5)
    v[0, 3:6, 4:7] = np.nan
    u[1, 0, 0] = np.nan                        # a corner: 3 valid neighbours
    v[1, 5, 14] = np.inf                       # an edge, v alone
    u[1, 7, 7] = -np.inf
    u[2, :2, :] = 0.0                          # mag = 0 in the first row
    v[2, :2, :] = 0.0
    u[2, 8, 3:6] = (0.5 / 64, 1.5 / 64, 2.5 / 64)
    v[2, 8, 3:6] = (-0.5 / 64, -1.5 / 64, -2.5 / 64)
    u[3, :, :2] = -1.9                         # the left columns move out of the frame (two of them: the median follows): dx clamped to 0 at the edge
    u[3, :, -2:] = 2.2                         # the right columns likewise
    v[3, :2, :] = -1.2                         # the top rows
    v[0, -2:, :] = 1.7                         # the bottom rows
    u[4, 2, 2] = 3.0e9                         # q clamped to 32767 * 64
    v[4, 9, 9] = -7.0e5
    return u, v


# ---- the benefit on a gentle river profile ------------------------------------------------------------------------------------------------
PROFILE_DIM, PROFILE_T, PROFILE_SEED, PROFILE_DENSITY, PROFILE_NOISE = (256, 160), 12, 4, 0.02, 6.0
PROFILE_K, PROFILE_SLOW, PROFILE_TAIL = 8, 0.6, 8            # lags up to 8; slow: truth < 0.6 px/frame; the last 8 pairs are left out
PROFILE_CASES = ((32, 16), (16, 8))
# slow-window median |error| in px per frame interval as this reference measures it: {(n, overlap): (lag 1, adaptive)}, ratios 0.21 and
# 0.18 (tests/test_lag_host.py holds the reference to these within 1 % and asserts the gate adaptive <= 0.5 * lag 1)
PROFILE_MEDIANS = {(32, 16): (0.02232, 0.004648), (16, 8): (0.04294, 0.007686)}


def profile_u(y):
    """u(y) = 0.15 + 2.4 smoothstep((y - 96) / 128) px/frame, v = 0: slow water near one bank, several pixels per frame mid-channel."""
    s = np.clip((np.asarray(y, dtype=np.float64) - 96.0) / 128.0, 0.0, 1.0)
    return 0.15 + 2.4 * s * s * (3.0 - 2.0 * s)


@functools.lru_cache(maxsize=None)
def profile_stack():
    """12 uint8 frames 256 x 160: Gaussian particles (pyorc_amd.synth's blobs) advected by profile_u, re-seeded when they leave, plus
    white noise of sigma 6 grey levels per frame."""
    H, W = PROFILE_DIM
    rng = np.random.default_rng(PROFILE_SEED)
    n_p = int(PROFILE_DENSITY * H * W)
    py, px, amp = rng.uniform(0, H, n_p), rng.uniform(0, W, n_p), rng.uniform(120.0, 255.0, n_p)
    out = np.empty((PROFILE_T, H, W), dtype=np.uint8)
    for t in range(PROFILE_T):
        img = synth._render(H, W, py, px, amp) + rng.normal(0.0, PROFILE_NOISE, (H, W))
        out[t] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        px = px + profile_u(py)
        gone = px >= W + synth.RADIUS
        px[gone] -= W + 2 * synth.RADIUS           # re-enter on the left at the same y with a new brightness
        amp[gone] = rng.uniform(120.0, 255.0, int(gone.sum()))
    return out


def profile_truth(n, overlap):
    """(u_true (rows, cols), slow (rows, cols) bool) at the window centres."""
    y0, x0 = mp.grid_origins(PROFILE_DIM, n, overlap)
    ut = np.broadcast_to(profile_u(y0 + (n - 1) / 2.0)[:, None], (len(y0), len(x0)))
    return ut, ut < PROFILE_SLOW


def slow_median_error(u, v, n, overlap):
    """Median over the slow windows of the pairs before the tail of the vector error |(u, v) - truth| in px per frame interval."""
    ut, slow = profile_truth(n, overlap)
    P = PROFILE_T - 1 - PROFILE_TAIL
    err = np.hypot(np.asarray(u)[:P] - ut[None], np.asarray(v)[:P])
    return float(np.nanmedian(err[:, slow]))


@functools.lru_cache(maxsize=None)
def profile_ref(n, overlap, adaptive_form):
    a = profile_stack().astype(np.float64)
    with po.semantics(v_sign=0):
        if adaptive_form:
            return adaptive(a, n, overlap, PROFILE_K)
        return mp.shifted_piv(a, n, overlap)
