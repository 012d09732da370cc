"""Float64 numpy reference of the multi-pass ensemble: the shifted ensemble pass and the chain.  Composed of
``tests/multipass_ref.py`` (``shifted_piv`` with ONE offset field broadcast over the pairs, ``predict_shift``) and the ensemble steps of
``oracle.piv_oracle.get_ffpiv`` (oracle/piv_oracle.py:407-445), both left as they are.  Like the rest of the PIV path it is this
project's reading: unpinned against a real ffpiv.

Also the inputs of tests/test_gpu_ensemble_multipass.py and their references, computed once per process and shared with the CPU checks
of those inputs (tests/test_ensemble_multipass_host.py).  Everything between the passes is in the kernels' orientation (u column shift,
v row shift, rows downward); SEMANTICS["v_sign"] is applied once, to the last pass of a chain."""
import functools
import warnings

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd.synth import particle_stack
from tests import multipass_ref as mp

DEFAULT_KW = dict(corr_min=0.2, s2n_min=3.0, count_min=0.2)     # the ensemble's default masks
KW = dict(corr_min=0.1, s2n_min=1.5, count_min=0.2)             # lowered: most planes of a dense stack are kept
OPEN_KW = dict(corr_min=0.0, s2n_min=0.5, count_min=0.2)        # masks that keep every plane (s2n >= 1 by construction): for windows that
                                                                # correlate with unrelated image content, whose s2n crowds around 1.4
KWS = {"KW": KW, "DEFAULT": DEFAULT_KW, "OPEN": OPEN_KW}


def ensemble_pass(imgs, n, overlap, shift=None, corr_min=0.2, s2n_min=3.0, count_min=0.2, n_frames=1, signal_threshold=None):
    """One (shifted) ensemble pass over all pairs of ``imgs``.  ``shift``: (rows, cols, 2) {dy, dx} or None (zeros), the same for every
    pair.  dict(u, v, corr, s2n (1, rows, cols), count (n_win,), planes (1, n_win, n, n) = the mean planes, shift = the CLAMPED offsets
    (rows, cols, 2), tie (1, rows, cols), pair_corr, pair_s2n (P, n_win) = the per-pair values BEFORE the masks); u, v in the kernels'
    orientation.  ``n_frames``: what the count filter multiplies ``count_min`` with (the reference's number of chunks, quirk Q3)."""
    imgs = np.asarray(imgs)
    P = imgs.shape[0] - 1
    rows, cols = (len(q) for q in mp.grid_origins(imgs.shape[1:], n, overlap))
    sh = None if shift is None else np.broadcast_to(np.asarray(shift).reshape(1, rows, cols, 2), (P, rows, cols, 2))
    with po.semantics(v_sign=0):
        r = mp.shifted_piv(imgs, n, overlap, sh, signal_threshold)
    corr = r["planes"].copy()                                                   # (P, n_win, n, n)
    pair_cm, pair_sn = r["corr"].reshape(P, -1).copy(), r["s2n"].reshape(P, -1).copy()
    cm, sn = pair_cm.copy(), pair_sn.copy()
    with np.errstate(invalid="ignore"):
        masks = (cm >= corr_min) & (sn >= s2n_min) & np.isfinite(cm)
    corr[~masks] = 0.0
    cm[~masks] = 0.0
    sn[~masks] = 0.0
    corr_sum = corr.sum(axis=0, keepdims=True)
    corr_count = (cm > 1e-6).sum(axis=0, keepdims=True)                         # (1, n_win)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", category=RuntimeWarning)
        low = corr_count < count_min * n_frames
        corr_sum[low] = np.nan
        cm[:, low.flatten()] = np.nan
        mean = corr_sum / corr_count[..., None, None]
        corr_mean = np.nanmean(cm, axis=0).reshape(1, rows, cols)
        s2n_mean = np.nanmean(sn, axis=0).reshape(1, rows, cols)
    with po.semantics(v_sign=0):
        u, v = po.u_v_displacement(mean, rows, cols)
    clamped = r["shift"][0]
    u = u + clamped[None, :, :, 1]
    v = v + clamped[None, :, :, 0]
    top = np.sort(mean.reshape(1, rows * cols, -1), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        tie = (((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (top[..., 1] > 0)).reshape(1, rows, cols)
    return dict(u=u, v=v, corr=corr_mean, s2n=s2n_mean, count=corr_count.reshape(-1).astype(np.float64), planes=mean, shift=clamped, tie=tie,
                pair_corr=pair_cm, pair_s2n=pair_sn)


def ensemble_multipass(imgs, passes, corr_min=0.2, s2n_min=3.0, count_min=0.2, n_frames=1, signal_threshold=None):
    """The chain: a list of per-pass dicts (:func:`ensemble_pass`; shift of pass 0 all zero) in the kernels' orientation, except that the
    LAST pass's v carries SEMANTICS["v_sign"]."""
    imgs = np.asarray(imgs)
    dim = imgs.shape[1:]
    out = []
    for k, (n, ov) in enumerate(passes):
        if k and n not in mp.SHIFT_WINDOWS:
            raise ValueError(f"pass {k}: window {n} not in {mp.SHIFT_WINDOWS}")
        shift = None if k == 0 else mp.predict_shift(out[-1]["u"], out[-1]["v"], dim, passes[k - 1], (n, ov))[0]
        out.append(ensemble_pass(imgs, n, ov, shift, corr_min, s2n_min, count_min, n_frames, signal_threshold))
    if po.SEMANTICS["v_sign"]:
        out[-1] = dict(out[-1], v=-out[-1]["v"])
    return out


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------
TRUTH = (9.3, -6.4)                       # (u, v) = (dx, dy) of the sparse river stack
CHAIN_FINAL = (16, 8)
CHAINS = {"64": [(64, 32), CHAIN_FINAL], "64-32": [(64, 32), (32, 16), CHAIN_FINAL]}


@functools.lru_cache(maxsize=None)
def river_stack():
    """The stack of the issue: sparse seeding, a uniform displacement well beyond a quarter of the final 16 px window."""
    return particle_stack(7, 160, 200, seed=5, density=0.012, uniform_shift=TRUTH)


@functools.lru_cache(maxsize=None)
def river_chain(name):
    return ensemble_multipass(river_stack(), CHAINS[name], **DEFAULT_KW)


@functools.lru_cache(maxsize=None)
def river_plain():
    return ensemble_pass(river_stack(), 16, 8, None, **DEFAULT_KW)


def within_half_px(r):
    """Share of ALL windows of a pass within 0.5 px of the truth (NaN windows count as misses)."""
    with np.errstate(invalid="ignore"):
        return float(((np.abs(r["u"] - TRUTH[0]) <= 0.5) & (np.abs(r["v"] - TRUTH[1]) <= 0.5)).mean())


# (n, overlap, (H, W)): a few windows per side with a ragged edge (the shapes of test_gpu_multipass.py's SHIFT_CASES)
PASS_CASES = {16: (16, 8, (48, 53)), 32: (32, 16, (96, 131)), 64: (64, 32, (160, 200))}
PASS_DTYPES = (np.uint8, np.float32, np.float64)
PASS_FRAMES = (6, 7)                      # 5 and 6 pairs: a lone last pair and the even case
PASS_SHIFT = (3, -2)                      # the stack's uniform displacement (dx, dy); the hand-made offsets scatter around it


def as_samples(a, dtype):
    """uint8 as drawn; floats signed, through an affine map (the same normalised windows)."""
    return a if dtype == np.uint8 else a.astype(dtype) * dtype(0.37) - dtype(11.0)


@functools.lru_cache(maxsize=None)
def pass_stack(n, T=7, dtype=np.uint8):
    _, _, (H, W) = PASS_CASES[n]
    return as_samples(particle_stack(7, H, W, seed=20 + n, density=0.05, uniform_shift=(float(PASS_SHIFT[0]), float(PASS_SHIFT[1])))[:T], dtype)


def grid_shape(n):
    m, ov, dim = PASS_CASES[n]
    return tuple(len(q) for q in mp.grid_origins(dim, m, ov))


@functools.lru_cache(maxsize=None)
def hand_shift(n):
    """A hand-made offset field: the true displacement plus a different small offset per window (so every window's B is cut somewhere
    else), clamped at the edge windows so that all of it is inside the frame."""
    rows, cols = grid_shape(n)
    rng = np.random.default_rng(100 + n)
    sh = np.empty((rows, cols, 2), dtype=np.int16)
    sh[..., 0] = PASS_SHIFT[1] + rng.integers(-2, 3, (rows, cols))
    sh[..., 1] = PASS_SHIFT[0] + rng.integers(-2, 3, (rows, cols))
    m, ov, dim = PASS_CASES[n]
    return mp.clamp_shift(sh, dim, m, ov).astype(np.int16)


@functools.lru_cache(maxsize=None)
def pass_ref(n, T=7, dtype=np.uint8, shift="hand", kw="KW", signal_threshold=None):
    m, ov, _ = PASS_CASES[n]
    sh = hand_shift(n) if shift == "hand" else far_shift(n) if shift == "far" else None
    return ensemble_pass(pass_stack(n, T, dtype), m, ov, sh, n_frames=1, signal_threshold=signal_threshold, **KWS[kw])


@functools.lru_cache(maxsize=None)
def far_shift(n):
    """Offsets far outside the frame in every direction: every one is clamped."""
    rows, cols = grid_shape(n)
    sh = np.empty((rows, cols, 2), dtype=np.int16)
    sh[..., 0] = np.where(np.arange(rows)[:, None] % 2 == 0, -300, 300)
    sh[..., 1] = np.where(np.arange(cols)[None, :] % 2 == 0, 32767, -32768)
    return sh


# masks: blanked frames (the count filter NaNs windows, the predictor skips them) and a signal threshold that scores the shifted B
COUNT_KW = dict(corr_min=0.1, s2n_min=1.5, count_min=0.2)
SIGNAL_THR = 0.2


@functools.lru_cache(maxsize=None)
def blanked_stack():
    """The river stack with the upper left quarter empty in EVERY frame: the coarse and fine windows there keep no pair (count 0 -> NaN),
    so the predictor has to do without their vectors."""
    a = river_stack().copy()
    a[:, :80, :100] = 0
    return a


@functools.lru_cache(maxsize=None)
def blanked_chain():
    return ensemble_multipass(blanked_stack(), CHAINS["64"], **COUNT_KW)


@functools.lru_cache(maxsize=None)
def signal_stack():
    """The 32 px pass stack with the columns 0 .. 41 of frame 3 empty: whether pair 2 keeps a window of the second grid column (x0 = 16) then
    depends on where its window of frame 3 is cut -- five windows score differently at their offsets than at zero offsets (0.2 of 1024
    samples is no whole number: no score sits on the threshold) -- and an upper right corner that is empty in every frame."""
    a = pass_stack(32).copy()
    a[3, :, :42] = 0
    a[:, :30, 100:] = 0
    return a


@functools.lru_cache(maxsize=None)
def signal_ref():
    m, ov, _ = PASS_CASES[32]
    return ensemble_pass(signal_stack(), m, ov, hand_shift(32), n_frames=1, signal_threshold=SIGNAL_THR, **KW)


# rescue: the recipe of tests/sliding_ref.py (``speckle_stack``) -- single-pixel speckles drifting one pixel per frame
RESCUE = (32, 16)


@functools.lru_cache(maxsize=None)
def speckle_stack():
    from tests import sliding_ref

    return sliding_ref.speckle_stack()


@functools.lru_cache(maxsize=None)
def speckle_shift():
    """The speckles drift +1 px in x per frame: every other column of windows gets the offset dx = 1 and is left with a residual of 0, the
    others keep the residual of 1 px -- either way the peak sits on exactly-zero neighbours, the worst case of the float32 fit."""
    a = speckle_stack()
    rows, cols = (len(q) for q in mp.grid_origins(a.shape[1:], *RESCUE))
    sh = np.zeros((rows, cols, 2), dtype=np.int16)
    sh[:, 1::2, 1] = 1
    return sh


@functools.lru_cache(maxsize=None)
def speckle_ref():
    return ensemble_pass(speckle_stack(), *RESCUE, speckle_shift(), n_frames=1, **KW)


# ---- the shifted ensemble over more than one pair-block (16 pairs): the inputs of tests/test_gpu_batch_loops.py -----------------------------
LONG_T = 36                               # 35 pairs: pair-blocks 16 + 16 + 3 in one accumulate call
LONG_CHUNKS = [(0, 18), (17, 36)]         # 17 + 18 pairs: two kept chunks of two pair-blocks each (16 + 1, 16 + 2)
LONG_DTYPES = (np.float32, np.float64)


@functools.lru_cache(maxsize=None)
def long_speckle_stack(dtype=np.uint8, stepped=False):
    """``stepped`` (tests/sliding_ref.py ``speckle_stack``): some pairs move 2 px, more of them after frame 20 -- the fit of a flagged
    window then depends on which pairs the float64 sums hold; on the steady stack it does not."""
    from tests import sliding_ref

    return as_samples(sliding_ref.speckle_stack(T=LONG_T, stepped=stepped), dtype)


@functools.lru_cache(maxsize=None)
def long_speckle_ref(dtype=np.uint8, stepped=False):
    return ensemble_pass(long_speckle_stack(dtype, stepped).astype(np.float64), *RESCUE, speckle_shift(), n_frames=1, **KW)
