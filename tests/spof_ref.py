"""Float64 numpy reference of the SPOF phase-filtered correlation: one plane, the per-pair result and the
ensemble, composed of the oracle's own pieces (``normalize_intensity``, ``signal_mask``, ``sliding_window_stack``, ``u_v_displacement``)
and the ensemble steps of ``oracle.piv_oracle.get_ffpiv`` as ``tests/ensemble_multipass_ref.py`` restates them; all left as they are.
Like the rest of the PIV path it is this project's reading: unpinned against a real ffpiv.  Kernel orientation throughout (u column
shift, v row shift, rows downward); SEMANTICS["v_sign"] is applied once, to the result.

Also the inputs tests/test_spof_host.py and tests/test_gpu_spof.py share, computed once per process."""
import functools
import warnings

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd import synth
from tests import deform_ref, multipass_ref

SPOF_WINDOWS = (16, 32, 64)


def plane(win_a, win_b):
    """The filtered plane(s) of window pairs (..., N, N): a^ = normalize_intensity(A), b^ likewise; Rn = conj(fft2 a^) fft2 b^ / N^2;
    R' = Rn / sqrt(|Rn|), 0 where Rn = 0; clip(fftshift(ifft2(R').real), 0, 1)."""
    n = win_a.shape[-1]
    a = po.normalize_intensity(win_a)
    b = po.normalize_intensity(win_b)
    rn = np.conj(np.fft.fft2(a)) * np.fft.fft2(b) / float(n * n)
    mag = np.abs(rn)
    rp = np.divide(rn, np.sqrt(mag), out=np.zeros_like(rn), where=(mag != 0))
    c = np.fft.fftshift(np.fft.ifft2(rp).real, axes=(-2, -1))
    return np.clip(c, 0.0, 1.0)


def ncc_plane(win_a, win_b):
    """The unfiltered plane of the same pairs (the oracle's ncc): what the filtered one is compared with."""
    return po.ncc(win_a, win_b)


def _planes(imgs, n, overlap, signal_threshold, fn):
    imgs = np.asarray(imgs)
    if n not in SPOF_WINDOWS:
        raise ValueError(f"window {n} not in {SPOF_WINDOWS}")
    if po.SEMANTICS["signal_mode"] == 1 or not po.SEMANTICS["norm_clip"]:
        raise NotImplementedError("filtered correlation: signal_mode = 1 and norm_clip = 0 are not supported")
    T = imgs.shape[0]
    stack = po.sliding_window_stack(imgs.astype(np.float64), (n, n), multipass_ref.overlap_pair(overlap))       # (T, n_win, n, n)
    out = np.full((T - 1,) + stack.shape[1:], np.nan)
    with np.errstate(all="ignore"):
        for t in range(T - 1):
            A, B = stack[t], stack[t + 1]
            keep = po.signal_mask(A, B, signal_threshold) & np.isfinite(A).all(axis=(-2, -1)) & np.isfinite(B).all(axis=(-2, -1))
            if keep.any():
                out[t, keep] = fn(A[keep], B[keep])
    return out


def _grid(dim_size, n, overlap):
    oy, ox = multipass_ref.overlap_pair(overlap)
    return po.get_axis_shape(dim_size[0], n, oy), po.get_axis_shape(dim_size[1], n, ox)


def fragile_mask(planes):
    """Per plane: a second sample within 1e-4 (relative) of the maximum, or a neighbour of an interior peak below 1e-5 -- windows whose
    float32 arg-max or log-Gaussian fit cannot be held to the float64 one's.  From the reference alone."""
    P, n_win, wy, wx = planes.shape
    flat = planes.reshape(P * n_win, wy * wx)
    out = np.zeros(P * n_win, dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in range(P * n_win):
            pl = flat[k]
            if not np.isfinite(pl).all() or pl.max() <= 0:
                continue
            top = np.sort(pl)[-2:]
            if top[1] - top[0] <= 1e-4 * top[1]:
                out[k] = True
                continue
            i, j = divmod(int(np.argmax(pl)), wx)
            if 0 < i < wy - 1 and 0 < j < wx - 1:
                p2 = pl.reshape(wy, wx)
                if min(p2[i - 1, j], p2[i + 1, j], p2[i, j - 1], p2[i, j + 1]) < 1e-5:
                    out[k] = True
    return out.reshape(P, n_win)


def piv(imgs, n, overlap, signal_threshold=None, fn=plane):
    """The per-pair result (``overlap`` an int or a pair (oy, ox)): dict(u, v, corr, s2n (T-1, rows, cols), planes (T-1, n_win, n, n), fragile (T-1, rows, cols)).  corr = max of
    the plane, s2n = max / mean of the clipped plane; a pair failing the signal threshold, or with a non-finite sample, is NaN throughout.
    ``fn``: :func:`plane` (the filter) or :func:`ncc_plane` (the unfiltered path, for comparisons)."""
    imgs = np.asarray(imgs)
    rows, cols = _grid(imgs.shape[1:], n, overlap)
    planes = _planes(imgs, n, overlap, signal_threshold, fn)
    u, v = po.u_v_displacement(planes, rows, cols)
    shape = (imgs.shape[0] - 1, rows, cols)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        cm = planes.max(axis=(-2, -1))
        s2n = cm / planes.mean(axis=(-2, -1))
    return dict(u=u, v=v, corr=cm.reshape(shape), s2n=s2n.reshape(shape), planes=planes, fragile=fragile_mask(planes).reshape(shape))


def ensemble(imgs, n, overlap, corr_min=0.2, s2n_min=3.0, count_min=0.2, n_frames=1, signal_threshold=None, fn=plane):
    """The ensemble over all pairs of ``imgs`` on the filtered planes (the steps of tests/ensemble_multipass_ref.ensemble_pass): dict(u, v,
    corr, s2n (1, rows, cols), count (n_win,), planes (1, n_win, n, n) = the mean planes, fragile (1, rows, cols), pair_corr, pair_s2n
    (P, n_win) = the per-pair values BEFORE the masks)."""
    imgs = np.asarray(imgs)
    P = imgs.shape[0] - 1
    rows, cols = _grid(imgs.shape[1:], n, overlap)
    corr = _planes(imgs, n, overlap, signal_threshold, fn)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        pair_cm = corr.max(axis=(-2, -1))
        pair_sn = pair_cm / corr.mean(axis=(-2, -1))
        cm, sn = pair_cm.copy(), pair_sn.copy()
        masks = (cm >= corr_min) & (sn >= s2n_min) & np.isfinite(cm)
        corr[~masks] = 0.0
        cm[~masks] = 0.0
        sn[~masks] = 0.0
        corr_sum = corr.sum(axis=0, keepdims=True)
        corr_count = (cm > 1e-6).sum(axis=0, keepdims=True)                         # (1, n_win)
        low = corr_count < count_min * n_frames
        corr_sum[low] = np.nan
        cm[:, low.flatten()] = np.nan
        mean = corr_sum / corr_count[..., None, None]
        corr_mean = np.nanmean(cm, axis=0).reshape(1, rows, cols)
        s2n_mean = np.nanmean(sn, axis=0).reshape(1, rows, cols)
    u, v = po.u_v_displacement(mean, rows, cols)
    return dict(u=u, v=v, corr=corr_mean, s2n=s2n_mean, count=corr_count.reshape(-1).astype(np.float64), planes=mean,
                fragile=fragile_mask(mean).reshape(1, rows, cols), pair_corr=pair_cm, pair_s2n=pair_sn)


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------------
def textured_stack(T, H, W, seed, density, shift, amp, gain=0.6, tex_seed=1, cutoff=0.06):
    """Tracers over a static smooth texture: the particle stack at ``gain`` on a background of ``amp`` (1 + 0.5 tex), tex a unit-variance
    Gaussian-filtered noise field (cut-off ``cutoff`` cycles per pixel), the same in every frame; uint8."""
    base = synth.particle_stack(T, H, W, seed=seed, density=density, uniform_shift=shift).astype(np.float64)
    k = np.hypot(np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :])
    tex = np.fft.ifft2(np.fft.fft2(np.random.default_rng(tex_seed).normal(size=(H, W))) * np.exp(-(k / cutoff) ** 2)).real
    tex /= tex.std()
    return np.clip(np.rint(gain * base + amp * (1 + 0.5 * tex)), 0, 255).astype(np.uint8)


TRUTH = (3.3, -2.4)                 # (dx, dy) of the textured stacks
TEX_DIM = (160, 200)
TEX_AMP = 80
# name -> (frames, density, seed); both are read at 32 @ 16
TEXTURED = {"pairs": (4, 0.02, 5), "ensemble": (7, 0.012, 5)}
TEX_WINDOW = (32, 16)
# the ensemble masks on the textured input: filtered peaks are lower than NCC peaks (0.19 - 0.27 median against 0.42 - 0.59), so the
# default corr_min = 0.2 would drop most filtered planes; the masks are lowered so that neither weighting loses planes to them and the
# comparison is of the weightings alone (with the defaults: NCC 0.303, SPOF 0.455)
TEX_KW = dict(corr_min=0.1, s2n_min=1.5, count_min=0.2)
# the parity inputs' masks: corr_min sits inside the spread of the filtered peaks of each size (medians 0.27 / 0.31 / 0.34), so that some
# planes of some windows are dropped and the sums are no plain sums (tests/test_spof_host.py checks that, and that no pair sits on a mask)
ENS_CORR_MIN = {16: 0.2263, 32: 0.2925, 64: 0.33736}     # each in a gap of the float64 peaks: 1.3e-3 relative or more to either side


def ens_kw(case):
    return dict(corr_min=ENS_CORR_MIN[case], s2n_min=1.5, count_min=0.2)


PASS_CASES = deform_ref.PASS_CASES
GRID_CASES = deform_ref.GRID_CASES
PASS_DTYPES = deform_ref.PASS_DTYPES
SIGNAL_THR = deform_ref.SIGNAL_THR
ENS_T = 7


@functools.lru_cache(maxsize=None)
def textured(name):
    T, density, seed = TEXTURED[name]
    return textured_stack(T, TEX_DIM[0], TEX_DIM[1], seed, density, TRUTH, TEX_AMP)


def within_half_px(u, v):
    """Share of ALL windows whose vector lies within 0.5 px (Euclidean distance) of the truth; NaN windows count as misses."""
    with np.errstate(invalid="ignore"):
        return float((np.hypot(np.asarray(u, np.float64) - TRUTH[0], np.asarray(v, np.float64) - TRUTH[1]) <= 0.5).mean())


@functools.lru_cache(maxsize=None)
def textured_ref(name, filtered=True):
    n, ov = TEX_WINDOW
    fn = plane if filtered else ncc_plane
    if name == "pairs":
        return piv(textured(name), n, ov, fn=fn)
    return ensemble(textured(name), n, ov, n_frames=1, fn=fn, **TEX_KW)


def case_geometry(case):
    return PASS_CASES[case] if case in PASS_CASES else GRID_CASES[case]


@functools.lru_cache(maxsize=None)
def pass_ref(case, dtype=np.uint8, signal_threshold=None):
    n, ov, _ = case_geometry(case)
    return piv(deform_ref.pass_stack(case, dtype), n, ov, signal_threshold)


@functools.lru_cache(maxsize=None)
def signal_ref(case):
    n, ov, _ = PASS_CASES[case]
    return piv(deform_ref.signal_stack(case), n, ov, SIGNAL_THR)


@functools.lru_cache(maxsize=None)
def ens_stack(case, dtype=np.uint8):
    """The ensemble parity input: seven frames of the multi-pass ensemble's pass stack (six pairs)."""
    from tests import ensemble_multipass_ref as emp

    return emp.pass_stack(case, ENS_T, dtype)


@functools.lru_cache(maxsize=None)
def ens_ref(case, dtype=np.uint8):
    n, ov, _ = PASS_CASES[case]
    return ensemble(ens_stack(case, dtype), n, ov, n_frames=1, **ens_kw(case))


@functools.lru_cache(maxsize=None)
def ens_signal_stack():
    """The 32 px ensemble input with the samples below 40 set to zero and the upper left quarter of every frame empty (the recipe of
    deform_ref.signal_stack): a threshold of 0.3 takes out some pairs of some windows, and every pair of the windows in the empty quarter."""
    a = ens_stack(32).copy()
    a[a < 40] = 0
    a[:, :a.shape[1] // 2, :a.shape[2] // 2] = 0
    return a


@functools.lru_cache(maxsize=None)
def ens_signal_ref():
    n, ov, _ = PASS_CASES[32]
    return ensemble(ens_signal_stack(), n, ov, n_frames=1, signal_threshold=SIGNAL_THR, **ens_kw(32))
