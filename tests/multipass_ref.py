"""Float64 numpy reference of multi-pass PIV: the shifted pass, the predictor between two passes and the
chain.  Composed of the oracle's own pieces (sliding_window_stack, ncc, signal_mask, u_v_displacement), which it leaves as they are.
Like the rest of the PIV path it is this project's reading: unpinned against a real ffpiv.

All pass-to-pass arithmetic is in the kernels' orientation (u column shift, v row shift, rows downward); SEMANTICS["v_sign"] is applied
once, to the result of a shifted pass or of a chain."""
import functools
import warnings

import numpy as np

from oracle import piv_oracle as po

SHIFT_WINDOWS = (16, 32, 64)


def overlap_pair(overlap):
    """``overlap`` as (oy, ox): an int stands for both axes."""
    if isinstance(overlap, (int, np.integer)):
        return int(overlap), int(overlap)
    oy, ox = overlap
    return int(oy), int(ox)


def grid_origins(dim_size, n, overlap):
    """(y0 (rows,), x0 (cols,)) of the n x n windows at the given overlap, an int or a pair (oy, ox)."""
    y0, x0 = po.window_origins(dim_size, (n, n), overlap_pair(overlap))
    return np.asarray(y0, dtype=np.int64), np.asarray(x0, dtype=np.int64)


def clamp_shift(shift, dim_size, n, overlap):
    """The frame clamp of every shifted pass: dy in [-y0, H - n - y0], dx in [-x0, W - n - x0].  shift (..., rows, cols, 2) {dy, dx}."""
    y0, x0 = grid_origins(dim_size, n, overlap)
    s = np.asarray(shift, dtype=np.int64)
    out = np.empty_like(s)
    out[..., 0] = np.clip(s[..., 0], -y0[:, None], dim_size[0] - n - y0[:, None])
    out[..., 1] = np.clip(s[..., 1], -x0[None, :], dim_size[1] - n - x0[None, :])
    return out


def shifted_piv(imgs, n, overlap, shift=None, signal_threshold=None):
    """One shifted pass; ``overlap`` an int or a pair (oy, ox).  dict(u, v, corr, s2n (T-1, rows, cols), planes (T-1, n_win, n, n), tie,
    shift = the CLAMPED offsets, x, y).  A = window of frame t at (y0, x0), B = window of frame t+1 at (y0 + dy, x0 + dx); everything else is the plain path's.  ``tie``
    marks the windows whose arg-max is a matter of rounding in any implementation (an exact float64 tie for the plane maximum)."""
    imgs = np.asarray(imgs)
    T, H, W = imgs.shape
    if po.SEMANTICS["signal_mode"] == 1 or not po.SEMANTICS["norm_clip"]:
        raise NotImplementedError("multi-pass PIV: signal_mode = 1 and norm_clip = 0 are not supported")
    x, y = po.get_rect_coordinates((H, W), (n, n), overlap_pair(overlap))
    y0, x0 = grid_origins((H, W), n, overlap)
    rows, cols = len(y0), len(x0)
    if shift is None:
        shift = np.zeros((T - 1, rows, cols, 2), dtype=np.int64)
    sh = clamp_shift(np.asarray(shift).reshape(T - 1, rows, cols, 2), (H, W), n, overlap)
    stack = po.sliding_window_stack(imgs, (n, n), overlap_pair(overlap))                   # (T, n_win, n, n)
    planes = np.full((T - 1, rows * cols, n, n), np.nan)
    ar = np.arange(n)
    for t in range(T - 1):
        by = (y0[:, None] + sh[t, :, :, 0]).reshape(-1)                                    # (n_win,)
        bx = (x0[None, :] + sh[t, :, :, 1]).reshape(-1)
        B = imgs[t + 1][(by[:, None] + ar[None, :])[:, :, None], (bx[:, None] + ar[None, :])[:, None, :]]
        A = stack[t]
        keep = po.signal_mask(A, B, signal_threshold)
        if keep.any():
            planes[t, keep] = po.ncc(A[keep], B[keep])
    with po.semantics(v_sign=0):
        u, v = po.u_v_displacement(planes, rows, cols)
    u = u + sh[..., 1]
    v = v + sh[..., 0]
    if po.SEMANTICS["v_sign"]:
        v = -v
    shape = (T - 1, rows, cols)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN planes (windows below the signal threshold)
        cm = np.nanmax(planes, axis=(-2, -1))
        s2n = cm / np.nanmean(planes, axis=(-2, -1))
    top = np.sort(planes.reshape(planes.shape[:2] + (-1,)), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        tie = ((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (cm > 0)
    return dict(u=u, v=v, corr=cm.reshape(shape), s2n=s2n.reshape(shape), planes=planes, tie=tie.reshape(shape), shift=sh, x=x, y=y)


def _median2(q, valid):
    """M2 (rows, cols): twice the median of q over the valid entries of the 3 x 3 neighbourhood clipped at the edges, centre included."""
    rows, cols = q.shape
    out = np.zeros((rows, cols), dtype=np.int64)
    for r in range(rows):
        for c in range(cols):
            r0, r1, c0, c1 = max(r - 1, 0), min(r + 2, rows), max(c - 1, 0), min(c + 2, cols)
            vals = np.sort(q[r0:r1, c0:c1][valid[r0:r1, c0:c1]])
            k = len(vals)
            if k:
                out[r, c] = 2 * vals[k // 2] if k % 2 else vals[k // 2 - 1] + vals[k // 2]
    return out


def _axis(cf, n_c, s, count):
    """(i0, i1, w0, w1) per fine centre: the interval between coarse centres cc = i s + n_c / 2 and its integer weights."""
    cf = np.asarray(cf, dtype=np.int64)
    cc0 = n_c // 2
    i0 = np.clip(np.floor_divide(cf - cc0, s), 0, max(count - 2, 0))
    w1 = np.clip(cf - (i0 * s + cc0), 0, s) if count > 1 else np.zeros_like(cf)
    return i0, np.minimum(i0 + 1, count - 1), s - w1, w1


def predict_shift(u, v, dim_size, coarse, fine):
    """(u, v) (P, rows_c, cols_c) of a pass on its grid ``coarse`` = (n, overlap) -> int16 offsets (P, rows_f, cols_f, 2) {dy, dx} on the
    grid ``fine``, clamped to the frame.  Exact integer arithmetic after the rint."""
    (nc, oc), (nf, of) = coarse, fine
    H, W = dim_size
    if H > 32767 or W > 32767:
        raise ValueError("a frame side above 32767 does not fit the int16 offsets")
    u = np.asarray(u, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32)
    y0c, x0c = grid_origins(dim_size, nc, oc)
    y0f, x0f = grid_origins(dim_size, nf, of)
    u = u.reshape(-1, len(y0c), len(x0c))
    v = v.reshape(-1, len(y0c), len(x0c))
    sy = sx = nc - oc
    iy0, iy1, wy0, wy1 = _axis(y0f + nf // 2, nc, sy, len(y0c))
    ix0, ix1, wx0, wx1 = _axis(x0f + nf // 2, nc, sx, len(x0c))
    den = 2 * sy * sx
    out = np.empty((u.shape[0], len(y0f), len(x0f), 2), dtype=np.int64)
    for p in range(u.shape[0]):
        valid = np.isfinite(u[p]) & np.isfinite(v[p])
        with np.errstate(invalid="ignore"):
            # rint: half to even, in float32; clamped to the range of the int16 offsets (no displacement a frame can hold is touched)
            qu = np.clip(np.where(valid, np.rint(u[p]), 0), -32768, 32767).astype(np.int64)
            qv = np.clip(np.where(valid, np.rint(v[p]), 0), -32768, 32767).astype(np.int64)
        for comp, q in ((1, qu), (0, qv)):
            m2 = _median2(q, valid)
            num = ((wy0[:, None] * wx0[None, :]) * m2[iy0[:, None], ix0[None, :]] + (wy0[:, None] * wx1[None, :]) * m2[iy0[:, None], ix1[None, :]] +
                   (wy1[:, None] * wx0[None, :]) * m2[iy1[:, None], ix0[None, :]] + (wy1[:, None] * wx1[None, :]) * m2[iy1[:, None], ix1[None, :]])
            out[p, :, :, comp] = np.floor_divide(2 * num + den, 2 * den)
    return clamp_shift(out, dim_size, nf, of).astype(np.int16)


def multipass(imgs, passes, signal_threshold=None):
    """The chain.  ``passes``: [(n, overlap), ...] coarsest first.  A list of per-pass dicts (u, v, corr, s2n, planes, tie, shift) in the
    kernels' orientation, except that the LAST pass's v carries SEMANTICS["v_sign"].  Pass 0 is the plain oracle."""
    imgs = np.asarray(imgs)
    dim = imgs.shape[1:]
    out = []
    with po.semantics(v_sign=0):
        for k, (n, ov) in enumerate(passes):
            if k and n not in SHIFT_WINDOWS:
                raise ValueError(f"pass {k}: window {n} not in {SHIFT_WINDOWS}")
            shift = None if k == 0 else predict_shift(out[-1]["u"], out[-1]["v"], dim, passes[k - 1], (n, ov))
            out.append(shifted_piv(imgs, n, ov, shift, signal_threshold))
    if po.SEMANTICS["v_sign"]:
        out[-1] = dict(out[-1], v=-out[-1]["v"])
    return out


# ---- the float64 rescue pass on shifted windows: the inputs of tests/test_gpu_rescue_modes.py ------------------------------------------------
# single-pixel speckles on a 16 px lattice drifting 1 px per frame (tests/sliding_ref.py ``speckle_stack``): every correlation peak sits on
# exactly-zero neighbours, the worst case of the float32 fit, so windows are flagged
RESCUE_GEOMETRIES = [(16, 8), (32, 16), (64, 32), (64, 48)]
RESCUE_DIM = (136, 200)
RESCUE_T = 5


@functools.lru_cache(maxsize=None)
def rescue_stack(dtype=np.uint8):
    from tests import sliding_ref

    return sliding_ref.as_samples(sliding_ref.speckle_stack(T=RESCUE_T, H=RESCUE_DIM[0], W=RESCUE_DIM[1], seed=11), dtype)


@functools.lru_cache(maxsize=None)
def rescue_offsets(n, overlap):
    """Raw int16 offsets (P, rows, cols, 2) {dy, dx}: every other column of windows follows the drift (residual 0, the others keep 1 px),
    every other pair sits 2 px lower -- and, in the speckle part, offsets that point out of the frame: pair 0's top row up, pair 2's left
    column to the left (``clamp_shift`` brings both back to 0)."""
    rows, cols = (len(q) for q in grid_origins(RESCUE_DIM, n, overlap))
    sh = np.zeros((RESCUE_T - 1, rows, cols, 2), dtype=np.int16)
    sh[:, :, 1::2, 1] = 1
    sh[1::2, :, :, 0] = 2
    sh[0, 0, :, 0] = -3
    sh[2, :, 0, 1] = -2
    return sh


@functools.lru_cache(maxsize=None)
def rescue_ref(n, overlap, dtype=np.uint8):
    return shifted_piv(rescue_stack(dtype).astype(np.float64), n, overlap, rescue_offsets(n, overlap))
