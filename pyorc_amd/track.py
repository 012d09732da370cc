"""Pyramidal Lucas-Kanade point tracking: the displacement of small windows around given points from one frame to the next.

The third family of image-based river gauging next to PIV and STIV (KLT-IV, optical tracking velocimetry, every OpenCV-based LSPTV
script): a velocity at a *point* from a window of 5 .. 31 px, no peak locking, and -- through the pyramid -- displacements far beyond the
window without a multi-pass chain:

    r = track.track_pairs(frames, points, window=21, levels=3)     # Tracks: .u .v (T - 1, N) px/frame, .status, .err, .min_eig, .n_iter
    g = track.track_grid(frames, 32, 16)                           # the points are the centres of the PIV grid: fields (T - 1, rows, cols)
    tr = track.trajectories(frames, points0)                       # Lagrangian: .xy (T, N, 2), NaN once a point is lost
    lvl1 = track.pyr_down(frames)                                  # one pyramid step, (T, (H + 1) // 2, (W + 1) // 2) float32

One wave of the GPU runs one (point, pair) through all levels.  The semantics are this project's own -- unpinned against OpenCV;
tests/track_ref.py is their float32 / float64 numpy statement.  Every pair stands alone, so a long video runs in time slices with one
frame of halo, bit for bit what one call gives.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _lib, device
from .device import DeviceFrames, is_device

MIN_WINDOW, MAX_WINDOW, MAX_LEVELS, MAX_ITER = 5, 31, 5, 100
STATUS_OK, STATUS_MAX_ITER, STATUS_LOST, STATUS_OUT, STATUS_NOT_FINITE, STATUS_BAD_POINT = 0, 1, 2, 3, 4, 5


class Tracks(NamedTuple):
    """``u``, ``v`` (T - 1, N) float64: pixels per frame; ``status`` uint8: 0 converged, 1 level 0 ended on ``max_iter`` (still a vector),
    2 lost (no texture: the normal matrix is singular, or its smaller eigenvalue is below ``min_eig``), 3 walked out of the frame, 4 a
    NaN sample, 5 the point is not finite; 2 .. 5 have NaN in ``u``, ``v``, ``err``.  ``err``: the mean |I - J| over the window at the
    result; ``min_eig``: the smaller eigenvalue of the normal matrix at level 0 over w^2 (the Shi-Tomasi score); ``n_iter`` int32: the
    iterations of all levels."""
    u: np.ndarray
    v: np.ndarray
    status: np.ndarray
    err: np.ndarray
    min_eig: np.ndarray
    n_iter: np.ndarray


class GridTracks(NamedTuple):
    """``Tracks`` on the PIV grid, every field (T - 1, rows, cols); ``u32``, ``v32``: u, v as float32 (what ``validate.median_test`` takes);
    ``x``, ``y``: the grid's columns and rows in pixels."""
    u: np.ndarray
    v: np.ndarray
    status: np.ndarray
    err: np.ndarray
    min_eig: np.ndarray
    n_iter: np.ndarray
    u32: np.ndarray
    v32: np.ndarray
    x: np.ndarray
    y: np.ndarray


class Trajectories(NamedTuple):
    """``xy`` (T, N, 2) float64: row 0 the start, row t + 1 = row t + (u, v) of pair t; NaN once the point is lost.  The other fields
    are ``Tracks``' (a lost point has status 5 from the next pair on)."""
    xy: np.ndarray
    u: np.ndarray
    v: np.ndarray
    status: np.ndarray
    err: np.ndarray
    min_eig: np.ndarray
    n_iter: np.ndarray


def level_shapes(H: int, W: int, levels: int):
    """[(H, W), ((H + 1) // 2, (W + 1) // 2), ..]: the sizes of the pyramid's levels."""
    out = [(int(H), int(W))]
    for _ in range(1, levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _check_levels(H, W, levels):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)):
        raise TypeError(f"levels must be an integer, got {levels!r}")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels {levels!r} outside 1 .. {MAX_LEVELS}")
    for lvl, (h, w) in enumerate(level_shapes(H, W, levels)):
        need = 3 if lvl < levels - 1 else 2
        if min(h, w) < need:
            raise ValueError(f"level {lvl} of a {H} x {W} frame is {h} x {w}, below {need} x {need}: too small for {levels} levels")
    return int(levels)


def _check_params(window, max_iter, eps, min_eig):
    for name, val in (("window", window), ("max_iter", max_iter)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {val!r}")
    if not MIN_WINDOW <= window <= MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"window {window!r} is not odd in {MIN_WINDOW} .. {MAX_WINDOW}")
    if not 1 <= max_iter <= MAX_ITER:
        raise ValueError(f"max_iter {max_iter!r} outside 1 .. {MAX_ITER}")
    eps, min_eig = float(eps), float(min_eig)
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError(f"eps {eps!r} must be >= 0")
    if not (min_eig >= 0.0 and np.isfinite(min_eig)):
        raise ValueError(f"min_eig {min_eig!r} must be >= 0")
    return int(window), int(max_iter), eps, min_eig


def _check_points(points, pairs, H, W, what="points", inside=True):
    """(N, 2) or (pairs, N, 2) float64, C-contiguous; -> (array, per_pair).  Points: every one finite and inside [0, W - 1] x [0, H - 1]."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
    if p.ndim not in (2, 3) or p.shape[-1] != 2 or (p.ndim == 3 and p.shape[0] != pairs):
        raise ValueError(f"{what} must be (N, 2) or ({pairs}, N, 2), got shape {p.shape}")
    if inside:
        ok = (p[..., 0] >= 0.0) & (p[..., 0] <= W - 1) & (p[..., 1] >= 0.0) & (p[..., 1] <= H - 1)   # False for NaN
    else:
        ok = np.isfinite(p).all(axis=-1)
    if not ok.all():
        idx = tuple(int(q) for q in np.argwhere(~ok)[0])
        where = f"point {idx[-1]}" + (f" of pair {idx[0]}" if p.ndim == 3 else "")
        raise ValueError(f"{what}: {where} ({float(p[idx][0])!r}, {float(p[idx][1])!r}) is "
                         + (f"not inside the frame [0, {W - 1}] x [0, {H - 1}] (or is not finite)" if inside else "not finite"))
    return p, int(p.ndim == 3)


def pyr_down(frames):
    """One pyramid step: (T, H, W) uint8 or float32 -> (T, (H + 1) // 2, (W + 1) // 2) float32, a host array for a host array and a
    ``DeviceFrames`` for a ``DeviceFrames`` (the same bits).  Taps [1, 4, 6, 4, 1] / 16 along x, then along y, on every second sample,
    the source reflected without repeating the edge; both sides at least 3."""
    a = device.check_stack(frames, "track")
    T, H, W = (int(q) for q in a.shape)
    if min(H, W) < 3:
        raise ValueError(f"frames of {H} x {W} are smaller than 3 x 3")
    shape = (T, (H + 1) // 2, (W + 1) // 2)
    dev = is_device(a)
    out = DeviceFrames.empty(shape, np.float32) if dev else np.empty(shape, dtype=np.float32)
    if T == 0:
        return out
    lib = _lib.load()
    _lib.require_device()
    code = _lib.DTYPE_CODES[np.dtype(a.dtype)]
    if dev:
        _lib.check(lib.lspiv_pyr_down_dev(a.c_ptr, code, T, H, W, out.c_ptr, None))
    else:
        _lib.check(lib.lspiv_pyr_down(_lib.ptr(a), code, T, H, W, _lib.ptr(out)))
    return out


def _run(a, pts, per_pair, guess, guess_per_pair, window, levels, max_iter, eps, min_eig, chain):
    """One C call on a checked stack; -> (u, v, status, err, min_eig, n_iter, xy or None)."""
    T, H, W = (int(q) for q in a.shape)
    P, N = T - 1, int(pts.shape[-2])
    u, v, err, lam = (np.empty((P, N)) for _ in range(4))
    n_iter, status = np.empty((P, N), dtype=np.int32), np.empty((P, N), dtype=np.uint8)
    xy = np.empty((T, N, 2)) if chain else None
    if N == 0:
        return u, v, status, err, lam, n_iter, xy
    lib = _lib.load()
    _lib.require_device()
    code = _lib.DTYPE_CODES[np.dtype(a.dtype)]
    args = (window, levels, max_iter, eps, min_eig, int(chain))
    if is_device(a):
        d_p = device.buffer(pts)
        d_g = None if guess is None else device.buffer(guess)
        d = [device.buffer(nbytes=q.nbytes) for q in (u, v, err, lam, n_iter, status)]
        d_xy = device.buffer(nbytes=xy.nbytes) if chain else None
        _lib.check(lib.lspiv_lk_track_dev(a.c_ptr, code, T, H, W, d_p.c_ptr, N, per_pair, None if d_g is None else d_g.c_ptr, guess_per_pair, *args,
                                          *(q.c_ptr for q in d), None if d_xy is None else d_xy.c_ptr, None))
        u, v, err, lam, n_iter, status = (device.download(q, h.shape, h.dtype) for q, h in zip(d, (u, v, err, lam, n_iter, status)))
        if chain:
            xy = device.download(d_xy, xy.shape, np.float64)
    else:
        _lib.check(lib.lspiv_lk_track(_lib.ptr(a), code, T, H, W, _lib.ptr(pts), N, per_pair, None if guess is None else _lib.ptr(guess),
                                      guess_per_pair, *args, _lib.ptr(u), _lib.ptr(v), _lib.ptr(err), _lib.ptr(lam), _lib.ptr(n_iter), _lib.ptr(status),
                                      None if xy is None else _lib.ptr(xy)))
    return u, v, status, err, lam, n_iter, xy


def _prepare(frames, points, window, levels, max_iter, eps, min_eig, guess, chain=False):
    a = device.check_stack(frames, "track", t_min=2)
    T, H, W = (int(q) for q in a.shape)
    window, max_iter, eps, min_eig = _check_params(window, max_iter, eps, min_eig)
    levels = _check_levels(H, W, levels)
    pts, per_pair = _check_points(points, T - 1, H, W)
    if chain and per_pair:
        raise ValueError(f"points0 must be (N, 2), got shape {pts.shape}")
    g, g_per_pair = None, 0
    if guess is not None:
        g, g_per_pair = _check_points(guess, T - 1, H, W, what="guess", inside=False)
        if g.shape[-2] != pts.shape[-2]:
            raise ValueError(f"guess has {g.shape[-2]} vectors for {pts.shape[-2]} points")
    return a, pts, per_pair, g, g_per_pair, window, levels, max_iter, eps, min_eig


def track_pairs(frames, points, window: int = 21, levels: int = 3, max_iter: int = 20, eps: float = 0.01, min_eig: float = 0.0,
                guess=None) -> Tracks:
    """The displacement of the ``window`` x ``window`` px around every point from frame t to frame t + 1, for every pair of ``frames``.

    ``frames``: (T >= 2, H, W) uint8 or float32, a host array or a ``DeviceFrames`` (the same bits).  ``points``: (N, 2) float64 (x, y)
    in pixels, the same for every pair, or (T - 1, N, 2); every point inside [0, W - 1] x [0, H - 1].  ``window``: odd, 5 .. 31;
    ``levels``: 1 .. 5 pyramid levels, each half the size of the one below -- the reach is about ``window`` * 2^(levels - 1) / 2 px;
    ``max_iter`` (1 .. 100) and ``eps`` (px, at the level's scale) end the iterations of a level; a point whose smaller eigenvalue
    (``Tracks.min_eig``) is below ``min_eig`` is not tracked; ``guess``: an initial (u, v) per point, shaped like ``points`` -- a PIV
    field handed over for refinement."""
    a, pts, per_pair, g, g_per_pair, window, levels, max_iter, eps, min_eig = _prepare(frames, points, window, levels, max_iter, eps, min_eig, guess)
    return Tracks(*_run(a, pts, per_pair, g, g_per_pair, window, levels, max_iter, eps, min_eig, False)[:6])


def track_grid(frames, window_size: int, overlap: Optional[int] = None, **kw) -> GridTracks:
    """``track_pairs`` at the centres of the PIV grid of ``window_size`` px windows at ``overlap`` (default: half a window); every field
    comes back as (T - 1, rows, cols).  ``kw``: ``window`` (the tracker's own, default 21), ``levels``, ``max_iter``, ``eps``,
    ``min_eig``, ``guess`` ((T - 1, rows, cols, 2) or (rows, cols, 2))."""
    from . import window as _window

    a = device.check_stack(frames, "track", t_min=2)
    H, W = int(a.shape[1]), int(a.shape[2])
    ov = int(window_size) // 2 if overlap is None else int(overlap)
    x, y = _window.get_rect_coordinates((H, W), (int(window_size),) * 2, (ov, ov))
    rows, cols = len(y), len(x)
    xx, yy = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    pts = np.stack([xx.ravel(), yy.ravel()], axis=1)
    if kw.get("guess") is not None:
        g = np.asarray(kw["guess"], dtype=np.float64)
        if g.shape[-3:] != (rows, cols, 2):
            raise ValueError(f"guess must be (..., {rows}, {cols}, 2), got shape {g.shape}")
        kw["guess"] = g.reshape(g.shape[:-3] + (rows * cols, 2))
    r = track_pairs(a, pts, **kw)
    f = [q.reshape(q.shape[0], rows, cols) for q in r]
    return GridTracks(*f, f[0].astype(np.float32), f[1].astype(np.float32), np.asarray(x), np.asarray(y))


def trajectories(frames, points0, window: int = 21, levels: int = 3, max_iter: int = 20, eps: float = 0.01, min_eig: float = 0.0) -> Trajectories:
    """Lagrangian tracks: every point of ``points0`` (N, 2) is followed through all T frames, pair t starting where pair t - 1 ended.
    The pairs run one after another on the GPU inside one call; the positions never come through the host in between.  A point that is
    lost (status 2, 3, 4) is NaN from the next row of ``xy`` on."""
    a, pts, _, _, _, window, levels, max_iter, eps, min_eig = _prepare(frames, points0, window, levels, max_iter, eps, min_eig, None, chain=True)
    u, v, status, err, lam, n_iter, xy = _run(a, pts, 0, None, 0, window, levels, max_iter, eps, min_eig, True)
    if xy.shape[1] == 0:
        xy = np.empty((a.shape[0], 0, 2))
    return Trajectories(xy, u, v, status, err, lam, n_iter)
