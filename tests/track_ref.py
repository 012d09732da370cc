"""The semantics of pyramidal Lucas-Kanade point tracking (pyorc_amd.track) in float32 / float64 numpy,
vectorised over the points of a pair.  Unpinned against OpenCV or any other tracker: this file IS the statement.

    pyramid    float32, every operation one correctly rounded float32 operation (numpy fuses nothing): the GPU gives the same bits
    sampling   float32 bilinear blend on the edge-replicated level, the fractions from float64 positions
    template   I, Ix, Iy in float32; the normal matrix G in float64 from exact float32 x float32 products
    iterations forward additive (Bouguet): b in float64, the 2 x 2 solve in float64, every operation rounded on its own
    outputs    u, v, err, min_eig float64, n_iter int32, status uint8

Only the ORDER of the float64 sums is free (``order``): "numpy" is numpy's own pairwise sum, "lanes" is the kernel's (sample k on lane
k mod 64, a lane adds its samples with k ascending, then the halving tree 32, 16, .. 1 over the lanes).  track_pairs also returns the
smallest margin of every data-dependent decision, so that a test can tell a decision that rounding could flip from one it cannot.
"""
import numpy as np

STATUS_OK, STATUS_MAX_ITER, STATUS_LOST, STATUS_OUT, STATUS_NOT_FINITE, STATUS_BAD_POINT = 0, 1, 2, 3, 4, 5
MIN_WINDOW, MAX_WINDOW, MAX_LEVELS, MAX_ITER = 5, 31, 5, 100
DET_BOUND = 1e-9      # the point is lost unless det > DET_BOUND * Gxx * Gyy
F32 = np.float32


# ---- 1. pyramid -----------------------------------------------------------------------------------------------------------------------
def _reflect(idx, n):
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def _pass(a, axis):
    n = a.shape[axis]
    idx = _reflect(2 * np.arange((n + 1) // 2)[:, None] + np.arange(5)[None, :] - 2, n)
    t = [np.take(a, idx[:, j], axis=axis) for j in range(5)]
    return ((t[0] + t[4]) + F32(4.0) * (t[1] + t[3])) + F32(6.0) * t[2]


def pyr_down(frames):
    """(..., H, W) uint8 or float32 -> (..., (H + 1) // 2, (W + 1) // 2) float32: taps [1, 4, 6, 4, 1] along x, then along y, source index
    2 x + j - 2 reflected without repeating the edge, each pass ((a0 + a4) + 4 (a1 + a3)) + 6 a2, the result times 2^-8."""
    a = np.asarray(frames)
    assert a.dtype in (np.uint8, np.float32) and a.shape[-1] >= 3 and a.shape[-2] >= 3
    with np.errstate(invalid="ignore", over="ignore"):
        out = _pass(_pass(a.astype(F32), -1), -2) * F32(2.0 ** -8)
    assert out.dtype == F32
    return out


def level_shapes(H, W, levels):
    shapes = [(H, W)]
    for _ in range(1, levels):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    return shapes


def failing_level(H, W, levels):
    """None, or the first level whose size breaks the rules: a source of pyr_down needs both sides >= 3, every level both >= 2."""
    for lvl, (h, w) in enumerate(level_shapes(H, W, levels)):
        if min(h, w) < 2 or (lvl < levels - 1 and min(h, w) < 3):
            return lvl
    return None


def pyramid(frames, levels):
    pyr = [np.asarray(frames)]
    for _ in range(1, levels):
        pyr.append(pyr_down(pyr[-1]))
    return pyr


# ---- 2. sampling ----------------------------------------------------------------------------------------------------------------------
def sample(img, qx, qy, oi, oj):
    """(n, len(oi), len(oj)) float32: the bilinear samples of img (H, W) at (qx + oj, qy + oi) for n positions, edge replicated."""
    H, W = img.shape
    with np.errstate(invalid="ignore", over="ignore"):
        flx, fly = np.floor(qx), np.floor(qy)
        fx, fy = (qx - flx).astype(F32)[:, None, None], (qy - fly).astype(F32)[:, None, None]
        ix = np.clip(np.nan_to_num(flx, nan=-2.0 ** 30), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
        iy = np.clip(np.nan_to_num(fly, nan=-2.0 ** 30), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
        c0 = np.clip(ix[:, None] + oj[None, :], 0, W - 1)[:, None, :]
        c1 = np.clip(ix[:, None] + oj[None, :] + 1, 0, W - 1)[:, None, :]
        r0 = np.clip(iy[:, None] + oi[None, :], 0, H - 1)[:, :, None]
        r1 = np.clip(iy[:, None] + oi[None, :] + 1, 0, H - 1)[:, :, None]
        a, b, c, d = (img[r, cc].astype(F32) for r, cc in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
        top = a + fx * (b - a)
        bot = c + fx * (d - c)
        val = top + fy * (bot - top)
    assert val.dtype == F32
    return val


# ---- the float64 sums -----------------------------------------------------------------------------------------------------------------
def total(terms, order):
    """terms (n, w, w) float64 -> (n,): the sum of each window in the given order."""
    t = terms.reshape(len(terms), terms.shape[1] * terms.shape[2])
    with np.errstate(invalid="ignore", over="ignore"):
        if order == "numpy":
            return t.sum(axis=1)
        assert order == "lanes"
        k = t.shape[1]
        ns = (k + 63) // 64
        p = np.zeros((len(t), ns * 64))
        p[:, :k] = t
        p = p.reshape(len(t), ns, 64)
        acc = np.zeros((len(t), 64))
        for s in range(ns):
            acc = acc + p[:, s]
        h = 32
        while h:
            acc = acc[:, :h] + acc[:, h:2 * h]
            h //= 2
        return acc[:, 0]


class Margins:
    """The smallest relative distance of each kind of decision from its threshold over a run (inf: never taken)."""

    def __init__(self):
        self.eps = self.det = self.min_eig = self.border = np.inf

    def smallest(self):
        return min(self.eps, self.det, self.min_eig, self.border)

    def __repr__(self):
        return f"Margins(eps={self.eps:.3g}, det={self.det:.3g}, min_eig={self.min_eig:.3g}, border={self.border:.3g})"


def _low(x):
    return float(np.min(x)) if np.size(x) else np.inf


# ---- 3 - 5. one pair ------------------------------------------------------------------------------------------------------------------
def track_pair(pyr_i, pyr_j, points, window=21, max_iter=20, eps=0.01, min_eig=0.0, guess=None, order="numpy", margins=None):
    """One pair: pyr_i, pyr_j the pyramids (lists of (H_l, W_l) arrays, level 0 first) of frames t and t + 1, points (N, 2) float64.
    Returns u, v, err, lam (N,) float64, n_iter (N,) int32, status (N,) uint8, and the scales of level 0's template: sum |I| / w^2 and
    (Gxx + Gyy) / w^2 (N,)."""
    m = margins if margins is not None else Margins()
    L, w = len(pyr_i), int(window)
    r, ww = (w - 1) // 2, float(w * w)
    p = np.asarray(points, dtype=np.float64)
    N = len(p)
    off, offp = np.arange(-r, r + 1), np.arange(-r - 1, r + 2)
    eps2 = float(eps) * float(eps)
    status = np.zeros(N, dtype=np.uint8)
    n_iter = np.zeros(N, dtype=np.int32)
    lam0 = np.full(N, np.nan)
    err = np.full(N, np.nan)
    scale_err, scale_eig = np.full(N, np.nan), np.full(N, np.nan)      # what a gate on err and on min_eig is relative to
    d = np.zeros((N, 2)) if guess is None else np.ldexp(np.asarray(guess, dtype=np.float64), -(L - 1))
    bad = ~np.isfinite(p).all(axis=1)
    status[bad] = STATUS_BAD_POINT
    alive = ~bad
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for lvl in range(L - 1, -1, -1):
            imi, imj = pyr_i[lvl], pyr_j[lvl]
            Hl, Wl = imi.shape
            a = np.flatnonzero(alive)
            pl = np.ldexp(p[a], -lvl)
            # template
            patch = sample(imi, pl[:, 0], pl[:, 1], offp, offp)
            I = patch[:, 1:-1, 1:-1]
            Ix = F32(0.5) * (patch[:, 1:-1, 2:] - patch[:, 1:-1, :-2])
            Iy = F32(0.5) * (patch[:, 2:, 1:-1] - patch[:, :-2, 1:-1])
            Ix64, Iy64 = Ix.astype(np.float64), Iy.astype(np.float64)
            Gxx, Gyy, Gxy = total(Ix64 * Ix64, order), total(Iy64 * Iy64, order), total(Ix64 * Iy64, order)
            finite = np.isfinite(Gxx) & np.isfinite(Gyy) & np.isfinite(Gxy)
            det = Gxx * Gyy - Gxy * Gxy
            bound = DET_BOUND * Gxx * Gyy
            dif = Gxx - Gyy
            lam = ((Gxx + Gyy) - np.sqrt(dif * dif + 4.0 * (Gxy * Gxy))) / (2.0 * ww)
            if lvl == 0:
                lam0[a] = np.where(finite, lam, np.nan)
                scale_err[a] = total(np.abs(I).astype(np.float64), order) / ww
                scale_eig[a] = (Gxx + Gyy) / ww
            det_ok = det > bound
            lost = finite & (~det_ok | (lam < min_eig))
            # margins: a window without any gradient along x (or y) has Gxx = Gxy = 0 (or Gyy = Gxy = 0) from sums of exact zeros, whatever
            # their order, so det = bound = 0 exactly: there is no margin to take, and rounding cannot flip that decision
            flat = (Gxx == 0.0) | (Gyy == 0.0)
            m_det = np.abs(det - bound) / np.abs(bound)
            m_lam = np.abs(lam - min_eig) / np.maximum(min_eig, (Gxx + Gyy) / (2.0 * ww))
            judged = finite & ~flat
            # lost on the determinant: that margin decides, whatever the eigenvalue says; kept: both tests had to pass
            m.det = min(m.det, _low(m_det[judged]))
            m.min_eig = min(m.min_eig, _low(m_lam[judged & det_ok]))
            status[a[~finite]] = STATUS_NOT_FINITE
            status[a[lost]] = STATUS_LOST
            alive[a[~finite | lost]] = False
            keep = finite & ~lost
            a, pl, I, Ix64, Iy64, Gxx, Gyy, Gxy, det = (x[keep] for x in (a, pl, I, Ix64, Iy64, Gxx, Gyy, Gxy, det))
            # iterations
            run = np.ones(len(a), dtype=bool)          # still iterating at this level
            converged = np.zeros(len(a), dtype=bool)
            for _ in range(int(max_iter)):
                k = np.flatnonzero(run)
                if not len(k):
                    break
                g = a[k]
                J = sample(imj, pl[k, 0] + d[g, 0], pl[k, 1] + d[g, 1], off, off)
                e = (I[k] - J).astype(np.float64)
                bx, by = total(e * Ix64[k], order), total(e * Iy64[k], order)
                fin = np.isfinite(bx) & np.isfinite(by)
                ddx = (Gyy[k] * bx - Gxy[k] * by) / det[k]
                ddy = (Gxx[k] * by - Gxy[k] * bx) / det[k]
                status[g[~fin]] = STATUS_NOT_FINITE
                alive[g[~fin]] = False
                run[k[~fin]] = False
                k, g, ddx, ddy = k[fin], g[fin], ddx[fin], ddy[fin]
                d[g, 0] += ddx
                d[g, 1] += ddy
                n_iter[g] += 1
                qx, qy = pl[k, 0] + d[g, 0], pl[k, 1] + d[g, 1]
                inside = (qx >= 0.0) & (qx <= Wl - 1.0) & (qy >= 0.0) & (qy <= Hl - 1.0)
                dist = np.minimum(np.minimum(np.abs(qx), np.abs(Wl - 1.0 - qx)) / max(Wl - 1.0, 1.0),
                                  np.minimum(np.abs(qy), np.abs(Hl - 1.0 - qy)) / max(Hl - 1.0, 1.0))
                m.border = min(m.border, _low(dist[np.isfinite(dist)]))
                status[g[~inside]] = STATUS_OUT
                alive[g[~inside]] = False
                run[k[~inside]] = False
                k, g, ddx, ddy = k[inside], g[inside], ddx[inside], ddy[inside]
                step2 = ddx * ddx + ddy * ddy
                if eps2 > 0.0:
                    m.eps = min(m.eps, _low(np.abs(step2 - eps2) / eps2))
                done = step2 < eps2
                converged[k[done]] = True
                run[k[done]] = False
            if lvl == 0:
                still = alive[a]
                status[a[still & ~converged]] = STATUS_MAX_ITER
                g = a[still]
                J = sample(imj, pl[still, 0] + d[g, 0], pl[still, 1] + d[g, 1], off, off)
                ee = total(np.abs(I[still] - J).astype(np.float64), order) / ww
                fin = np.isfinite(ee)
                err[g[fin]] = ee[fin]
                status[g[~fin]] = STATUS_NOT_FINITE
                alive[g[~fin]] = False
            else:
                d[a] = 2.0 * d[a]
    u, v = np.where(alive, d[:, 0], np.nan), np.where(alive, d[:, 1], np.nan)
    err = np.where(alive, err, np.nan)
    lam0[bad] = np.nan
    return u, v, err, lam0, n_iter, status, scale_err, scale_eig


def _per_pair(a, pairs, what):
    """(N, 2) for every pair or (pairs, N, 2) -> (pairs, N, 2)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        a = np.broadcast_to(a, (pairs,) + a.shape)
    assert a.ndim == 3 and a.shape[0] == pairs and a.shape[2] == 2, what
    return a


def track_pairs(frames, points, window=21, levels=3, max_iter=20, eps=0.01, min_eig=0.0, guess=None, order="numpy"):
    """dict of u, v, err, min_eig (T - 1, N) float64, n_iter int32, status uint8, err_scale and eig_scale (sum |I| / w^2 and
    (Gxx + Gyy) / w^2 of level 0's template: what a gate on err and on min_eig is relative to), and "margins" (Margins)."""
    f = np.asarray(frames)
    T, H, W = f.shape
    assert f.dtype in (np.uint8, np.float32) and T >= 2 and failing_level(H, W, levels) is None
    assert window % 2 == 1 and MIN_WINDOW <= window <= MAX_WINDOW and 1 <= levels <= MAX_LEVELS and 1 <= max_iter <= MAX_ITER
    pts = _per_pair(points, T - 1, "points")
    gs = None if guess is None else _per_pair(guess, T - 1, "guess")
    pyr = pyramid(f, levels)
    m = Margins()
    out = [track_pair([q[t] for q in pyr], [q[t + 1] for q in pyr], pts[t], window, max_iter, eps, min_eig,
                      None if gs is None else gs[t], order, m) for t in range(T - 1)]
    names = ("u", "v", "err", "min_eig", "n_iter", "status", "err_scale", "eig_scale")
    res = {n: np.stack([o[i] for o in out]) for i, n in enumerate(names)}
    res["margins"] = m
    return res


def trajectories(frames, points0, **kw):
    """xy (T, N, 2): row 0 = points0, row t + 1 = row t + (u, v) of pair t tracked from row t; NaN once lost (status 5 from then on)."""
    f = np.asarray(frames)
    T = f.shape[0]
    levels = kw.pop("levels", 3)
    order = kw.pop("order", "numpy")
    pyr = pyramid(f, levels)
    xy = np.empty((T,) + np.asarray(points0).shape)
    xy[0] = points0
    m = Margins()
    out = []
    for t in range(T - 1):
        o = track_pair([q[t] for q in pyr], [q[t + 1] for q in pyr], xy[t], order=order, margins=m, **kw)
        out.append(o)
        xy[t + 1, :, 0] = xy[t, :, 0] + o[0]
        xy[t + 1, :, 1] = xy[t, :, 1] + o[1]
    names = ("u", "v", "err", "min_eig", "n_iter", "status", "err_scale", "eig_scale")
    res = {n: np.stack([o[i] for o in out]) for i, n in enumerate(names)}
    res["xy"], res["margins"] = xy, m
    return res


def grid_points(H, W, window_size, overlap=None):
    """The centres of the PIV grid as points (rows * cols, 2) and its shape: pyorc_amd.window.get_rect_coordinates."""
    from pyorc_amd import window

    ov = window_size // 2 if overlap is None else overlap
    x, y = window.get_rect_coordinates((H, W), (window_size, window_size), (ov, ov))
    xx, yy = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    return np.stack([xx.ravel(), yy.ravel()], axis=1), (len(y), len(x))
