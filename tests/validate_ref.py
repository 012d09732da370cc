"""Float32 numpy restatement of the vector validation (include/lspiv.h, "Vector validation"): the normalised
median test over the 3 x 3 neighbourhood with the runner-up vector as the first substitute -- ``np.sort`` with NaN last,
``take_along_axis`` at ``(n - 1) // 2`` and ``n // 2``, every operation a single float32 operation -- and nothing else.

Also the inputs tests/test_validate_host.py and tests/test_gpu_validate.py share, computed once per process and never changed.  The sign
of a zero median is not defined by a sort: every gate compares values (``np.array_equal(..., equal_nan=True)``), not bit patterns."""
import functools

import numpy as np

F32 = np.float32
OFFSETS = tuple((di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0))


def _neighbours(a):
    """(8, T, R, C): the eight neighbours of every position of ``a`` (T, R, C), NaN outside the grid (no wrap)."""
    T, R, C = a.shape
    pad = np.full((T, R + 2, C + 2), np.nan, dtype=F32)
    pad[:, 1:-1, 1:-1] = a
    return np.stack([pad[:, 1 + di:1 + di + R, 1 + dj:1 + dj + C] for di, dj in OFFSETS])


def _median(x_sorted, n):
    """Median of the first ``n`` of the ascending ``x_sorted`` (8, ...): the middle one for odd n, 0.5f * (the two middle ones) for even n.
    (n = 0: whatever sits at position 0 -- such a vector is never judged.)"""
    lo = np.take_along_axis(x_sorted, (np.maximum(n - 1, 0) // 2)[None], axis=0)[0]
    hi = np.take_along_axis(x_sorted, (n // 2).clip(max=7)[None], axis=0)[0]
    return np.where(n % 2 == 1, lo, F32(0.5) * (lo + hi)).astype(F32)


def step(u, v, flag, second, threshold, epsilon, min_neighbours, replace):
    """One Jacobi iteration: new (u, v, flag, n) from the fields of the iteration before; ``n`` the neighbour counts it saw."""
    tau, eps = F32(threshold), F32(epsilon)
    with np.errstate(all="ignore"):
        un, vn = _neighbours(u), _neighbours(v)
        ok = np.isfinite(un) & np.isfinite(vn)
        un, vn = np.where(ok, un, F32(np.nan)), np.where(ok, vn, F32(np.nan))
        n = ok.sum(axis=0)
        um, vm = _median(np.sort(un, axis=0), n), _median(np.sort(vn, axis=0), n)
        ru = _median(np.sort(np.abs(un - um[None]), axis=0), n)
        rv = _median(np.sort(np.abs(vn - vm[None]), axis=0), n)
        lu, lv = tau * (ru + eps), tau * (rv + eps)
        judged = np.isfinite(u) & np.isfinite(v) & (n >= min_neighbours)
        outlier = judged & ((np.abs(u - um) > lu) | (np.abs(v - vm) > lv))
        sub = np.zeros_like(outlier)
        if second is not None:
            u2, v2 = second[..., 0], second[..., 1]
            sub = outlier & (flag == 0) & np.isfinite(u2) & np.isfinite(v2) & ~((np.abs(u2 - um) > lu) | (np.abs(v2 - vm) > lv))
    rest = outlier & ~sub
    u, v, flag = u.copy(), v.copy(), flag.copy()
    if second is not None:
        u[sub], v[sub], flag[sub] = second[..., 0][sub], second[..., 1][sub], 2
    if replace == "nan":
        u[rest], v[rest], flag[rest] = np.nan, np.nan, 1
    else:
        u[rest], v[rest], flag[rest] = um[rest], vm[rest], 3
    return u, v, flag, n


def median_test(u, v, second=None, threshold=2.0, epsilon=0.1, min_neighbours=3, replace="nan", iterations=1, history=None):
    """``(u, v, flag)`` after ``iterations`` iterations on float32 ``(T, R, C)`` fields; new arrays.  ``history``: a list that receives every
    iteration's ``(u, v, flag, n)``."""
    u, v = np.array(u, dtype=F32), np.array(v, dtype=F32)
    second = None if second is None else np.asarray(second, dtype=F32)
    flag = np.zeros(u.shape, dtype=np.uint8)
    for _ in range(iterations):
        u, v, flag, n = step(u, v, flag, second, threshold, epsilon, min_neighbours, replace)
        if history is not None:
            history.append((u, v, flag, n))
    return u, v, flag


def same(a, b):
    """Equality by value, NaN positions included."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------
GRIDS = ((1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 2), (3, 3, 3), (2, 5, 7), (3, 37, 131))


@functools.lru_cache(maxsize=None)
def field(grid):
    """``(u, v, peak2)`` on ``grid`` = (T, R, C), seeded by it: a smooth field plus 0.05 px noise; 10 % outliers of +-5 px; 10 % NaN; a few
    +-Inf; ``peak2`` (T, R, C, 4) in which half of the outliers carry the true vector as runner-up, a quarter another outlier and the
    rest NaN (elsewhere: a vector 5 px off).  Read-only."""
    T, R, C = grid
    rng = np.random.default_rng(1000 * T + 100 * R + C)
    t, i, j = np.meshgrid(np.arange(T), np.arange(R), np.arange(C), indexing="ij")
    true_u = (3.0 + 0.08 * j - 0.05 * i + 0.3 * t).astype(F32)
    true_v = (-2.0 + 0.06 * i + 0.04 * j - 0.2 * t).astype(F32)
    u = (true_u + rng.normal(0.0, 0.05, grid)).astype(F32)
    v = (true_v + rng.normal(0.0, 0.05, grid)).astype(F32)
    clean_u, clean_v = u.copy(), v.copy()
    kind = rng.random(grid)
    out = kind < 0.10
    sign = lambda: np.where(rng.random(grid) < 0.5, -5.0, 5.0).astype(F32)
    u = np.where(out, u + sign(), u).astype(F32)
    v = np.where(out & (rng.random(grid) < 0.5), v + sign(), v).astype(F32)
    nan = (kind >= 0.10) & (kind < 0.20)
    u[nan & (rng.random(grid) < 0.7)] = np.nan
    v[nan & ~np.isnan(u)] = np.nan
    inf = (kind >= 0.20) & (kind < 0.23)
    u[inf] = np.where(rng.random(grid) < 0.5, -np.inf, np.inf).astype(F32)[inf]
    peak2 = np.empty(grid + (4,), dtype=F32)
    share = rng.random(grid)
    peak2[..., 0] = np.where(share < 0.5, clean_u, np.where(share < 0.75, clean_u + sign(), np.nan))
    peak2[..., 1] = np.where(share < 0.5, clean_v, np.where(share < 0.75, clean_v - sign(), np.nan))
    peak2[..., 0] = np.where(out, peak2[..., 0], clean_u + F32(5.0))
    peak2[..., 1] = np.where(out, peak2[..., 1], clean_v)
    peak2[..., 2] = rng.random(grid).astype(F32) * F32(0.5)
    peak2[..., 3] = F32(1.0) + rng.random(grid).astype(F32)
    for a in (u, v, peak2):
        a.setflags(write=False)
    return u, v, peak2


WRAP_GRID = (2, 4, 6)


@functools.lru_cache(maxsize=None)
def wrap_field():
    """``(u, v)`` on (2, 4, 6): smooth inside every time step, but the last column of each row disagrees with the first column of the next
    row by 10 px (u) and the last row of each time step with the first row of the next by 10 px (v) -- and nothing is an outlier among
    its true neighbours.  A wrap across row ends or time steps in either direction flips flags."""
    T, R, C = WRAP_GRID
    t, i, j = np.meshgrid(np.arange(T), np.arange(R), np.arange(C), indexing="ij")
    # planes: a gradient a along x and a / 2 along y keeps every edge and corner vector inside its limits (the corner has 0.2 px to spare
    # at the default threshold and epsilon), and a (C - 1) - a / 2 = 10 for u; for v, 3 px per row, 1.5 per column and -1 per time step
    # give 3 (R - 1) + 1 = 10
    a = 10.0 / (C - 1.5)
    u = (a * j + 0.5 * a * i).astype(F32)
    v = (3.0 * i + 1.5 * j - 1.0 * t).astype(F32)
    u.setflags(write=False); v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def expected(grid, with_second, replace, iterations, min_neighbours):
    """The reference's ``(u, v, flag)`` on :func:`field` of ``grid``; read-only."""
    u, v, p2 = field(grid)
    res = median_test(u, v, p2 if with_second else None, replace=replace, iterations=iterations, min_neighbours=min_neighbours)
    for a in res:
        a.setflags(write=False)
    return res


def share_within(u, v, truth, among):
    """Share of the positions ``among`` whose vector lies within 0.5 px of ``truth``."""
    with np.errstate(invalid="ignore"):
        good = np.hypot(np.asarray(u, np.float64) - truth[0], np.asarray(v, np.float64) - truth[1]) <= 0.5
    return float((good & among).sum()) / float(among.sum())
