"""Float64 numpy reference of the second correlation peak on the planes of the project's own float64
reference, ``spof_ref.piv(..., fn=spof_ref.ncc_plane)``: the rule, the fit of the runner-up vector by the primary's rule, the windows a
float32 plane cannot be held to it on ("fragile"), the bound on the fit's own motion under plane noise, hand-made planes and the sparse
noisy scene on which the peak ratio is compared with ``s2n``.  Kernel orientation throughout (u column shift, v row shift).

Also the inputs tests/test_peak2_host.py and tests/test_gpu_peak2.py share, computed once per process and never changed."""
import functools
import itertools

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd import synth
from tests import deform_ref, spof_ref

FLOOR = 1e-5            # a candidate is at least this high: five times the project's plane gate
PLANE_GATE = 2e-6       # what a float32 plane of the fused kernels may deviate from the float64 one
PEAK2_WINDOWS = (16, 32, 64)
PASS_CASES = deform_ref.PASS_CASES
RADII = (1, 2, 4)


def candidates(plane, r, margin=0.0, floor=FLOOR):
    """Boolean map of the candidates of one fft-shifted plane: s >= floor, outside the box |i - ip| <= r and |j - jp| <= r around the
    primary (the first maximum in row-major order; the box is clipped at the edge, no wrap), and s + margin * max >= each of its existing
    4-neighbours (a neighbour inside the box counts)."""
    pl = np.asarray(plane, dtype=np.float64)
    wy, wx = pl.shape
    ip, jp = divmod(int(np.argmax(pl)), wx)
    s = pl + margin * pl.max()
    ok = pl >= floor
    ok[max(ip - r, 0):ip + r + 1, max(jp - r, 0):jp + r + 1] = False
    ok[1:] &= s[1:] >= pl[:-1]
    ok[:-1] &= s[:-1] >= pl[1:]
    ok[:, 1:] &= s[:, 1:] >= pl[:, :-1]
    ok[:, :-1] &= s[:, :-1] >= pl[:, 1:]
    return ok


def second_peak(plane, r, margin=0.0, floor=FLOOR):
    """(found, i2, j2, corr2, runner_up): the candidate with the largest value, the first in row-major order among equals; runner_up is
    the value of the largest candidate at another position (0 without one).  Not found: (False, -1, -1, 0.0, 0.0)."""
    pl = np.asarray(plane, dtype=np.float64)
    ok = candidates(pl, r, margin, floor)
    if not ok.any():
        return False, -1, -1, 0.0, 0.0
    vals = np.where(ok, pl, -1.0)
    k = int(np.argmax(vals))                       # first maximum in row-major order
    i2, j2 = divmod(k, pl.shape[1])
    rest = vals.copy().reshape(-1)
    rest[k] = -1.0
    return True, i2, j2, float(pl[i2, j2]), float(max(rest.max(), 0.0))


def fit(five, i, j, wy, wx):
    """(u, v) of the peak at shifted (i, j) by the primary's rule from ``five`` = (c0, up, down, left, right): inside, the 3-point
    log-Gaussian fit on plane + 1e-7 (zero denominator: zero offset); on the border, SEMANTICS["border_peak"].  "v_sign" applies."""
    if i == 0 or i == wy - 1 or j == 0 or j == wx - 1:
        mode = po.SEMANTICS["border_peak"]
        u, v = (np.nan, np.nan) if mode == 0 else (0.0, 0.0) if mode == 1 else (float(j - wx // 2), float(i - wy // 2))
    else:
        with np.errstate(all="ignore"):
            l0, lu, ld, ll, lr = (np.log(np.float64(x) + po.EPS_PEAK) for x in five)
            den_v, den_u = 2 * lu - 4 * l0 + 2 * ld, 2 * ll - 4 * l0 + 2 * lr
            v = i + ((lu - ld) / den_v if den_v != 0.0 else 0.0) - wy // 2
            u = j + ((ll - lr) / den_u if den_u != 0.0 else 0.0) - wx // 2
    return float(u), float(-v if po.SEMANTICS["v_sign"] else v)


def five_samples(plane, i, j):
    """(c0, up, down, left, right) around (i, j); a neighbour outside the plane is 0 (the border rule does not read them)."""
    pl = np.asarray(plane, dtype=np.float64)
    wy, wx = pl.shape
    at = lambda a, b: float(pl[a, b]) if 0 <= a < wy and 0 <= b < wx else 0.0
    return at(i, j), at(i - 1, j), at(i + 1, j), at(i, j - 1), at(i, j + 1)


def plane_result(plane, r):
    """The four outputs of one plane and where they come from: dict(u2, v2, corr2, ratio, found, i2, j2).  A NaN plane (a skipped
    window) is NaN in all four; no candidate: corr2 = 0, ratio = +inf, u2 = v2 = NaN."""
    pl = np.asarray(plane, dtype=np.float64)
    if not np.isfinite(pl).all():
        return dict(u2=np.nan, v2=np.nan, corr2=np.nan, ratio=np.nan, found=False, i2=-1, j2=-1)
    found, i2, j2, c2, _ = second_peak(pl, r)
    if not found:
        return dict(u2=np.nan, v2=np.nan, corr2=0.0, ratio=np.inf, found=False, i2=-1, j2=-1)
    u2, v2 = fit(five_samples(pl, i2, j2), i2, j2, *pl.shape)
    return dict(u2=u2, v2=v2, corr2=c2, ratio=float(pl.max() / c2), found=True, i2=i2, j2=j2)


def fragile_plane(plane, r):
    """A window whose second peak a float32 plane cannot be held to: the runner-up candidate is within 1e-4 (relative) of the second peak,
    or one of the four evaluations at margin = +-1e-4 x floor in {0.5e-5, 2e-5} disagrees with the nominal one on existence or position."""
    pl = np.asarray(plane, dtype=np.float64)
    if not np.isfinite(pl).all():
        return False
    found, i2, j2, c2, runner = second_peak(pl, r)
    if found and c2 - runner <= 1e-4 * c2:
        return True
    for margin, floor in itertools.product((-1e-4, 1e-4), (0.5e-5, 2e-5)):
        if second_peak(pl, r, margin, floor)[:3] != (found, i2, j2):
            return True
    return False


def fit_motion(plane, i, j, d):
    """B: the largest motion of the reference's own fit at (i, j), over u and v, when its five samples move by +-2 d over all 32 sign
    patterns (samples stay >= 0: the planes are clipped).  0 on the border, where nothing is fitted."""
    wy, wx = np.asarray(plane).shape
    if i == 0 or i == wy - 1 or j == 0 or j == wx - 1:
        return 0.0
    five = np.array(five_samples(plane, i, j))
    u0, v0 = fit(five, i, j, wy, wx)
    worst = 0.0
    for signs in itertools.product((-1.0, 1.0), repeat=5):
        u, v = fit(np.maximum(five + 2.0 * d * np.array(signs), 0.0), i, j, wy, wx)
        worst = max(worst, abs(u - u0), abs(v - v0))
    return worst


def on_planes(planes, r, with_fragile=True):
    """:func:`plane_result` over ``planes`` (P, n_win, wy, wx): dict of (P, n_win) arrays u2, v2, corr2, ratio, found, i2, j2[, fragile]
    (fragile here is this module's two clauses only; :func:`piv` adds ``spof_ref.fragile_mask``)."""
    planes = np.asarray(planes)
    P, n_win = planes.shape[:2]
    keys = ("u2", "v2", "corr2", "ratio", "found", "i2", "j2")
    out = {k: np.empty((P, n_win), dtype=bool if k == "found" else np.int64 if k in ("i2", "j2") else np.float64) for k in keys}
    if with_fragile:
        out["fragile"] = np.zeros((P, n_win), dtype=bool)
    for p in range(P):
        for w in range(n_win):
            res = plane_result(planes[p, w], r)
            for k in keys:
                out[k][p, w] = res[k]
            if with_fragile:
                out["fragile"][p, w] = fragile_plane(planes[p, w], r)
    return out


def piv(imgs, n, overlap, r=2, signal_threshold=None):
    """``spof_ref.piv(..., fn=spof_ref.ncc_plane)`` (``overlap`` an int or a pair (oy, ox)) plus the second peak of every plane: u2, v2,
    corr2, ratio, found, i2, j2 as (P, rows, cols), ``fragile2`` = the windows left out of the gates (``spof_ref.fragile_mask`` or :func:`fragile_plane`)."""
    res = dict(spof_ref.piv(imgs, n, overlap, signal_threshold, fn=spof_ref.ncc_plane))
    shape = res["corr"].shape
    second = on_planes(res["planes"], r)
    for k, v in second.items():
        res["own_fragile" if k == "fragile" else k] = v.reshape(shape)
    res["fragile2"] = res["fragile"] | res["own_fragile"]
    return res


@functools.lru_cache(maxsize=None)
def pass_ref(case, dtype=np.uint8, r=2):
    n, ov, _ = PASS_CASES[case]
    return piv(deform_ref.pass_stack(case, dtype), n, ov, r)


@functools.lru_cache(maxsize=None)
def signal_ref(case, r=2):
    n, ov, _ = PASS_CASES[case]
    return piv(deform_ref.signal_stack(case), n, ov, r, deform_ref.SIGNAL_THR)


def fragile_share(res):
    """(fragile windows, finite windows) of a :func:`piv` result."""
    kept = np.isfinite(res["corr"])
    return int((res["fragile2"] & kept).sum()), int(kept.sum())


# ---- hand-made planes ---------------------------------------------------------------------------------------------------------------
def _bump(pl, i, j, height, sigma=0.8):
    """A small Gaussian peak of ``height`` at (i, j), added where it lies inside the plane."""
    wy, wx = pl.shape
    for a in range(max(i - 3, 0), min(i + 4, wy)):
        for b in range(max(j - 3, 0), min(j + 4, wx)):
            pl[a, b] = max(pl[a, b], height * np.exp(-((a - i) ** 2 + (b - j) ** 2) / (2.0 * sigma * sigma)))


def hand_planes(wy, wx):
    """Hand-made float32 planes of wy x wx (both >= 16) and what the rule says about them at r = 2: a list of (name, plane, expected)
    with expected = None (no candidate), "nan" (a skipped window) or the shifted position (i2, j2) of the second peak."""
    cy, cx = wy // 2, wx // 2
    out = []
    z = lambda: np.zeros((wy, wx), dtype=np.float64)
    pl = z(); pl[cy, cx] = 1.0
    out.append(("single delta", pl, None))
    pl = z(); _bump(pl, 0, 0, 0.9); _bump(pl, cy, cx + 1, 0.5)
    out.append(("primary in a corner", pl, (cy, cx + 1)))
    pl = z(); _bump(pl, 5, 6, 0.8); _bump(pl, 0, wx - 3, 0.4)
    out.append(("second peak on the top border", pl, (0, wx - 3)))
    pl = z(); _bump(pl, cy, cx, 0.8); _bump(pl, wy - 4, wx - 1, 0.3)
    out.append(("second peak on the right border", pl, (wy - 4, wx - 1)))
    pl = z(); _bump(pl, cy, cx, 0.9); _bump(pl, wy - 4, 3, 0.4); _bump(pl, 3, wx - 4, 0.4)
    out.append(("two equal second peaks", pl, (3, wx - 4)))
    pl = z(); _bump(pl, cy, cx, 1.0, sigma=2.0)
    out.append(("only the flank of the primary outside the box", pl, None))
    pl = z(); _bump(pl, cy, cx, 1.0, sigma=2.0); _bump(pl, 2, 3, 0.05)
    out.append(("a weak peak beats the primary's flank", pl, (2, 3)))
    pl = z(); _bump(pl, cy, cx, 0.7); _bump(pl, 3, 3, 5e-6)
    out.append(("a peak below the floor", pl, None))
    pl = z(); _bump(pl, cy, cx, 0.7); pl[3, 4] = pl[3, 5] = 0.25
    out.append(("a plateau of two equal samples", pl, (3, 4)))
    pl = z(); _bump(pl, cy - 1, cx + 2, 0.6); _bump(pl, cy + 2, cx + 2, 0.45)
    out.append(("second peak next to the box, its neighbour inside it", pl, (cy + 2, cx + 2)))
    out.append(("NaN plane", np.full((wy, wx), np.nan), "nan"))
    return [(name, np.ascontiguousarray(p, dtype=np.float32), exp) for name, p, exp in out]


HAND_SHAPES = ((16, 16), (32, 32), (64, 64), (24, 24), (16, 40))


# ---- what the peak ratio gains: a sparse noisy scene -----------------------------------------------------------------------------------
TRUTH = (3.3, -2.4)
SPARSE_SEEDS = (5, 6)
SPARSE_WINDOW = (32, 16)


@functools.lru_cache(maxsize=None)
def sparse_stack(seed, density=0.004, sigma=8.0):
    """``synth.particle_stack(4, 160, 200, density, uniform_shift=TRUTH)`` of ``seed`` plus Gaussian noise of ``sigma`` grey levels, uint8."""
    a = synth.particle_stack(4, 160, 200, seed=seed, density=density, uniform_shift=TRUTH).astype(np.float64)
    noise = np.random.default_rng(1000 + seed).normal(0.0, sigma, a.shape)
    return np.clip(np.rint(a + noise), 0, 255).astype(np.uint8)


def auc(score, good):
    """Area under the ROC curve of ``score`` for telling ``good`` from not good (Mann-Whitney, ties at half); NaN scores rank lowest."""
    s = np.where(np.isnan(score), -np.inf, np.asarray(score, dtype=np.float64)).reshape(-1)
    g = np.asarray(good, dtype=bool).reshape(-1)
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    hi = np.cumsum(cnt)
    rank = (hi - (cnt - 1) / 2.0)[inv]              # average ranks, 1-based
    n1, n0 = int(g.sum()), int((~g).sum())
    if n1 == 0 or n0 == 0:
        raise ValueError("auc needs both classes")
    return float((rank[g].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def within_half_px(u, v):
    with np.errstate(invalid="ignore"):
        return np.hypot(np.asarray(u, np.float64) - TRUTH[0], np.asarray(v, np.float64) - TRUTH[1]) <= 0.5


@functools.lru_cache(maxsize=None)
def sparse_ref(seed):
    n, ov = SPARSE_WINDOW
    return piv(sparse_stack(seed), n, ov, 2)


def auc_pair(res_u, res_v, ratio, s2n):
    """(AUC of the peak ratio, AUC of s2n) over all windows."""
    good = within_half_px(res_u, res_v)
    return auc(ratio, good), auc(s2n, good)
