"""Correlation planes with a chosen arg-max, chosen ties, chosen NaN / inf placement and chosen conditioning of the 3-point fit, for
the paths that fit planes with no frames behind them (``u_v_displacement``, ``Ensemble.finish`` on an imported state; csrc/piv_direct.hip,
``peaks_kernel``), and their reference: ``oracle.piv_oracle.u_v_displacement`` on the SAME float32 samples widened to float64.  There is
no plane noise on these paths -- the kernel and the reference read the same numbers -- so the arg-max agrees on every plane and the only
error left is the arithmetic of the fit.  tests/test_peaks_host.py (CPU) and tests/test_gpu_peaks_planes.py share what is made here;
everything is computed once per process and never changed.

Three families:

"argmax"  14 shapes from 1 x 9 to 130 x 257 (sides of 1 and 2, fewer than 64 samples, sample counts that are no multiple of 64); on a
          seeded uniform background in [0, 0.2] one plane per: a single maximum 0.9 at the corners, the edge middles, (1, 1),
          (wy - 2, wx - 2), the centre and the flat indices 0, 63, 64, 65, 127, 128, n - 1 (lane and iteration boundaries of the 64-lane
          strided search); exact two-way ties at p < q = p + 1, p + 63, p + 64, p + 128 and q = n - 1, with p interior and q on the
          border and the other way round; NaN / inf / signed-zero / negative planes.
"fit"     Gaussian peaks bg + h exp(-r^2 / 2 sigma^2) at 4 x 81 sub-pixel centres, sigma 0.7 ... 12, four (h, bg); the same peaks
          clipped so that one, two and four neighbours of the maximum are exactly 0; rows of three equal samples at the maximum.
"many"    70 000 planes of 4 x 4 (more blocks than a 16-bit grid dimension holds)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import piv_oracle as po

TOL = 1e-4          # the project's gate: |got - ref| <= TOL * max(|ref|, FLOOR)  (tests/test_gpu_parity.py)
FLOOR = 0.05

ARGMAX_SHAPES = ((1, 9), (9, 1), (2, 2), (2, 40), (3, 3), (3, 5), (7, 9), (8, 8), (5, 130), (24, 40), (33, 33), (64, 64), (65, 63),
                 (130, 257))
PEAK = np.float32(0.9)
FLAT_MARKS = (0, 63, 64, 65, 127, 128)
TIE_STEPS = (1, 63, 64, 128)

FIT_SIZES = (16, 33, 64)
SIGMAS = (0.7, 1.5, 3.0, 5.0, 8.0, 12.0)
HEIGHTS = ((1.0, 0.0), (0.3, 0.2), (0.02, 0.0), (1e-6, 0.0))      # (h, bg)
GRID = np.linspace(-0.5, 0.5, 9)
FINE = 0.08
# clipped variants: offsets whose four neighbours of the maximum all differ (|dy| != |dx|, neither 0 nor 0.5)
CLIP_OFFSETS = ((0.125, -0.375), (-0.375, 0.125), (0.25, 0.125), (-0.125, 0.25), (0.375, -0.25), (-0.25, -0.375))
CLIP_SIGMAS = (0.7, 1.5, 3.0)

MANY = 70000

Family = namedtuple("Family", "planes labels")      # planes (k, wy, wx) float32; labels: k strings
FitFamily = namedtuple("FitFamily", "planes kind sigma h bg")   # per plane: kind "gauss" / "clip1" / "clip2" / "clip4" / "row3"


def _interior(o, wy, wx):
    i, j = divmod(o, wx)
    return 0 < i < wy - 1 and 0 < j < wx - 1


@functools.lru_cache(maxsize=None)
def argmax_family(shape):
    wy, wx = shape
    n = wy * wx
    rng = np.random.default_rng(7000 + 1000 * wy + wx)
    planes, labels = [], []

    def background():
        return rng.uniform(0.0, 0.2, n).astype(np.float32)

    def add(label, flat):
        planes.append(np.asarray(flat, np.float32).reshape(wy, wx))
        labels.append(label)

    # ---- one maximum
    spots = {}
    for name, (i, j) in (("corner00", (0, 0)), ("corner01", (0, wx - 1)), ("corner10", (wy - 1, 0)), ("corner11", (wy - 1, wx - 1)),
                         ("edge-top", (0, wx // 2)), ("edge-bottom", (wy - 1, wx // 2)), ("edge-left", (wy // 2, 0)),
                         ("edge-right", (wy // 2, wx - 1)), ("one-one", (1, 1)), ("last-but-one", (wy - 2, wx - 2)),
                         ("centre", (wy // 2, wx // 2))):
        if 0 <= i < wy and 0 <= j < wx:
            spots.setdefault(i * wx + j, name)
    for o in FLAT_MARKS + (n - 1,):
        if o < n:
            spots.setdefault(o, f"flat{o}")
    for o, name in sorted(spots.items()):
        b = background()
        b[o] = PEAK
        add(f"max-{name}", b)

    # ---- exact two-way ties, the winner is p
    def first_pair(step, p_interior):
        for p in range(n):
            q = n - 1 if step is None else p + step
            if p < q < n and _interior(p, wy, wx) == p_interior and _interior(q, wy, wx) != p_interior:
                return p, q
        return None

    for step in TIE_STEPS + (None,):
        found = [pq for pq in (first_pair(step, True), first_pair(step, False)) if pq]
        if not found:       # a shape without interior (a side of 1 or 2): any pair at that distance
            p, q = 0, (n - 1 if step is None else step)
            found = [(p, q)] if p < q < n else []
        for p, q in found:
            b = background()
            b[p] = b[q] = PEAK
            add(f"tie-{'last' if step is None else step}-p{p}-q{q}", b)

    # ---- NaN, inf, zeros, negative samples
    inner = [o for o in range(n) if _interior(o, wy, wx)]
    if inner:
        a, m, z = inner[0], inner[len(inner) // 2], inner[-1]
    else:
        a, m, z = 0, n // 2, n - 1
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    if a < m:
        b = background(); b[a] = PEAK; b[m] = nan; add("nan-after-max", b)
        b = background(); b[a] = nan; b[m] = PEAK; add("nan-before-max", b)
    if a < m < z:
        b = background(); b[a] = inf; b[m] = nan; b[z] = inf; add("inf-nan-inf", b)
        b = background(); b[a] = nan; b[m] = inf; b[z] = nan; add("nan-inf-nan", b)
    add("all-nan", np.full(n, nan))
    add("all-minus-inf", np.full(n, -inf))
    add("all-zero", np.zeros(n))
    add("all-0.37", np.full(n, 0.37))
    b = np.zeros(n, np.float32); b[::2] = -0.0; add("signed-zeros-minus-first", b)
    b = np.zeros(n, np.float32); b[1::2] = -0.0; add("signed-zeros-plus-first", b)
    if inner:
        b = np.full(n, -0.5, np.float32); b[m] = -0.1; add("negative-max", b)
        b = background(); b[m] = PEAK; b[m - 1] = -0.1; add("negative-neighbour-u", b)
        b = background(); b[m] = PEAK; b[m + wx] = -0.1; add("negative-neighbour-v", b)
    out = np.ascontiguousarray(np.stack(planes))
    out.setflags(write=False)
    return Family(out, tuple(labels))


def fit_centres(n):
    """(324, 2) peak centres (y, x): the plane centre, and two samples off it along each axis, each plus the 9 x 9 offset grid over
    [-0.5, 0.5]^2; and the plane centre plus that grid shrunk to [-0.04, 0.04]^2 -- displacements under the gate's floor of 0.05 px, where
    the gate is an absolute 5e-6 px (without these the family stays under the 5 % of planes outside the gate in float32 that
    tests/test_peaks_host.py asks of it)."""
    c = float(n // 2)
    oy, ox = (g.ravel() for g in np.meshgrid(GRID, GRID, indexing="ij"))
    wide = [np.stack([c + by + oy, c + bx + ox], axis=1) for by, bx in ((0.0, 0.0), (2.0, 0.0), (0.0, 2.0))]
    return np.concatenate(wide + [np.stack([c + FINE * oy, c + FINE * ox], axis=1)])


def _gauss(n, cy, cx, sigma, h, bg):
    wy, wx = (n, n) if np.isscalar(n) else n
    y, x = np.arange(wy, dtype=np.float64), np.arange(wx, dtype=np.float64)
    r2 = (y[None, :, None] - np.asarray(cy)[:, None, None]) ** 2 + (x[None, None, :] - np.asarray(cx)[:, None, None]) ** 2
    return (bg + h * np.exp(-r2 / (2.0 * sigma * sigma))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_family(n):
    planes, kind, sig, hh, bb = [], [], [], [], []

    def add(p, k, sigma, h, bg):
        planes.append(p)
        kind.extend([k] * len(p)); sig.extend([sigma] * len(p)); hh.extend([h] * len(p)); bb.extend([bg] * len(p))

    cen = fit_centres(n)
    sigmas = [s for s in SIGMAS if n > 16 or s <= 3.0]
    for sigma in sigmas:
        for h, bg in HEIGHTS:
            add(_gauss(n, cen[:, 0], cen[:, 1], sigma, h, bg), "gauss", sigma, h, bg)
    # clipped: max(g - t, 0) in float32 with t = the smallest, the second smallest, the largest neighbour of the maximum
    c = n // 2
    for sigma in CLIP_SIGMAS:
        g = _gauss(n, [c + dy for dy, _ in CLIP_OFFSETS], [c + dx for _, dx in CLIP_OFFSETS], sigma, 1.0, 0.0)
        nb = np.sort(np.stack([g[:, c - 1, c], g[:, c + 1, c], g[:, c, c - 1], g[:, c, c + 1]], axis=1), axis=1)
        assert np.all(np.diff(nb, axis=1) > 0) and np.all(nb[:, 3] < g[:, c, c])
        for name, col in (("clip1", 0), ("clip2", 1), ("clip4", 3)):
            add(np.maximum(g - nb[:, col][:, None, None], np.float32(0.0)), name, sigma, 1.0, 0.0)
    # three equal samples in a row at the maximum: the first of them is the arg-max, its right neighbour equals it
    rng = np.random.default_rng(9100 + n)
    rows = []
    for i, j in ((c, c), (1, 1), (n - 2, n - 4), (c - 3, 2)):
        b = rng.uniform(0.0, 0.2, (n, n)).astype(np.float32)
        b[i, j:j + 3] = PEAK
        rows.append(b)
    add(np.stack(rows), "row3", 0.0, 0.9, 0.1)
    out = np.ascontiguousarray(np.concatenate(planes))
    out.setflags(write=False)
    return FitFamily(out, np.array(kind), np.array(sig), np.array(hh), np.array(bb))


@functools.lru_cache(maxsize=None)
def ensemble_planes(window, n_win):
    """n_win "fit"-family planes of a window (wy, wx) for an imported ensemble state: Gaussian peaks that walk through the sigmas the window
    holds, the four (h, bg) and seeded centres of the offset grids -- exact ties at +-0.5 among them."""
    wy, wx = window
    rng = np.random.default_rng(5300 + 100 * wy + wx)
    sigmas = [s for s in SIGMAS if s <= min(wy, wx) / 3.0]
    grid = np.concatenate([GRID, FINE * GRID])
    out = []
    for k in range(n_win):
        sigma = sigmas[k % len(sigmas)]
        h, bg = HEIGHTS[(k // len(sigmas)) % len(HEIGHTS)]
        cy = wy // 2 + rng.choice(grid) + (1.0 if k % 5 == 0 and wy > 6 else 0.0)
        cx = wx // 2 + rng.choice(grid) - (1.0 if k % 7 == 0 and wx > 6 else 0.0)
        out.append(_gauss((wy, wx), [cy], [cx], sigma, h, bg)[0])
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def many_family():
    rng = np.random.default_rng(4242)
    p = rng.uniform(0.0, 0.2, (MANY, 4, 4)).astype(np.float32)
    k = np.arange(MANY)
    p[k, 1 + (k & 1), 1 + ((k >> 1) & 1)] = rng.uniform(0.5, 1.0, MANY).astype(np.float32)
    p.setflags(write=False)
    return p


def _reference(planes, **sem):
    with po.semantics(**sem):
        u, v = po.u_v_displacement(np.asarray(planes, np.float64)[None], 1, len(planes))
    return u.ravel(), v.ravel()


@functools.lru_cache(maxsize=None)
def argmax_reference(shape, border_peak=0, v_sign=0):
    return _reference(argmax_family(shape).planes, border_peak=border_peak, v_sign=v_sign)


@functools.lru_cache(maxsize=None)
def fit_reference(n):
    return _reference(fit_family(n).planes)


@functools.lru_cache(maxsize=None)
def many_reference():
    return _reference(many_family())


def reference(planes, **sem):
    """(u, v) float64, one per plane of (k, wy, wx) float32 planes: the float64 fit on those very samples."""
    return _reference(planes, **sem)


def bound(ref, side):
    """The gate per value: TOL * max(|ref|, FLOOR); above 64 samples per side plus one float32 ulp of side / 2 -- the result is formed
    as (float)i + offset - side / 2 in float32 and cannot be more exact than that."""
    b = TOL * np.maximum(np.abs(ref), FLOOR)
    if side > 64:
        b = b + float(np.spacing(np.float32(side // 2)))
    return b


def rel_error(got, ref):
    """|got - ref| / max(|ref|, FLOOR) where both are finite (NaN elsewhere)."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), FLOOR)


def assert_within_gate(got_u, got_v, ref_u, ref_v, shape, what):
    """NaN masks equal on every plane, every finite value within the gate; returns the worst relative error."""
    wy, wx = shape
    worst = 0.0
    for got, ref, side, name in ((got_u, ref_u, wx, "u"), (got_v, ref_v, wy, "v")):
        got = np.asarray(got).ravel()
        assert got.dtype == np.float32 and got.shape == ref.shape, (what, name)
        bad = np.nonzero(np.isnan(got) != np.isnan(ref))[0]
        assert bad.size == 0, f"{what}: {name} NaN mask differs on planes {bad[:8].tolist()} ({bad.size} in all)"
        fin = ~np.isnan(ref)
        assert np.all(np.isfinite(got[fin])), (what, name, "non-finite value where the reference is finite")
        err = np.abs(got[fin].astype(np.float64) - ref[fin])
        over = err > bound(ref[fin], side)
        rel = rel_error(got[fin], ref[fin])
        if rel.size:
            worst = max(worst, float(rel.max()))
        idx = np.nonzero(fin)[0][over]
        assert idx.size == 0, (f"{what}: {name} outside the gate on {idx.size} of {fin.sum()} planes, first {idx[:8].tolist()}, "
                               f"worst relative error {rel.max():.3e}")
    return worst
