"""The inputs that the CPU and the GPU tests of pyorc_amd.track share (tests/test_track_host.py qualifies them on the reference,
tests/test_gpu_track.py runs them on the GPU), and the reference's results on them, computed once per process.

The scenes are small on purpose: 33 x 47 and 48 x 64, a smooth random texture that moves by a sub-pixel shift per frame, so that
a 5-px window at one level converges as well as a 31-px window at four.  The points cover what the tracker can meet: see points().

CASES is the first table (tests index it by position); VARIANT_CASES has one case for each of the kernel's 28 (window, dtype) instances,
five levels on 97 x 127 among them; NOT_FINITE_CASES put one NaN, +inf or -inf sample into a scene; FAR_CASES hand over guesses beyond
the kernel's index clamp."""
import functools

import numpy as np

from tests import track_ref as tr

SHAPES = ((33, 47), (48, 64))
SHIFT = (0.7, -0.4)          # px per frame along x and y: towards the right and the top border
FLAT = 20                    # the texture is constant on [0, FLAT) x [0, FLAT): a window at the corner (0, 0) sees no gradient
# kind -> the sample that is not finite and its (row, column) in an H x W frame: away from the constant block, and placed so that some
# windows hold it and others do not, at level 1 as well
NOT_FINITE = {
    "float32-nan": (np.nan, lambda H, W: (H // 2 + 3, W // 2 - 5)),
    "float32-inf": (np.inf, lambda H, W: (H // 8, W - 7)),
    "float32-ninf": (-np.inf, lambda H, W: (5 * H // 6, W - 14)),
}


@functools.lru_cache(maxsize=None)
def scene(shape, T, kind):
    """(T, H, W) frames: kind "uint8", "float32" (unrounded, offset by -100) or "float32-nan", "float32-inf", "float32-ninf" (one NaN,
    +inf or -inf sample in frame 1: NOT_FINITE).  A Gaussian-filtered random texture (sigma 1.6 px) on a periodic canvas of 128 samples
    a side, moved by SHIFT per frame with a Fourier shift; a constant block at the top left corner."""
    H, W = shape
    n = 128
    rng = np.random.default_rng(H * 100 + W)
    ky, kx = np.fft.fftfreq(n)[:, None], np.fft.fftfreq(n)[None, :]
    spec = np.fft.fft2(rng.normal(size=(n, n))) * np.exp(-2.0 * (np.pi * 1.6) ** 2 * (kx * kx + ky * ky))
    base = np.fft.ifft2(spec).real
    scale = 45.0 / base.std()
    frames = np.empty((T, H, W))
    for t in range(T):
        moved = np.fft.ifft2(spec * np.exp(-2j * np.pi * (kx * SHIFT[0] + ky * SHIFT[1]) * t)).real
        frames[t] = 128.0 + scale * moved[:H, :W]
    frames[:, :FLAT, :FLAT] = 77.0
    if kind == "uint8":
        out = np.clip(np.rint(frames), 0, 255).astype(np.uint8)
    else:
        out = (frames - 100.0).astype(np.float32)
        if kind in NOT_FINITE:      # (frame 1 is pair 0's J and, from T = 3 on, pair 1's template)
            value, at = NOT_FINITE[kind]
            out[(1,) + at(H, W)] = value
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def points(shape, N):
    """N points (x, y), the special ones first: a generic fractional position; an integer position (fx = fy = 0); the corner
    (W - 1, H - 1); the corner (0, 0), which sits on the constant block (status 2); the corners (W - 1, 0) and (0, H - 1); a point next
    to the right border, which the motion walks out (status 3); one more integer position; then random positions."""
    H, W = shape
    special = [[W / 2 + 0.37, H / 2 - 0.21], [W // 2 + 4.0, H // 2 + 3.0], [W - 1.0, H - 1.0], [0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0],
               [W - 1.25, H / 2 + 0.5], [FLAT + 6.0, FLAT + 2.0]]
    rng = np.random.default_rng(N * 7 + H)
    rand = np.stack([rng.uniform(0.0, W - 1.0, max(N, 8)), rng.uniform(0.0, H - 1.0, max(N, 8))], axis=1)
    p = np.concatenate([np.array(special), rand])[:N]
    p.setflags(write=False)
    return p


# (shape, kind, T, N, window, levels): every T in {2, 3, 5}, N in {1, 3, 64, 65, 200}, window in {5, 9, 15, 21, 31} (and 17, 19: the last
# window whose template stays in registers and the first whose does not), levels 1 .. 4, both dtypes, both shapes
CASES = [
    ((33, 47), "uint8", 2, 1, 5, 1),
    ((33, 47), "float32", 3, 3, 9, 2),
    ((48, 64), "uint8", 5, 64, 15, 3),
    ((48, 64), "float32", 2, 65, 21, 4),
    ((33, 47), "uint8", 3, 200, 31, 1),
    ((48, 64), "uint8", 2, 65, 31, 3),
    ((33, 47), "float32", 5, 65, 21, 3),
    ((48, 64), "float32-nan", 3, 200, 9, 3),
    ((33, 47), "uint8", 2, 64, 17, 4),
    ((48, 64), "float32", 3, 200, 19, 2),
    ((48, 64), "uint8", 3, 65, 5, 2),
]
# One case for each of the 28 instances of lk_track_kernel<T, WIN> (window 5, 7, .. 31 in uint8 and float32), so that a slip in one
# instance's unroll counts, tail trip, lane-past-the-window weight or patch index cannot pass: NS = ceil(w^2 / 64) runs over 1 .. 16,
# windows up to 17 keep the template in registers ("register family"), windows from 19 read it back from the patch in groups of four
# ("patch family": 23 -> NS 9, 25 -> 10, 27 -> 12 and 29 -> 14 are no multiples of the group).  N = 65: with four waves per block, T = 2
# is 16 full blocks and one block with a single live wave, T = 3 is 32 blocks and two waves.  With i = (w - 5) / 2: one dtype (uint8 for
# even i) on 33 x 47 at 1 + i mod 4 levels, the other on 48 x 64 at 1 + (i + 2) mod 4 levels; T alternates.  Five levels (MAX_LEVELS:
# p.pyr[4], ldexp(guess, -4)) stand in the second place for w = 7, 13 (registers) and 23, 29 (patch), in both dtypes of each family, on
# 97 x 127 -- 48 x 64 has a level 4 of 3 x 4, out of which the reference walks half of the points.  tests/test_track_host.py qualifies
# every case; all 28 qualified on their first shape, level count, T and N, so none had to be moved.
VARIANT_N = 65
VARIANT_CASES = [
    ((33, 47), "uint8", 2, VARIANT_N, 5, 1),
    ((48, 64), "float32", 3, VARIANT_N, 5, 3),
    ((33, 47), "float32", 3, VARIANT_N, 7, 2),
    ((97, 127), "uint8", 3, VARIANT_N, 7, 5),
    ((33, 47), "uint8", 2, VARIANT_N, 9, 3),
    ((48, 64), "float32", 3, VARIANT_N, 9, 1),
    ((33, 47), "float32", 3, VARIANT_N, 11, 4),
    ((48, 64), "uint8", 2, VARIANT_N, 11, 2),
    ((33, 47), "uint8", 2, VARIANT_N, 13, 1),
    ((97, 127), "float32", 3, VARIANT_N, 13, 5),
    ((33, 47), "float32", 3, VARIANT_N, 15, 2),
    ((48, 64), "uint8", 2, VARIANT_N, 15, 4),
    ((33, 47), "uint8", 2, VARIANT_N, 17, 3),
    ((48, 64), "float32", 3, VARIANT_N, 17, 1),
    ((33, 47), "float32", 3, VARIANT_N, 19, 4),
    ((48, 64), "uint8", 2, VARIANT_N, 19, 2),
    ((33, 47), "uint8", 2, VARIANT_N, 21, 1),
    ((48, 64), "float32", 3, VARIANT_N, 21, 3),
    ((33, 47), "float32", 3, VARIANT_N, 23, 2),
    ((97, 127), "uint8", 3, VARIANT_N, 23, 5),
    ((33, 47), "uint8", 2, VARIANT_N, 25, 3),
    ((48, 64), "float32", 3, VARIANT_N, 25, 1),
    ((33, 47), "float32", 3, VARIANT_N, 27, 4),
    ((48, 64), "uint8", 2, VARIANT_N, 27, 2),
    ((33, 47), "uint8", 2, VARIANT_N, 29, 1),
    ((97, 127), "float32", 3, VARIANT_N, 29, 5),
    ((33, 47), "float32", 3, VARIANT_N, 31, 2),
    ((48, 64), "uint8", 2, VARIANT_N, 31, 4),
]
REG_WINDOW = 17              # kRegWindow of track.hip: the largest window whose template stays in registers
VARIANT_MODES = ("fixed2", "converge", "converge-min-eig", "converge-guess")
LANE_MODES = ("fixed2", "converge-guess")      # what is compared bit for bit with the reference summed in the kernel's order
FIVE_LEVEL_CASE = VARIANT_CASES[19]            # w = 23, uint8, T = 3: the workspace batches, the upload chunks and trajectories at five levels

# One sample that is not finite, in both families: T = 3, so that the sample is in pair 1's template as well (the patch family forms
# Ix, Iy from the patch anew in every iteration) and in pair 0's J (inf - inf inside the blend; the isfinite tests on the sums); one
# and two levels and windows that leave most points clear of it (test_track_host.py: some status 4, a third of the points tracked).
NOT_FINITE_CASES = [
    ((48, 64), "float32-nan", 3, 200, 13, 2),
    ((48, 64), "float32-nan", 3, 200, 19, 1),
    ((48, 64), "float32-inf", 3, 200, 11, 1),
    ((48, 64), "float32-inf", 3, 200, 19, 2),
    ((48, 64), "float32-ninf", 3, 200, 15, 2),
    ((48, 64), "float32-ninf", 3, 200, 23, 1),
]

# Guesses far outside the frame, on one variant case of each family at three levels: split() clamps the position to +-2^30 before any
# index arithmetic and bilinear() clamps the indices to the level, so the reference's status 3 after one iteration is the kernel's
FAR_CASES = [VARIANT_CASES[12], VARIANT_CASES[17]]      # w = 17, uint8, 33 x 47 and w = 21, float32, 48 x 64
FAR_POINTS = {0: (1e12, -1e12), 8: (-3e9, 0.3)}         # point -> guess: the generic point and the first random one, in every pair
EXTRA_RUNS = ([(c, m) for c in NOT_FINITE_CASES for m in VARIANT_MODES]
              + [(c, "far-guess") for c in FAR_CASES])   # (the lane-order bits: LANE_MODES on NOT_FINITE_CASES, "far-guess" on FAR_CASES)

MIN_EIG_QUANTILE = 0.3       # see min_eig_for

# name -> keyword arguments of track_pairs; "guess" is filled in per case, and so is "min_eig" for VARIANT_CASES and NOT_FINITE_CASES
# (see kwargs)
MODES = {
    "fixed1": dict(eps=0.0, max_iter=1),
    "fixed2": dict(eps=0.0, max_iter=2),
    "fixed5": dict(eps=0.0, max_iter=5),
    "converge": dict(eps=0.01, max_iter=20),
    "converge-min-eig": dict(eps=0.01, max_iter=20, min_eig=30.0),
    "converge-guess": dict(eps=0.01, max_iter=20, guess=True),
}
# (apart from MODES: every test over CASES x MODES stays as it is)
EXTRA_MODES = {
    "far-guess": dict(eps=0.01, max_iter=20, guess="far"),
}


def case_id(case):
    shape, kind, T, N, w, L = case
    return f"{shape[0]}x{shape[1]}-{kind}-T{T}-N{N}-w{w}-L{L}"


def guess_for(case):
    """(T - 1, N, 2): the true shift, off by up to 0.6 px, different for every point and pair."""
    shape, kind, T, N, w, L = case
    rng = np.random.default_rng(N + 31 * T)
    return np.array(SHIFT) + rng.uniform(-0.6, 0.6, size=(T - 1, N, 2))


def kwargs(case, mode):
    shape, kind, T, N, w, L = case
    kw = dict(MODES[mode] if mode in MODES else EXTRA_MODES[mode], window=w, levels=L)
    if kw.get("guess"):
        g = guess_for(case)
        if kw["guess"] == "far":
            for n, far in FAR_POINTS.items():
                g[:, n] = far
        kw["guess"] = g
    if "min_eig" in kw and (case in VARIANT_CASES or case in NOT_FINITE_CASES):
        kw["min_eig"] = min_eig_for(case)
    return kw


@functools.lru_cache(maxsize=None)
def min_eig_for(case):
    """The min_eig of a case of its own (CASES keep MODES' 30.0): the MIN_EIG_QUANTILE quantile -- the middle between the two order
    statistics around it, so that no point sits on it -- of the eigenvalue that decides, over the points that the determinant test
    keeps in mode "converge".  At one level that is the reference's min_eig output.  At more levels it is the smallest of the point's
    lambdas over the levels, each the reference's min_eig output of a one-level run on that level of the pyramid (the template does not
    depend on d): the lambdas shrink with the level (w = 29 on 97 x 127: median 225 at level 0, 12 at level 4, which every window nearly
    covers), so that a quantile of level 0's alone loses every point of a deep case at its coarsest level, as 30.0 did."""
    shape, kind, T, N, w, L = case
    f, p = scene(shape, T, kind), points(shape, N)
    lam = np.stack([tr.track_pairs(level, np.ldexp(p, -lvl), window=w, levels=1, max_iter=1)["min_eig"]
                    for lvl, level in enumerate(tr.pyramid(f, L))])
    lowest = np.fmin.reduce(lam, axis=0)                   # (fmin: a level whose sums are not finite has no lambda)
    kept = (reference(case, "converge")["status"] != tr.STATUS_LOST) & np.isfinite(lowest)
    s = np.sort(lowest[kept])
    k = int(MIN_EIG_QUANTILE * len(s))
    return float(0.5 * (s[k - 1] + s[k]))


@functools.lru_cache(maxsize=None)
def reference(case, mode, order="numpy"):
    """tests/track_ref.py on a case: computed once, shared by every test that needs it, never written to."""
    shape, kind, T, N, w, L = case
    r = tr.track_pairs(scene(shape, T, kind), points(shape, N), order=order, **kwargs(case, mode))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference_trajectories(case):
    """tests/track_ref.py's trajectories on a case with the defaults of track.trajectories: computed once, never written to."""
    shape, kind, T, N, w, L = case
    r = tr.trajectories(scene(shape, T, kind), points(shape, N), window=w, levels=L)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the trajectory and time-slice inputs -------------------------------------------------------------------------------------------------
TRAJ_CASE = ((48, 64), "uint8", 5, 65, 15, 2)
CHUNK_CASE = ((48, 64), "uint8", 5, 65, 15, 3)     # 4 pairs: slices of 2 + 2 pairs, and 1 + 3 (an odd start)

# ---- the accuracy study -------------------------------------------------------------------------------------
STUDY_SHAPE = (160, 200)
STUDY_SHIFT = (9.3, -6.4)


@functools.lru_cache(maxsize=None)
def study_scene(flow, density):
    """Two frames of synth.particle_stack, 160 x 200: flow "shift" (uniform 9.3 / -6.4 px) or "sine" (the default flow)."""
    from pyorc_amd.synth import particle_stack

    f = particle_stack(2, *STUDY_SHAPE, density=density, uniform_shift=STUDY_SHIFT if flow == "shift" else None)
    f.setflags(write=False)
    return f


def study_truth(flow, pts):
    """(u, v) at the points."""
    if flow == "shift":
        return np.full(len(pts), STUDY_SHIFT[0]), np.full(len(pts), STUDY_SHIFT[1])
    from pyorc_amd.synth import flow_field

    return flow_field(*STUDY_SHAPE, pts[:, 1], pts[:, 0])


def study_figures(r, truth):
    """(share within 0.5 px of all points, median error of the tracked ones, lost count) of one pair's result."""
    e = np.hypot(r["u"][0] - truth[0], r["v"][0] - truth[1])
    lost = int((r["status"][0] >= 2).sum())
    return float(np.mean(e < 0.5)), float(np.nanmedian(e)) if lost < e.size else float("nan"), lost
