"""The inputs that the CPU and the GPU tests of pyorc_amd.track share (tests/test_track_host.py qualifies them on the reference,
tests/test_gpu_track.py runs them on the GPU), and the reference's results on them, computed once per process.

The scenes are small on purpose: 33 x 47 and 48 x 64, a smooth random texture that moves by a sub-pixel shift per frame, so that
a 5-px window at one level converges as well as a 31-px window at four.  The points cover what the tracker can meet: see points()."""
import functools

import numpy as np

from tests import track_ref as tr

SHAPES = ((33, 47), (48, 64))
SHIFT = (0.7, -0.4)          # px per frame along x and y: towards the right and the top border
FLAT = 20                    # the texture is constant on [0, FLAT) x [0, FLAT): a window at the corner (0, 0) sees no gradient


@functools.lru_cache(maxsize=None)
def scene(shape, T, kind):
    """(T, H, W) frames: kind "uint8", "float32" (unrounded, offset by -100) or "float32-nan" (one NaN sample in frame 1).  A Gaussian-
    filtered random texture (sigma 1.6 px) on a periodic canvas, moved by SHIFT per frame with a Fourier shift; a constant block at the
    top left corner."""
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
        if kind == "float32-nan":
            out[1, H // 2 + 3, W // 2 - 5] = np.nan
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
# name -> keyword arguments of track_pairs; "guess" and "min_eig" are filled in per case (see kwargs)
MODES = {
    "fixed1": dict(eps=0.0, max_iter=1),
    "fixed2": dict(eps=0.0, max_iter=2),
    "fixed5": dict(eps=0.0, max_iter=5),
    "converge": dict(eps=0.01, max_iter=20),
    "converge-min-eig": dict(eps=0.01, max_iter=20, min_eig=30.0),
    "converge-guess": dict(eps=0.01, max_iter=20, guess=True),
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
    kw = dict(MODES[mode], window=w, levels=L)
    if kw.get("guess"):
        kw["guess"] = guess_for(case)
    return kw


@functools.lru_cache(maxsize=None)
def reference(case, mode, order="numpy"):
    """tests/track_ref.py on a case: computed once, shared by every test that needs it, never written to."""
    shape, kind, T, N, w, L = case
    r = tr.track_pairs(scene(shape, T, kind), points(shape, N), order=order, **kwargs(case, mode))
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
