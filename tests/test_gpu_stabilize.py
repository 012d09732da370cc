"""GPU tests of frame stabilisation against the float64 reference tests/stabilize_ref.py: the warp bit for
bit, the fit to 1e-9 px at the frame corners, the chain bit for bit, every path (one call, chunks with halo and carry, DeviceFrames) to
the same bits, and the whole mode on the shaken scene that tests/test_stabilize_host.py qualified."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyorc_amd
from pyorc_amd import DeviceFrames, _lib, stabilize
from tests import stabilize_ref as sr

pytestmark = pytest.mark.gpu

SHAPE = (70, 150)      # two full 64-px blocks and a partial one, an odd height


def _rot(deg, scale, shape):
    H, W = shape
    cx, cy, th = (W - 1) / 2.0, (H - 1) / 2.0, np.deg2rad(deg)
    c, s = scale * np.cos(th), scale * np.sin(th)
    return [[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]]


WARP_A = np.array([
    [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],                      # identity
    [[1.0, 0.0, 5.0], [0.0, 1.0, -3.0]],                     # integer shift
    [[1.0, 0.0, 16.5 / 32], [0.0, 1.0, 16.5 / 32]],          # every coordinate a rounding tie of the 1/32 px grid
    _rot(0.7, 1.01, SHAPE),                                  # rotation with scale: row changes inside a wave
    [[1.0, 0.0, 130.0], [0.0, 1.0, 60.0]],                   # most of the frame outside: zeros
    [[1.0, 0.0, -20.3], [0.0, 1.0, -10.7]],                  # negative source coordinates
    [[1.0, 0.0, np.nan], [0.0, 1.0, 2.0]],                   # a NaN entry: the coordinate becomes 0
    [[np.inf, 0.0, 1.0], [0.0, -1e300, 0.0]],                # clipped to the int32 range, far outside
])


def _warp_frames(dtype, nonfinite=False):
    rng = np.random.default_rng(4)
    f = rng.integers(0, 256, size=(len(WARP_A),) + SHAPE)
    if dtype == np.uint8:
        return f.astype(np.uint8)
    f = (f + rng.random(f.shape)).astype(np.float32)
    if nonfinite:
        bad = rng.random(f.shape)
        f[bad < 0.02] = np.nan
        f[(bad >= 0.02) & (bad < 0.03)] = np.inf
        f[(bad >= 0.03) & (bad < 0.04)] = -np.inf
    return f


def _same_bits(got, want):
    """Equal bit for bit; a NaN must be a NaN (its payload is the hardware's own)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    return np.array_equal(got, want)


@pytest.mark.parametrize("case", ["uint8", "float32", "float32-nonfinite"])
def test_warp_is_the_references_bits(gpu, case):
    f = _warp_frames(np.uint8 if case == "uint8" else np.float32, nonfinite=case.endswith("nonfinite"))
    want = sr.warp(f, WARP_A)
    got = stabilize.warp(f, WARP_A)
    for t in range(len(WARP_A)):
        assert _same_bits(got[t], want[t]), f"transform {t}"
    assert np.array_equal(got[0].view(np.uint8), f[0].view(np.uint8)) or case.endswith("nonfinite")
    assert (got[4] == 0).mean() > 0.7      # the case is what it says
    # a DeviceFrames stack: the same kernel on the stack in HBM, into a caller's buffer
    d_out = DeviceFrames.empty(f.shape, f.dtype)
    res = stabilize.warp(DeviceFrames.from_host(f), WARP_A, out=d_out)
    assert res is d_out and _same_bits(d_out.to_host(), got)


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------
FIT_GRIDS = {(5, 7): (96, 128), (40, 60): (656, 976)}
FIT_P = np.array([[[1.0015, -0.0030, 1.75], [0.0030, 1.0015, -2.5]],
                  [[0.9990, 0.0020, -3.25], [-0.0020, 0.9990, 0.5]],
                  [[1.0030, -0.0020, 1.25], [0.0040, 0.9980, 0.75]]])


@functools.lru_cache(maxsize=None)
def _fit_vectors(grid):
    """(u, v) (3, rows, cols) float32: a model each, 0.05 px noise, 15 % gross outliers, 5 % NaN."""
    H, W = FIT_GRIDS[grid]
    xc, yc = sr.centres(32, 16, (H, W))
    X, Y = np.meshgrid(xc, yc)
    rng = np.random.default_rng(grid[0])
    u = np.stack([(P[0, 0] - 1.0) * X + P[0, 1] * Y + P[0, 2] for P in FIT_P]) + rng.normal(size=(3,) + grid) * 0.05
    v = np.stack([P[1, 0] * X + (P[1, 1] - 1.0) * Y + P[1, 2] for P in FIT_P]) + rng.normal(size=(3,) + grid) * 0.05
    sel = rng.random(u.shape)
    ang, mag = rng.uniform(0, 2 * np.pi, u.shape), rng.uniform(3.0, 8.0, u.shape)
    u = np.where(sel < 0.15, u + mag * np.cos(ang), u)
    v = np.where(sel < 0.15, v + mag * np.sin(ang), v)
    u = np.where((sel >= 0.15) & (sel < 0.18), np.nan, u)
    v = np.where((sel >= 0.18) & (sel < 0.20), np.nan, v)
    return np.ascontiguousarray(u, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)


def _fit_host(lib, u, v, shape, model, reject=sr.REJECT, min_vectors=sr.MIN_VECTORS, n=32, o=16):
    pairs, rows, cols = u.shape
    P = np.full((pairs, 2, 3), np.nan)
    n_used = np.full(pairs, -1, dtype=np.int32)
    _lib.check(lib.lspiv_stabilize_fit(_lib.ptr(u), _lib.ptr(v), pairs, rows, cols, n, o, o, shape[0], shape[1], stabilize.MODELS[model],
                                       float(reject[0]), float(reject[1]), int(min_vectors), _lib.ptr(P), _lib.ptr(n_used)))
    return P, n_used


@pytest.mark.parametrize("grid", list(FIT_GRIDS))
@pytest.mark.parametrize("model", sr.MODELS)
def test_fit_matches_the_reference(gpu, grid, model):
    shape = FIT_GRIDS[grid]
    u, v = _fit_vectors(grid)
    for t in range(len(u)):      # the inputs keep clear of the thresholds: the selections cannot differ by rounding
        P, k, res = sr.fit(u[t], v[t], 32, 16, shape, model, details=True)
        assert k >= 6 and all(np.abs(r - lim).min() > 1e-6 for r, lim in zip(res, sr.REJECT))
    want_P, want_n = sr.fit_pairs(u, v, 32, 16, shape, model)
    got_P, got_n = _fit_host(gpu, u, v, shape, model)
    assert np.array_equal(got_n, want_n)
    err = sr.corner_error(got_P, want_P, shape)
    print(f"grid {grid} {model}: n_used {got_n.tolist()}, corner difference {err.max():.2e} px")
    assert err.max() <= 1e-9
    if model == "similarity":     # ... and the fit finds what was put in
        assert sr.corner_error(got_P[0], FIT_P[0], shape) < (0.2 if grid == (5, 7) else 0.02)


@pytest.mark.parametrize("model", sr.MODELS)
def test_degenerate_fits_are_the_identity(gpu, model):
    u, v = (q.copy() for q in _fit_vectors((5, 7)))
    keep = [3, 9, 17, 22, 30]
    few = np.full(u.shape, np.nan, dtype=np.float32)
    few.reshape(3, -1)[1, keep] = u.reshape(3, -1)[1, keep]       # pair 1: 5 finite vectors < min_vectors = 6; pairs 0 and 2: none
    P, n_used = _fit_host(gpu, few, v, FIT_GRIDS[(5, 7)], model)
    assert np.array_equal(n_used, [0, 0, 0]) and np.array_equal(P, np.broadcast_to(sr.IDENTITY, (3, 2, 3)))
    # one row of windows: "affine" is not determined, the others are -- as the reference says
    shape = (40, 128)
    u1, v1 = np.ascontiguousarray(u[:, 2:3]), np.ascontiguousarray(v[:, 2:3])
    want_P, want_n = sr.fit_pairs(u1, v1, 32, 16, shape, model, reject=(50.0, 25.0), min_vectors=3)
    P, n_used = _fit_host(gpu, u1, v1, shape, model, reject=(50.0, 25.0), min_vectors=3)
    assert np.array_equal(n_used, want_n) and (want_n == 0).all() == (model == "affine")
    assert sr.corner_error(P, want_P, shape).max() <= 1e-9


# ---- chain -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [0, 1, 64, 150])
@pytest.mark.parametrize("with_carry", [False, True])
def test_chain_is_the_references_bits(gpu, pairs, with_carry):
    rng = np.random.default_rng(pairs)
    P = np.ascontiguousarray(sr.IDENTITY + rng.normal(size=(pairs, 2, 3)) * [[2e-3, 2e-3, 2.0]])
    carry = np.ascontiguousarray(sr.IDENTITY + rng.normal(size=(2, 3)) * [[1e-2, 1e-2, 9.0]]) if with_carry else None
    want_A, want_c = sr.chain(P, carry)
    A, c = np.full((pairs + 1, 2, 3), np.nan), np.full((2, 3), np.nan)
    _lib.check(gpu.lspiv_stabilize_chain(_lib.ptr(P), pairs, None if carry is None else _lib.ptr(carry), _lib.ptr(A), _lib.ptr(c)))
    assert np.array_equal(A.view(np.uint64), want_A.view(np.uint64)) and np.array_equal(c.view(np.uint64), want_c.view(np.uint64))


# ---- the whole mode on the shaken scene ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_run():
    f = sr.scene(*sr.GPU_SCENE)["frames"]
    n, o = sr.SCENE_WINDOW
    out, tr = stabilize.stabilize(f, sr.stable_mask(), window_size=n, overlap=o)
    return f, out, tr


def test_paths_give_the_same_bits(gpu):
    f, whole, tr = _scene_run()
    n, o = sr.SCENE_WINDOW
    kw = dict(window_size=n, overlap=o)
    for cut in (4, 3):       # 4 + 4 frames, and an odd start: a one-frame halo, carry = the pose at the chunk's first frame
        a = stabilize.estimate(f[:cut + 1], sr.stable_mask(), **kw)
        b = stabilize.estimate(f[cut:], sr.stable_mask(), carry=a.carry, **kw)
        assert np.array_equal(np.concatenate([a.A, b.A[1:]]), tr.A) and np.array_equal(b.carry, tr.carry)
        assert np.array_equal(a.A[cut], a.carry)
        assert np.array_equal(np.concatenate([a.pairwise, b.pairwise]), tr.pairwise)
        assert np.array_equal(np.concatenate([a.n_used, b.n_used]), tr.n_used)
        frames = np.concatenate([stabilize.warp(f[:cut], a.A[:cut]), stabilize.warp(f[cut:], b.A)])
        assert np.array_equal(frames, whole)
    d_out, d_tr = stabilize.stabilize(DeviceFrames.from_host(f), sr.stable_mask(), **kw)
    assert isinstance(d_out, DeviceFrames) and np.array_equal(d_out.to_host(), whole)
    for got, want in zip(d_tr, tr):
        assert np.array_equal(got, want)
    # the frames are the reference warp of the transforms that came out: the warp adds nothing of its own
    assert np.array_equal(whole, sr.warp(f, tr.A))


def test_end_to_end_on_the_qualified_scene(gpu):
    f, out, tr = _scene_run()
    ref = sr.scene_ref(*sr.GPU_SCENE)
    assert tr.A.shape == (len(f), 2, 3) and tr.pairwise.shape == (len(f) - 1, 2, 3) and tr.A.dtype == np.float64
    assert np.array_equal(tr.n_used, ref["n_used"]) and tr.n_used.min() >= 30
    move = float(sr.corner_error(tr.A, ref["A"], sr.SCENE_DIM).max())
    print(f"corner positions differ from the reference's by <= {move:.3e} px (allowed {4 * sr.GATE_CORNER_MOVE:.1e})")
    assert move <= 4 * sr.GATE_CORNER_MOVE
    assert np.array_equal(tr.A[0], sr.IDENTITY) and np.array_equal(tr.carry, tr.A[-1])
    # plain PIV of the stabilised stack finds the tracers' truth where the raw stack does not
    n, o = sr.SCENE_WINDOW
    want_share, _, n_water = sr.water_score(sr.plain_piv(ref["frames"]))
    sign = -1.0 if _lib.get_option("v_sign") else 1.0
    u, v = pyorc_amd.piv_pairs(out, (n, n), (o, o))[:2]
    share, median, _ = sr.water_score((u, sign * v))
    u, v = pyorc_amd.piv_pairs(f, (n, n), (o, o))[:2]
    raw_share, raw_median, _ = sr.water_score((u, sign * v))
    print(f"water windows within 0.5 px: raw {raw_share:.3f} (median {raw_median:.3f} px), stabilised {share:.3f} (median {median:.3f} px), "
          f"reference {want_share:.3f}, {n_water} windows")
    assert share >= want_share - 1.0 / n_water - 1e-12
    assert share > raw_share and median < raw_median


def test_estimate_warns_once_about_identity_pairs(gpu):
    f = sr.scene(*sr.GPU_SCENE)["frames"][:4]
    n, o = sr.SCENE_WINDOW
    with pytest.warns(RuntimeWarning, match="identity") as rec:
        tr = stabilize.estimate(f, sr.stable_mask(), window_size=n, overlap=o, min_vectors=1000)
    assert len(rec) == 1 and (tr.n_used == 0).all() and np.array_equal(tr.A, np.broadcast_to(sr.IDENTITY, (4, 2, 3)))
