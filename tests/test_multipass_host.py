"""Multi-pass PIV, host side (CPU): the reference (tests/multipass_ref.py) against the oracle at zero offsets, the predictor reference on
hand-worked grids, ``multipass_spec`` and the keyword validation, the planner, the plugin's TypeError for another engine, the CPU
checks of the inputs tests/test_gpu_multipass.py relies on (tie shares, coarse vectors next to a half-integer), and the value of the
feature on the reference alone."""
import functools

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import frames, piv, shard, velocimetry, window
from pyorc_amd.synth import particle_stack
from tests import multipass_ref as ref
from tests import recipe_doubles as rd
from tests.test_search_area_host import fine_particles

# ---- inputs shared with tests/test_gpu_multipass.py ---------------------------------------------------------------------------------
# the shifted kernel: (n, (H, W), overlap, seed) on particle_stack(4, H, W, seed, density=0.04)
SHIFT_CASES = [(16, (70, 101), 8, 6), (16, (48, 53), 0, 3), (32, (96, 133), 16, 7), (32, (70, 101), 0, 8), (64, (130, 197), 32, 9),
               (64, (192, 200), 0, 10)]
# the chains, on the two stacks of the feature's value (T = 3)
CHAINS = [[(64, 32), (32, 16), (16, 8)], [(32, 16), (32, 16)]]
CHAIN_STACKS = ("particles", "fine")
TRUE_SHIFT = {"particles": (9.3, -6.4), "fine": (10.0, -9.0)}
# get_ffpiv / frames.get_piv: coarse_passes=[(64, 32)], final 16 @ 8, T = 9 on a 70 x 101 frame
FFPIV_PASSES = [(64, 32), (16, 8)]


def as_samples(a, dtype):
    """uint8 as drawn, float32 / float64 through the affine map x * 0.37 - 11 (the same normalised windows)."""
    return a if dtype == np.uint8 else a.astype(dtype) * dtype(0.37) - dtype(11.0)


def shift_stack(i, dtype=np.uint8):
    n, (H, W), ov, seed = SHIFT_CASES[i]
    return as_samples(particle_stack(4, H, W, seed=seed, density=0.04), dtype)


def shift_offsets(i):
    """default_rng(seed).integers(-12, 13) per (pair, window, component), clamped to the frame."""
    n, (H, W), ov, seed = SHIFT_CASES[i]
    rows, cols = po.get_axis_shape(H, n, ov), po.get_axis_shape(W, n, ov)
    raw = np.random.default_rng(seed).integers(-12, 13, size=(3, rows, cols, 2))
    return ref.clamp_shift(raw, (H, W), n, ov).astype(np.int16)


# offsets far outside the frame, the int16 extremes included: the kernel clamps them
WILD_CASES = (1, 2, 5)


def wild_offsets(i):
    n, (H, W), ov, seed = SHIFT_CASES[i]
    rows, cols = po.get_axis_shape(H, n, ov), po.get_axis_shape(W, n, ov)
    values = np.array([-32768, -32767, -300, -40, 40, 300, 32767], dtype=np.int16)
    return np.random.default_rng(seed + 100).choice(values, size=(3, rows, cols, 2))


# a signal threshold that takes out some windows and keeps others: samples below 40 set to zero, the upper left quarter of every frame
# empty, at least 30 % of a window non-zero
SIGNAL_CASES = (0, 3, 4)
SIGNAL_THRESHOLD = 0.3


def signal_stack(i):
    a = shift_stack(i).copy()
    a[a < 40] = 0
    a[:, :a.shape[1] // 2, :a.shape[2] // 2] = 0
    return a


@functools.lru_cache(maxsize=None)
def chain_stack(name):
    if name == "particles":
        return particle_stack(3, 160, 200, seed=5, density=0.06, uniform_shift=(9.3, -6.4))
    return fine_particles(3, 160, 160, 22, 0.2, sigma=0.8, shift=(10.0, -9.0))


@functools.lru_cache(maxsize=None)
def ffpiv_stack():
    return particle_stack(9, 70, 101, seed=7, density=0.04)


@functools.lru_cache(maxsize=None)
def long_stack():
    """More pairs than two anchor lengths of pass 0 (64 px on this grid: 25 pairs): 51 pairs, so that chunks fall at pairs 25 and 50."""
    return particle_stack(52, 70, 101, seed=7, density=0.04)


@functools.lru_cache(maxsize=None)
def chain_ref(name, c):
    return ref.multipass(chain_stack(name), CHAINS[c])


def near_half_dependents(u, v, dim, coarse, fine, eps=1e-3):
    """(P, rows_f, cols_f) bool: the fine windows whose offset depends on a valid coarse vector with a component within ``eps`` of a
    half-integer -- where a 1e-4 difference of a pass could turn the predictor's rint.  A fine window reads the medians of up to four
    coarse windows (those with a non-zero weight), a median the 3 x 3 neighbourhood of its window."""
    (nc, oc), (nf, of) = coarse, fine
    y0c, x0c = ref.grid_origins(dim, nc, oc)
    y0f, x0f = ref.grid_origins(dim, nf, of)
    u = np.asarray(u, dtype=np.float64).reshape(-1, len(y0c), len(x0c))
    v = np.asarray(v, dtype=np.float64).reshape(u.shape)
    with np.errstate(invalid="ignore"):
        risky = np.isfinite(u) & np.isfinite(v) & ((np.abs(np.abs(u - np.floor(u)) - 0.5) < eps) | (np.abs(np.abs(v - np.floor(v)) - 0.5) < eps))
    med = np.zeros_like(risky)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            src = risky[:, max(dr, 0):risky.shape[1] + min(dr, 0), max(dc, 0):risky.shape[2] + min(dc, 0)]
            med[:, max(-dr, 0):risky.shape[1] + min(-dr, 0), max(-dc, 0):risky.shape[2] + min(-dc, 0)] |= src
    iy0, iy1, wy0, wy1 = ref._axis(y0f + nf // 2, nc, nc - oc, len(y0c))
    ix0, ix1, wx0, wx1 = ref._axis(x0f + nf // 2, nc, nc - oc, len(x0c))
    out = np.zeros((u.shape[0], len(y0f), len(x0f)), dtype=bool)
    for iy, wy in ((iy0, wy0), (iy1, wy1)):
        for ix, wx in ((ix0, wx0), (ix1, wx1)):
            out |= med[:, iy[:, None], ix[None, :]] & ((wy[:, None] * wx[None, :]) != 0)[None]
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_reference_with_zero_offsets_is_the_oracle():
    a = particle_stack(3, 70, 90, seed=2, density=0.05)
    for n, ov in ((16, 8), (32, 16), (64, 32)):
        rows, cols = po.get_axis_shape(70, n, ov), po.get_axis_shape(90, n, ov)
        _, _, oracle = po.cross_corr(a, (n, n), (ov, ov), signal_threshold=0.05)
        uo, vo = po.u_v_displacement(oracle, rows, cols)
        for shift in (None, np.zeros((2, rows, cols, 2), np.int16)):
            r = ref.shifted_piv(a, n, ov, shift, signal_threshold=0.05)
            assert np.array_equal(r["planes"], oracle, equal_nan=True)
            assert np.array_equal(r["u"], uo, equal_nan=True) and np.array_equal(r["v"], vo, equal_nan=True)
        uu, vv, cm, sn = po.get_uv_timestep(a, cols, rows, (n, n), (ov, ov), signal_threshold=0.05)
        assert np.array_equal(r["corr"].astype(np.float32), cm, equal_nan=True) and np.array_equal(r["s2n"].astype(np.float32), sn, equal_nan=True)


def test_reference_shifted_window_is_the_window_at_the_offset():
    """A frame pair whose second frame is the first moved by (dy, dx) = (5, -3): with that offset every inner window correlates with
    itself (the peak at the centre, residual 0, u = dx, v = dy)."""
    rng = np.random.default_rng(0)
    big = rng.integers(0, 255, size=(120, 140)).astype(np.uint8)
    a = np.stack([big[20:100, 20:120], big[15:95, 23:123]])      # frame 1 [y, x] = frame 0 [y - 5, x + 3]
    sh = np.zeros((1, 4, 5, 2), np.int16)
    sh[..., 0], sh[..., 1] = 5, -3
    r = ref.shifted_piv(a, 32, 16, sh)
    inner = np.all(r["shift"] == sh, axis=-1)
    assert inner.sum() >= 6 and np.allclose(r["u"][inner], -3.0, atol=1e-9) and np.allclose(r["v"][inner], 5.0, atol=1e-9)
    same = ref.shifted_piv(a[:1].repeat(2, 0), 32, 16)               # every window against itself
    assert np.allclose(r["corr"][inner], same["corr"][inner]) and np.allclose(r["planes"].reshape(1, 4, 5, 32, 32)[inner], same["planes"].reshape(1, 4, 5, 32, 32)[inner])
    with po.semantics(v_sign=1):
        assert np.allclose(ref.shifted_piv(a, 32, 16, sh)["v"][inner], -5.0)


# ---- the predictor reference on hand-worked grids -------------------------------------------------------------------------------------
def test_predictor_one_by_one_coarse_grid_is_constant():
    # 64 x 64 frame, one 64 window; fine 16 @ 8: 7 x 7.  M2 = 2 * q everywhere, weights (s, 0): d = q, then the frame clamp
    d = ref.predict_shift([[[3.4]]], [[[-2.6]]], (64, 64), (64, 32), (16, 8))
    assert d.shape == (1, 7, 7, 2) and d.dtype == np.int16
    y0 = np.arange(7) * 8
    assert np.array_equal(d[0, :, :, 1], np.clip(3, -y0, 48 - y0)[None, :].repeat(7, 0))         # dx = rint(3.4) = 3, clamped on the right
    assert np.array_equal(d[0, :, :, 0], np.clip(-3, -y0, 48 - y0)[:, None].repeat(7, 1))        # dy = rint(-2.6) = -3, clamped at the top


def test_predictor_single_row_and_single_column():
    # one row of three coarse windows 32 @ 16 on a 32 x 64 frame: centres x = 16, 32, 48; medians over the row neighbours
    u = np.array([[[2.0, 4.0, 12.0]]])
    v = np.zeros_like(u)
    # M2 = [2 + 4, 2 * 4, 4 + 12] = [6, 8, 16]; fine 16 @ 0 on 32 x 64: centres x = 8, 24, 40, 56, y = 8, 24 (one coarse row: w1 = 0)
    # x = 8: left of the first centre -> 6 / 2 = 3; x = 24: halfway 16..32 -> (8 * 6 + 8 * 8) / 32 = 3.5 -> 4 (half up);
    # x = 40: halfway 32..48 -> (8 * 8 + 8 * 16) / 32 = 6; x = 56: right of the last centre -> 8, clamped to W - n - x0 = 0
    d = ref.predict_shift(u, v, (32, 64), (32, 16), (16, 0))
    assert d.shape == (1, 2, 4, 2) and np.array_equal(d[0, :, :, 1], [[3, 4, 6, 0]] * 2) and not d[..., 0].any()
    # the same numbers down a single column (u and v, rows and columns swapped)
    dT = ref.predict_shift(np.zeros((1, 3, 1)), u.reshape(1, 3, 1), (64, 32), (32, 16), (16, 0))
    assert np.array_equal(dT[0, :, :, 0], np.array([[3, 4, 6, 0]] * 2).T) and not dT[..., 1].any()


def test_predictor_all_nan_block_half_values_and_even_counts():
    nan = np.nan
    # a 3 x 3 coarse grid (32 @ 16 on 64 x 64), all NaN: no valid vector -> 0
    assert not ref.predict_shift(np.full((1, 3, 3), nan), np.zeros((1, 3, 3)), (64, 64), (32, 16), (32, 16)).any()
    # a vector is valid only when BOTH components are finite
    u = np.full((1, 3, 3), 5.0)
    v = np.full((1, 3, 3), nan)
    assert not ref.predict_shift(u, v, (64, 64), (32, 16), (32, 16)).any()
    # values at exactly +-k.5 round half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2, -2.5 -> -2; one window per frame
    for x, q in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (3.5, 4)):
        d = ref.predict_shift([[[x]]], [[[-x]]], (96, 96), (96, 0), (32, 0))[0, 1, 1]
        assert tuple(d) == (-q, q), (x, q, d)
    # an even valid count: the corner (0, 0) of a 3 x 3 grid sees 4 vectors, [1, 2, 4, 9] -> M2 = 2 + 4 = 6 -> d = 3; with one of
    # them NaN three remain, [1, 4, 9] -> 2 * 4 -> 4
    u = np.array([[[1.0, 2.0, 50.0], [4.0, 9.0, 50.0], [50.0, 50.0, 50.0]]])
    d = ref.predict_shift(u, np.zeros_like(u), (96, 96), (32, 0), (32, 0))
    assert d[0, 0, 0, 1] == 3
    u[0, 0, 1] = nan
    assert ref.predict_shift(u, np.zeros_like(u), (96, 96), (32, 0), (32, 0))[0, 0, 0, 1] == 4
    # two middle values of different parity: [1, 2] -> M2 = 3 -> 1.5 -> 2 (half up); [-2, -1] -> M2 = -3 -> -1.5 -> -1 (half up)
    # (one row of two windows on a 32 x 64 frame; the second window sits on the centre of coarse window 1: all weight there)
    assert ref.predict_shift([[[1.0, 2.0]]], [[[0.0, 0.0]]], (32, 64), (32, 0), (32, 0))[0, 0, 0].tolist() == [0, 2]
    assert ref.predict_shift([[[-2.0, -1.0]]], [[[0.0, 0.0]]], (32, 64), (32, 0), (32, 0))[0, 0, 1].tolist() == [0, -1]


def test_predictor_outside_the_outermost_centres_and_the_clamp_at_all_four_edges():
    # coarse 64 @ 0 on 130 x 197: 2 x 3 windows, centres y = 32, 96, x = 32, 96, 160; fine 16 @ 8: 15 x 23, centres 8 .. 120 / 8 .. 184
    u = np.full((1, 2, 3), 20.0)
    v = np.full((1, 2, 3), 20.0)
    d = ref.predict_shift(u, v, (130, 197), (64, 0), (16, 8)).astype(int)
    y0, x0 = np.arange(15) * 8, np.arange(23) * 8
    assert np.array_equal(d[0, :, :, 0], np.minimum(20, 130 - 16 - y0)[:, None].repeat(23, 1))     # bottom edge
    assert np.array_equal(d[0, :, :, 1], np.minimum(20, 197 - 16 - x0)[None, :].repeat(15, 0))     # right edge
    d = ref.predict_shift(-u, -v, (130, 197), (64, 0), (16, 8)).astype(int)
    assert np.array_equal(d[0, :, :, 0], np.maximum(-20, -y0)[:, None].repeat(23, 1))              # top edge
    assert np.array_equal(d[0, :, :, 1], np.maximum(-20, -x0)[None, :].repeat(15, 0))              # left edge
    # constant extrapolation: a gradient along x only between the centres 32 .. 160; left of 32 and right of 160 it is flat
    u = np.array([[[0.0, 8.0, 16.0]] * 2])
    d = ref.predict_shift(u, np.zeros_like(u), (130, 197), (64, 0), (16, 8))
    # medians along the row (both rows equal): M2 = [0 + 8, 2 * 8, 8 + 16] = [8, 16, 24] -> values 4, 8, 12 at x = 32, 96, 160
    x0 = np.arange(d.shape[2]) * 8
    cf = x0 + 8
    expect = np.floor(np.interp(cf, [32, 96, 160], [4.0, 8.0, 12.0]) + 0.5).astype(int)
    assert np.array_equal(d[0, 0, :, 1], np.minimum(expect, 197 - 16 - x0))
    assert d[0, 0, :3, 1].tolist() == [4, 4, 4] and d[0, 0, 19:21, 1].tolist() == [12, 12]      # flat outside 32 .. 160
    with pytest.raises(ValueError, match="32767"):
        ref.predict_shift(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), (64, 40000), (64, 0), (16, 8))
    # every finite float32 is valid and is clamped to the int16 range before the integer arithmetic: 1e10 and -3.3e38 (above 3e38, still
    # finite) act as 32767 and -32768; next to a 0 the even count gives M2 = 32767 -> 16383.5 -> 16384, then the frame clamp
    d = ref.predict_shift([[[1e10]]], [[[-3.3e38]]], (96, 96), (96, 0), (32, 0))
    assert d[0, 1, 1].tolist() == [-32, 32]
    # one row of 62 windows of 512 px on a 512 x 32000 frame, the first vector huge: left of the first centre all weight is on
    # M2[0] = 32767 + 0 (two valid neighbours): d = floor((32767 + 1) / 2) = 16384, inside the clamp [0, 31984]; and down one column
    row = np.zeros((1, 1, 62))
    row[0, 0, 0] = 1e10
    assert ref.predict_shift(row, np.zeros_like(row), (512, 32000), (512, 0), (16, 0))[0, 0, 0].tolist() == [0, 16384]
    assert ref.predict_shift(np.zeros((1, 62, 1)), row.reshape(1, 62, 1), (32000, 512), (512, 0), (16, 0))[0, 0, 0].tolist() == [16384, 0]
    assert not ref.predict_shift([[[np.inf]]], [[[0.0]]], (96, 96), (96, 0), (32, 0)).any()


# ---- validation -----------------------------------------------------------------------------------------------------------------------
def test_multipass_spec(lib):
    assert window.multipass_spec((16, 16), (8, 8), None) == (16, 16) and window.multipass_spec((16, 16), (8, 8), []) == (16, 16)
    assert not isinstance(window.multipass_spec((16, 16), (8, 8), []), window.MultiPassWindow)
    spec = window.multipass_spec((16, 16), (8, 8), [64, (32, 8)])
    assert isinstance(spec, window.MultiPassWindow) and tuple(spec) == (16, 16) and spec.passes == ((64, 32), (32, 8), (16, 8))
    assert spec.overlap == (8, 8) and window.multipass_spec(spec, (8, 8)) is spec
    assert window.multipass_spec((32, 32), (16, 16), [np.int64(64)]).passes == ((64, 32), (32, 16))
    assert window.multipass_spec((16, 16), (8, 8), [(20, 10)]).passes == ((20, 10), (16, 8))      # pass 0: any even square window
    assert window.multipass_spec((32, 32), (16, 16), [32]).passes == ((32, 16), (32, 16))          # non-increasing: equal is fine
    for ws, ov, cp, msg in (((16, 16), (8, 8), [64, 24], r"pass 1: window 24 is not supported.*\(16, 32, 64\)"),
                            ((24, 24), (12, 12), [64], r"pass 1: window 24 is not supported.*\(16, 32, 64\)"),
                            ((32, 32), (16, 16), [16], "pass 1: window 32 is larger than pass 0's 16"),
                            ((16, 16), (8, 8), [32, 64], "pass 1: window 64 is larger than pass 0's 32"),
                            ((16, 16), (8, 8), [63], "pass 0: window 63 must be even"),
                            ((16, 16), (8, 8), [(64, 64)], "pass 0: overlap 64 must satisfy"),
                            ((16, 16), (8, 8), [(64, -1)], "pass 0: overlap -1 must satisfy"),
                            ((16, 16), (8, 8), [2.5], "an entry is a window size n or a pair"),
                            ((16, 16), (8, 8), [(64, 32, 1)], "an entry is a window size n or a pair"),
                            ((16, 16), (8, 8), [(64.0, 32)], "whole numbers"),
                            ((16, 32), (8, 8), [64], "square window and overlap"),
                            ((16, 16), (8, 4), [64], "square window and overlap"),
                            ((16, 16), (8, 8), [64] * 8, "at most 8 passes")):
        with pytest.raises(ValueError, match=msg):
            window.multipass_spec(ws, ov, cp)
    with pytest.raises(NotImplementedError, match="search_area_size"):
        window.multipass_spec(window.search_spec((12, 12), (32, 32)), (16, 16), [64])
    assert [lib.lspiv_shift_supported(n, n) for n in (8, 16, 24, 32, 48, 64, 128)] == [0, 1, 0, 1, 0, 1, 0]
    assert lib.lspiv_shift_supported(16, 32) == 0 and lib.lspiv_abi_version() == 5


def test_keyword_validation():
    a = np.zeros((3, 96, 96), np.uint8)
    run = lambda **kw: velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), (16, 16), (8, 8), kw.pop("sa", (16, 16)), 1.0, 1.0, **kw)
    with pytest.raises(NotImplementedError, match="coarse_passes with ensemble_corr=True is not implemented"):
        run(coarse_passes=[64], ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="coarse_passes together with a search_area_size"):
        velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), (12, 12), (16, 16), (32, 32), 1.0, 1.0, coarse_passes=[64])
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        run(coarse_passes=[64, 48])
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        frames.get_piv(a, 24, coarse_passes=[64])

    class Comm:
        rank, world = 0, 1

    spec = window.multipass_spec((16, 16), (8, 8), [64])
    with pytest.raises(NotImplementedError, match="coarse_passes with pyorc_amd.shard is not implemented"):
        shard.sharded_piv(lambda f0, f1: a[f0:f1], 2, spec, (8, 8), Comm())
    with pytest.raises(NotImplementedError, match="coarse_passes with pyorc_amd.shard is not implemented"):
        shard.sharded_piv_dev(object(), 2, spec, (8, 8), Comm())
    with pytest.raises(ValueError, match="passes is empty"):
        piv.piv_multipass(a, [])


def test_other_engines_do_not_know_the_keyword(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((3, 96, 96), np.uint8))
        with pytest.raises(TypeError, match="coarse_passes is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", coarse_passes=[64])
    finally:
        plugin.uninstall()


def test_planner_alignment_and_grid_follow_the_chain(lib):
    dim = (160, 200)
    spec = window.multipass_spec((16, 16), (8, 8), [64, 32])
    assert window.get_array_shape(dim, spec, spec.overlap) == window.get_array_shape(dim, (16, 16), (8, 8)) == (19, 24)
    # the alignment is pass 0's, on pass 0's grid
    assert window.chunk_alignment(spec, dim, (8, 8)) == window.chunk_alignment((64, 64), dim, (32, 32))
    assert window.chunk_alignment(spec) == window.chunk_alignment((64, 64))
    spec20 = window.multipass_spec((16, 16), (8, 8), [(20, 10)])
    assert window.chunk_alignment(spec20, dim, (8, 8)) == window.chunk_alignment((20, 20), dim, (10, 10))
    # memory: the frames once + the largest pass's launch + two result blocks of the largest intermediate grid + one offset array
    T = 10
    need = window.required_memory(T, dim, (16, 16), (8, 8), coarse_passes=[64, 32])
    assert need == window.required_memory(T, dim, spec, (8, 8))
    fb = T * 160 * 200
    single = [window.required_memory(T, dim, (n, n), (o, o)) - fb for n, o in spec.passes]
    tiles = [(T - 1) * int(np.prod(window.get_array_shape(dim, (n, n), (o, o)))) for n, o in spec.passes]
    assert need == fb + max(single) + 2 * 16 * max(tiles[:2]) + 4 * max(tiles[1:])
    assert need > window.required_memory(T, dim, (16, 16), (8, 8)) >= fb + 16 * tiles[2]
    with_planes = window.required_memory(T, dim, spec, (8, 8), with_planes=True)
    assert with_planes - need == tiles[2] * 16 * 16 * 4      # the planes of the FINAL pass only
    assert window.required_memory(T, dim, (16, 16), (8, 8), coarse_passes=[]) == window.required_memory(T, dim, (16, 16), (8, 8))
    assert frames.resolve_window(16, None, None) == ((16, 16), (16, 16), (8, 8))


# ---- the inputs the GPU tests rely on ---------------------------------------------------------------------------------------------------
def test_shift_cases_have_rare_ties_and_offsets_inside_the_frame():
    for i, (n, (H, W), ov, seed) in enumerate(SHIFT_CASES):
        sh = shift_offsets(i)
        assert sh.min() >= -12 and sh.max() <= 12 and (sh != 0).mean() > 0.5
        r = ref.shifted_piv(shift_stack(i), n, ov, sh)
        assert np.array_equal(r["shift"], sh)                       # clamped already
        assert r["tie"].mean() <= 0.01, (i, float(r["tie"].mean()))
        assert np.isfinite(r["u"]).mean() > 0.5
    for i in WILD_CASES:
        n, (H, W), ov, seed = SHIFT_CASES[i]
        r = ref.shifted_piv(shift_stack(i), n, ov, wild_offsets(i))
        assert np.abs(r["shift"]).max() <= max(H, W) and r["tie"].mean() <= 0.01, (i, float(r["tie"].mean()))
    for i in SIGNAL_CASES:
        n, (H, W), ov, seed = SHIFT_CASES[i]
        r = ref.shifted_piv(signal_stack(i), n, ov, shift_offsets(i), signal_threshold=SIGNAL_THRESHOLD)
        skipped = float(np.isnan(r["corr"]).mean())
        print("case", i, "below the threshold:", skipped, "ties:", float(r["tie"].mean()))
        assert 0.05 < skipped < 0.95 and r["tie"].mean() <= 0.01, (i, skipped)


def test_chain_cases_have_rare_ties_and_few_vectors_next_to_a_half_integer():
    for name in CHAIN_STACKS:
        dim = chain_stack(name).shape[1:]
        for c, chain in enumerate(CHAINS):
            passes = chain_ref(name, c)
            for k, r in enumerate(passes):
                assert r["tie"].mean() <= 0.01, (name, c, k, float(r["tie"].mean()))
                if k + 1 < len(passes):
                    dep = near_half_dependents(r["u"], r["v"], dim, chain[k], chain[k + 1])
                    print(name, chain, "pass", k, "fine windows next to a half-integer:", float(dep.mean()))
                    assert dep.mean() <= 0.01, (name, c, k, float(dep.mean()))


def test_ffpiv_case_has_rare_ties_and_few_vectors_next_to_a_half_integer():
    a = ffpiv_stack()
    for sem in (dict(), dict(v_sign=1), dict(border_peak=1), dict(border_peak=2), dict(std_ddof=1)):
        with po.semantics(**sem):
            passes = ref.multipass(a, FFPIV_PASSES)
        assert all(r["tie"].mean() <= 0.01 for r in passes), sem
        dep = near_half_dependents(passes[0]["u"], passes[0]["v"], a.shape[1:], *FFPIV_PASSES)
        assert dep.mean() <= 0.01, (sem, float(dep.mean()))
        assert np.isfinite(passes[-1]["u"]).mean() > 0.5


# ---- the value of the feature, on the reference alone -----------------------------------------------------------------------------------
def within_half_px(r, true):
    with np.errstate(invalid="ignore"):
        good = (np.abs(r["u"] - true[0]) <= 0.5) & (np.abs(r["v"] - true[1]) <= 0.5)
    return float(good.mean()), float(np.nanmedian(np.hypot(r["u"] - true[0], r["v"] - true[1]))), float(np.isnan(r["u"]).mean())


def test_a_coarse_pass_recovers_a_displacement_the_final_window_loses():
    """Final window 16 @ 8, uniform displacement of ~10 px per frame (n / 4 = 4 px is where a plain 16 x 16 pass loses its pairs).
    Measured on the reference (share of windows within 0.5 px, median error, NaN share):
      particle_stack(3, 160, 200, seed=5, density=0.06, uniform_shift=(9.3, -6.4)): single pass 0 %, 14.0 px, 18.6 %;
          chain 64 @ 32 -> 16 @ 8: 94.63 %, 0.156 px, 0.33 %   (seeds 4 and 6: 94.63 % and 95.29 %)
      fine_particles(3, 160, 160, 22, 0.2, sigma=0.8, shift=(10, -9)): single pass 0 %, 14.5 px, 36.6 %;
          chain: 89.75 %, 0 px, 4.7 %   (seeds 21 and 23: 89.75 % both -- what is lost are the windows whose offset the frame clamps)
    asserted at the measured share less the spread over the neighbouring seeds (none downwards): 94.6 % and 89.7 %."""
    for name, least in (("particles", 0.946), ("fine", 0.897)):
        a, true = chain_stack(name), TRUE_SHIFT[name]
        single = within_half_px(ref.multipass(a, [(16, 8)])[-1], true)
        chain = within_half_px(ref.multipass(a, [(64, 32), (16, 8)])[-1], true)
        print(name, "single pass 16:", single, "| 64 @ 32 -> 16 @ 8:", chain)
        assert single[0] == 0.0
        assert chain[0] >= least and chain[1] < 0.2


# ---- the inputs of tests/test_gpu_rescue_modes.py -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ov", ref.RESCUE_GEOMETRIES, ids=[f"{n}@{ov}" for n, ov in ref.RESCUE_GEOMETRIES])
def test_rescue_inputs_have_no_ties_and_offsets_the_clamp_changes(n, ov):
    """Measured: tie share 0.0 at every geometry and sample type, 94.1 % of the windows finite at 16 @ 8 and all of them at the others;
    149 / 18 / 8 / 14 offsets changed by the clamp, the hand-made ones at pair 0's top row and pair 2's left column among them."""
    raw = ref.rescue_offsets(n, ov)
    for dtype in (np.uint8, np.float32, np.float64):
        r = ref.rescue_ref(n, ov, dtype)
        print(n, ov, dtype.__name__, "ties:", float(r["tie"].mean()), "finite:", float(np.isfinite(r["u"]).mean()))
        assert r["tie"].mean() <= 0.01 and np.isfinite(r["u"]).mean() >= 0.93
        assert np.array_equal(r["shift"], ref.clamp_shift(raw, ref.RESCUE_DIM, n, ov))
    changed = np.any(r["shift"] != raw, axis=-1)
    assert changed[0, 0, :].all() and changed[2, :, 0].all()             # the hand-made ones: all of them point out of the frame
    assert (r["shift"][0, 0, :, 0] == 0).all() and (r["shift"][2, :, 0, 1] == 0).all()
    assert not changed[1, 1:-1, 1:-1].any()                              # an interior window keeps its offset
