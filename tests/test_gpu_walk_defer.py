"""The batched sub-pixel fit of the 32 x 32 walking kernels (csrc/piv_fft_impl.h, DEFER; option "defer_fit" = 1, the default) against the
fit inside every iteration ("defer_fit" = 0): the same expressions on the same operands, issued once per 16 iterations with one plane per
lane instead of 32 times -- hence the same BITS in u, v, corr, s2n (and the planes), NaN masks and payloads included, and the same rescue
records.  No tolerance anywhere.

Shapes: 80 frames (79 pairs) of 64 x 96 with 32 x 32 windows at 50 % overlap = 15 windows: an odd count, so a wave holds an invalid job
and the two lane groups of a wave sit in different segments.  The anchor length is forced through the "walk" option (a grid this small
takes 25 pairs = 13 iterations and would never reach a flush inside the loop):

    3   2 iterations                         31  exactly 16: the flush inside the loop coincides with the end
    25  the default anchor                   32  even: a half iteration
    33  17 iterations                        75  flushes at 16, 32 and a tail of 6

each at pair offsets 0 and 7 (lspiv_piv_pairs_dev_at): offset 7 shortens the first segment, so the groups of a wave leave the loop at
different iterations.  Every case runs with the rescue pass off and on; with it on, the lists the kernel left behind
(lspiv_debug_rescue_lists) are compared as sets -- their order is whatever the waves made it."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from pyorc_amd import _lib, piv, window
from pyorc_amd.device import DeviceFrames
from pyorc_amd.synth import particle_stack

pytestmark = pytest.mark.gpu
T, H, W, WS, OV = 80, 64, 96, (32, 32), (16, 16)
ANCHORS = (3, 25, 31, 32, 33, 75)
OFFSETS = (0, 7)


@contextlib.contextmanager
def options(**kw):
    old = {k: _lib.get_option(k) for k in kw if k != "walk"}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
        if "walk" in kw:
            _lib.set_option("walk", -1)   # back to the environment


@functools.lru_cache(maxsize=None)
def host_stack(kind):
    if kind == "border":   # a displacement of half the window: the circular peak sits on the plane border
        return particle_stack(T, H, W, seed=11, uniform_shift=(16.0, 0.0))
    a = particle_stack(T, H, W, seed=5)
    a[:, :32, :32] = 17   # window (0, 0) is constant over time: zero variance, "dead"
    if kind in ("tie2", "tie4"):
        # under windows (2, 0) and (2, 1) every frame carries its own random tile, repeated every 16 px along x (tie2) or along x and y
        # (tie4): a 32 px window holds whole periods, so its circular correlation has 2 resp. 4 equal maxima up to rounding -- the "amb" cold
        # path inside the iteration, with exactly two candidates (a "fit" record that names the other one) resp. more (an "amb" record).
        # Two windows only: a stack of nothing but ties overflows the "amb" list, and WHICH records are dropped then is up to the waves.
        rng = np.random.default_rng(3)
        tile = rng.integers(0, 256, (T, 32 if kind == "tie2" else 16, 16), dtype=np.uint8)
        a[:, 32:, :48] = np.tile(tile, (1, 1 if kind == "tie2" else 2, 3))
        return a
    if kind == "u8":
        return a
    f = a.astype(np.float32 if kind == "f32" else np.float64)
    f[20, 40, 50] = np.nan   # two frames with a non-finite sample in some windows: "skip"
    f[41, 10, 70] = np.inf
    return f


@functools.lru_cache(maxsize=None)
def dev_stack(kind):
    a = host_stack(kind)
    d = DeviceFrames.empty(a.shape, a.dtype)   # float64 stays float64 in HBM: the <double> kernels
    _lib.check(_lib.load().lspiv_memcpy_h2d(d.c_ptr, _lib.ptr(a), a.nbytes))
    return d


def rescue_lists():
    """The two lists of the last launch as sorted arrays: (n_fit, 4) records and (n_amb,) result indices."""
    counts = np.zeros(2, np.int64)
    pc = counts.ctypes.data_as(C.POINTER(C.c_int64))
    _lib.check(_lib.load().lspiv_debug_rescue_lists(None, None, 0, None, 0, pc))
    fit, amb = np.zeros((int(counts[0]), 4), np.uint32), np.zeros(int(counts[1]), np.uint32)
    _lib.check(_lib.load().lspiv_debug_rescue_lists(None, fit.ctypes.data, fit.shape[0], amb.ctypes.data, amb.shape[0], pc))
    assert counts[0] == fit.shape[0] and counts[1] == amb.shape[0]
    fit = fit[np.lexsort(fit.T[::-1])] if fit.size else fit
    return fit, np.sort(amb)


def same_bytes(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, "NaN mask")
        assert np.array_equal(g, w, equal_nan=True), (what, k)
        assert g.tobytes() == w.tobytes(), (what, k, "raw bytes")


def both_forms(call, what):
    """``call`` under "defer_fit" 0 and 1, rescue off and on.  Returns the rescue-on results of the batched form and its list sizes."""
    out = None
    for rescue in (0, 1):
        with options(rescue=rescue, defer_fit=0):
            want = list(call())
            lists_want = rescue_lists() if rescue else None
        with options(rescue=rescue, defer_fit=1):
            got = list(call())
            lists_got = rescue_lists() if rescue else None
        same_bytes(got, want, (what, "rescue", rescue))
        if rescue:
            print(what, "| fit", lists_want[0].shape[0], "amb", lists_want[1].shape[0])
            assert np.array_equal(lists_got[0], lists_want[0]), (what, "fit records")
            assert np.array_equal(lists_got[1], lists_want[1]), (what, "amb records")
            out = got, (lists_got[0].shape[0], lists_got[1].shape[0])
    return out


def test_option_is_listed_and_defaults_to_the_batched_fit(gpu):
    assert _lib.get_option("defer_fit") == 1
    with options(defer_fit=0):
        assert _lib.get_option("defer_fit") == 0
    assert _lib.get_option("defer_fit") == 1
    with pytest.raises(_lib.LspivError):
        _lib.set_option("defer_fit", 2)


# content and mode of a case: (stack, signal threshold, planes, further options)
CONTENT = {
    "u8": ("u8", None, False, {}),
    "u8-flagged": ("u8", None, False, {"rescue_kappa": 200000, "rescue_tau": 1000000}),   # an allowance that flags windows: non-empty lists
    "u8-nz": ("u8", 0.0, False, {}),
    "u8-planes": ("u8", None, True, {}),
    "u8-nz-planes": ("u8", 0.02, True, {}),
    "f32-nan-inf": ("f32", None, False, {}),
    "f32-nz-planes": ("f32", 0.0, True, {}),
    "f64": ("f64", None, False, {}),
    "f64-planes": ("f64", None, True, {}),
    "tie2": ("tie2", None, False, {}),
    "tie4": ("tie4", None, False, {}),
    "border-nan": ("border", None, False, {"border_peak": 0}),
    "border-centre": ("border", None, False, {"border_peak": 1}),
    "border-integer": ("border", None, False, {"border_peak": 2}),
}


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("walk", ANCHORS)
@pytest.mark.parametrize("content", list(CONTENT))
def test_batched_fit_has_the_bits_of_the_fit_per_iteration(gpu, content, walk, offset):
    kind, thr, planes, opts = CONTENT[content]
    d = dev_stack(kind)
    with options(walk=walk, **opts):
        (got, (n_fit, n_amb)) = both_forms(lambda: piv.piv_pairs(d, WS, OV, signal_threshold=thr, return_planes=planes, pair_offset=offset),
                                           f"{content} walk {walk} offset {offset}")
    u, v, corr, s2n = got[:4]
    assert u.shape == (T - 1, 3, 5)
    if content == "u8-flagged":
        assert n_fit + n_amb >= 1, "no rescue record: the lists compare nothing"
    if kind == "tie4":
        assert n_amb >= 1, "no ambiguous window: the cold path inside the iteration is not compared"
    if kind == "tie2":
        assert n_fit + n_amb >= 1, "no ambiguous window: the cold path inside the iteration is not compared"
    if kind in ("u8", "f32", "f64"):
        assert np.all(corr[:, 0, 0] == 0.0) and np.all(np.isnan(u[:, 0, 0])), "the constant window is dead: corr 0, u NaN"
        assert np.isfinite(u[:, 1:, 1:]).any()
    if kind in ("f32", "f64"):   # pairs 19, 20 (frame 20) and 40, 41 (frame 41): the windows over the sample are skipped, corr NaN
        assert np.isnan(corr[[19, 20]][:, 1, 2]).all() and np.isnan(corr[[40, 41]][:, 0, 3]).all()
    if kind == "border":
        mode = opts["border_peak"]
        on_border = {0: np.isnan(u), 1: u == 0.0, 2: np.abs(u) == 16.0}[mode]
        assert on_border.mean() > 0.5, "the peaks were meant to sit on the plane border"


def test_one_launch_equals_two_launches_cut_on_the_alignment(gpu):
    """The defaults (anchor 25, batched fit): one launch over the stack against two launches cut on lspiv_chunk_alignment_grid, and both
    against the fit per iteration."""
    a = host_stack("u8")
    A = window.chunk_alignment(WS, (H, W), OV)
    cut = 2 * A
    assert 0 < cut < T - 1
    d, d0, d1 = dev_stack("u8"), DeviceFrames.from_host(a[:cut + 1]), DeviceFrames.from_host(a[cut:])

    def two():
        r0 = piv.piv_pairs(d0, WS, OV, pair_offset=0)
        r1 = piv.piv_pairs(d1, WS, OV, pair_offset=cut)
        return [np.concatenate([x, y]) for x, y in zip(r0, r1)]

    with options(defer_fit=1):
        whole, cutted = list(piv.piv_pairs(d, WS, OV)), two()
    with options(defer_fit=0):
        former = list(piv.piv_pairs(d, WS, OV))
    same_bytes(cutted, whole, "two launches against one")
    same_bytes(whole, former, "batched against per iteration")
