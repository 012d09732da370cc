"""The un-packing through DPP of the per-pair 32 x 32 walking kernels (csrc/piv_fft_impl.h, UDPP; option "unpack_dpp" = 1) against the
exchange through LDS ("unpack_dpp" = 0): the same expressions on the same operands, only the lane a column sits in between the two
transposes differs -- hence the same BITS in u, v, corr, s2n and the planes, NaN masks and payloads included, and the same rescue
records.  No tolerance there.

The same cases also run against the kernels that compute every pair on its own ("walk" = 0) under the gate the parity tests use for
that comparison (test_gpu_parity.assert_same_to_rounding): the walking kernels leave out plane a of a wave's first iteration, which
belongs to no pair, and every pair must still come out.

Shapes: 64 x 96 frames, 32 x 32 windows at 50 % overlap = 15 windows (an odd count: a wave holds an invalid job, and the two lane
groups of a wave sit in different segments); 3, 25, 26 and 76 pairs (one short segment; exactly the anchor of 25; one pair more; three
segments and one pair), each at pair offsets 0 and 7 (offset 7 shortens the first segment)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
from test_gpu_parity import assert_same_to_rounding

from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames
from pyorc_amd.synth import particle_stack

pytestmark = pytest.mark.gpu
H, W, WS, OV = 64, 96, (32, 32), (16, 16)
PAIRS = (3, 25, 26, 76)
OFFSETS = (0, 7)
T_MAX = max(PAIRS) + 1


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
    a = particle_stack(T_MAX, H, W, seed=5)
    if kind == "u8":
        return a
    if kind == "f32-nan":
        f = a.astype(np.float32)
        f[2, 40, 50] = np.nan   # frame 2 is in every stack: pairs 1 and 2, the four windows over the sample
        return f
    if kind == "f32-dead":
        f = a.astype(np.float32)
        f[:, :32, :32] = 17.0   # window (0, 0) is constant over time: zero variance
        return f
    return a.astype(np.float32 if kind == "f32" else np.float64) * 0.5 - 3.0


@functools.lru_cache(maxsize=None)
def dev_stack(kind, pairs):
    a = np.ascontiguousarray(host_stack(kind)[:pairs + 1])
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
        assert np.array_equal(g, w, equal_nan=True), (what, k)
        assert g.tobytes() == w.tobytes(), (what, k, "raw bytes")


def test_option_is_listed(gpu):
    default = _lib.get_option("unpack_dpp")
    assert default in (0, 1)
    with options(unpack_dpp=1 - default):
        assert _lib.get_option("unpack_dpp") == 1 - default
    assert _lib.get_option("unpack_dpp") == default
    with pytest.raises(_lib.LspivError):
        _lib.set_option("unpack_dpp", 2)


# (stack, signal threshold, planes, further options)
CONTENT = {f"{kind}{'-nz' if thr is not None else ''}{'-planes' if planes else ''}": (kind, thr, planes, {})
           for kind in ("u8", "f32", "f64") for thr in (None, 0.02) for planes in (False, True)}
CONTENT["f32-nan"] = ("f32-nan", None, False, {})
CONTENT["f32-dead"] = ("f32-dead", None, False, {})
CONTENT["u8-flagged"] = ("u8", None, False, {"rescue_kappa": 200000, "rescue_tau": 1000000})   # an allowance that flags windows: non-empty lists


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("content", list(CONTENT))
def test_dpp_unpack_has_the_bits_of_the_lds_unpack(gpu, content, pairs, offset):
    kind, thr, planes, opts = CONTENT[content]
    d = dev_stack(kind, pairs)

    def call():
        return list(piv.piv_pairs(d, WS, OV, signal_threshold=thr, return_planes=planes, pair_offset=offset))

    with options(**opts):
        for defer in (1, 0):
            for rescue in (0, 1):
                with options(rescue=rescue, defer_fit=defer, unpack_dpp=0):
                    want = call()
                    lists_want = rescue_lists() if rescue else None
                with options(rescue=rescue, defer_fit=defer, unpack_dpp=1):
                    got = call()
                    lists_got = rescue_lists() if rescue else None
                same_bytes(got, want, (content, pairs, offset, "defer_fit", defer, "rescue", rescue))
                if rescue:
                    assert np.array_equal(lists_got[0], lists_want[0]), "fit records"
                    assert np.array_equal(lists_got[1], lists_want[1]), "amb records"
                    if content == "u8-flagged":
                        assert lists_got[0].shape[0] + lists_got[1].shape[0] >= 1, "no rescue record: the lists compare nothing"
        # every pair on its own: no first iteration to leave anything out of
        with options(walk=0):
            ref = call()
        assert_same_to_rounding(got[:4], ref[:4])
    u, corr = got[0], got[2]
    assert u.shape == (pairs, 3, 5)
    if kind == "f32-nan":
        assert np.isnan(corr[1:3, 1:3, 2:4]).all() and np.isfinite(corr[0]).all()
    elif kind == "f32-dead":
        assert np.all(corr[:, 0, 0] == 0.0) and np.all(np.isnan(u[:, 0, 0])) and np.isfinite(u[:, 1:, 1:]).any()
    else:
        assert np.isfinite(u).any()
