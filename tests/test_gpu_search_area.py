"""Extended search area on the GPU ("Extended search area") against tests/search_area_ref.py, the float64 reference.
Gate, the project's own: NaN masks identical, u, v, corr, s2n within 1e-4 (of max(|ref|, 0.05)), planes within 2e-6.  Only windows
whose reference plane has an exact float64 tie for its maximum (the clip at 1 binding on two samples included) are set aside, at
most 1 % of a case's windows; seeds and densities are checked for that on the CPU (tests/test_search_area_host.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from pyorc_amd.synth import particle_stack
from tests import search_area_ref as ref
from tests.test_search_area_host import CASES, case_stack, fast_flow_shares, fast_stack

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel_err(got, ref_, floor=0.05):
    with np.errstate(all="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - ref_) / np.maximum(np.abs(ref_), floor)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


def gate(got, r, planes=None, cap=0.01):
    u, v, cm, sn = got
    ok = ~r["tie"]
    print("set aside:", int(r["tie"].sum()), "of", ok.size, "| u", rel_err(u[ok], r["u"][ok]), "v", rel_err(v[ok], r["v"][ok]),
          "corr", rel_err(cm, r["corr"]), "s2n", rel_err(sn, r["s2n"]))
    assert r["tie"].mean() <= cap
    assert u.dtype == v.dtype == cm.dtype == sn.dtype == np.float32 and u.shape == r["u"].shape
    for name, g, x in (("u", u, r["u"]), ("v", v, r["v"])):
        assert np.array_equal(np.isnan(g)[ok], np.isnan(x)[ok]), f"{name}: NaN mask differs"
        assert rel_err(g[ok], x[ok]) <= TOL, name
    for name, g, x in (("corr", cm, r["corr"]), ("s2n", sn, r["s2n"])):
        assert np.array_equal(np.isnan(g), np.isnan(x)), f"{name}: NaN mask differs"
        assert rel_err(g, x) <= TOL, name
    if planes is not None:
        assert np.array_equal(np.isnan(planes), np.isnan(r["planes"]))
        print("planes", float(np.nanmax(np.abs(planes - r["planes"]), initial=0.0)))
        assert np.nanmax(np.abs(planes - r["planes"]), initial=0.0) < 2e-6


@functools.lru_cache(maxsize=None)
def case_ref(i):   # one reference per case, shared by the three sample types (an affine map of the samples normalises to the same windows)
    n, S, H, W, ov, seed, density = CASES[i]
    return ref.search_piv(case_stack(*CASES[i]).astype(np.float64), (n, n), (S, S), (ov, ov))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c[0]}in{c[1]}" for c in CASES])
def test_parity_host_and_device_entry(gpu, i, dtype):
    n, S, H, W, ov, seed, density = CASES[i]
    a = case_stack(*CASES[i], dtype=dtype)
    r = case_ref(i) if dtype == np.uint8 else ref.search_piv(a.astype(np.float64), (n, n), (S, S), (ov, ov))
    *host, planes = piv.piv_pairs(a, (n, n), (ov, ov), search_area_size=(S, S), return_planes=True)
    gate(host, r, planes)
    d = DeviceFrames.from_host(a)
    *dev, dplanes = piv.piv_pairs(d, (n, n), (ov, ov), search_area_size=(S, S), return_planes=True)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        for g, h in zip(dev + [dplanes], host + [planes]):
            assert np.array_equal(g, h, equal_nan=True), "host and device entry points differ"
    else:
        gate(dev, r, dplanes)
    x, y, cc = piv.cross_corr(a, (n, n), (ov, ov), search_area_size=(S, S)) if dtype == np.uint8 else (r["x"], r["y"], planes)
    assert np.array_equal(x, r["x"]) and np.array_equal(y, r["y"]) and np.array_equal(cc, planes, equal_nan=True)


def test_chunking_and_devices_are_bit_identical(gpu):
    a = particle_stack(9, 70, 101, seed=7, density=0.04)   # seed 7: no tie in the reference's 120 planes (seed 6 has 3: over the cap)
    x, y = window.get_rect_coordinates(a.shape[1:], (16, 16), (16, 16), search_area_size=(32, 32))
    run = lambda **kw: velocimetry.get_ffpiv(a, y, x, np.full(8, 0.5), (16, 16), (16, 16), (32, 32), 0.02, 0.02, **kw)
    whole = run()
    r = ref.search_piv(a, (16, 16), (32, 32), (16, 16))
    # back to pixels (dt / res = 25; the float32 storage of m/s and of this product add 6e-8 relative each, far inside the gate)
    gate((np.asarray(whole["v_x"]) * 25.0, np.asarray(whole["v_y"]) * 25.0, np.asarray(whole["corr"]), np.asarray(whole["s2n"])), r)
    for kw in (dict(chunksize=2), dict(chunksize=3), dict(devices=[0, 0]), dict(chunksize=3, devices=[0, 0])):
        got = run(**kw)
        for k in ("v_x", "v_y", "corr", "s2n"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (kw, k)
    d = velocimetry.get_ffpiv(DeviceFrames.from_host(a), y, x, np.full(8, 0.5), (16, 16), (16, 16), (32, 32), 0.02, 0.02, chunksize=4)
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(np.asarray(d[k]), np.asarray(whole[k]), equal_nan=True), k


OPT_STACK = dict(T=3, H=70, W=101, seed=6, density=0.04)


@pytest.mark.parametrize("opt,val", [("border_peak", 1), ("border_peak", 2), ("v_sign", 1), ("std_ddof", 1), ("signal_mode", 1),
                                     ("signal_positive", 1)])
def test_options_follow_the_reference(gpu, opt, val):
    a = particle_stack(**OPT_STACK)
    a[:, :40, :50] = 0          # border peaks (empty planes) and windows below the threshold
    thr = 0.05 if opt.startswith("signal") else None
    _lib.set_option(opt, val)
    try:
        with po.semantics(**{opt: val}):
            r = ref.search_piv(a, (16, 16), (32, 32), (16, 16), thr)
        gate(piv.piv_pairs(a, (16, 16), (16, 16), thr, search_area_size=(32, 32)), r)
    finally:
        _lib.set_option(opt, 0)
    with pytest.raises(ValueError, match="norm_clip"):
        _lib.set_option("norm_clip", 0)
        try:
            piv.piv_pairs(a, (16, 16), (16, 16), search_area_size=(32, 32))
        finally:
            _lib.set_option("norm_clip", 1)


def test_signal_threshold_where_only_the_small_window_fails(gpu):
    a = particle_stack(**OPT_STACK)
    a[0, 8:24, 8:24] = 0        # the 16 x 16 window of tile (0, 0) in frame 0 is empty, its 32 x 32 tile is not
    r = ref.search_piv(a, (16, 16), (32, 32), (16, 16), 0.05)
    assert np.isnan(r["corr"][0, 0, 0]) and (a[0, :32, :32] != 0).mean() >= 0.05 and np.isfinite(r["corr"][1, 0, 0])
    gate(piv.piv_pairs(a, (16, 16), (16, 16), 0.05, search_area_size=(32, 32)), r)


def test_rescue_covers_sparse_integer_particles(gpu):
    """Single bright pixels: the neighbours of a correlation peak are exactly zero, the float32 log fit is ill-conditioned there."""
    rng = np.random.default_rng(5)
    a = np.zeros((3, 70, 101), np.uint8)
    yy, xx = rng.integers(2, 66, 500), rng.integers(2, 94, 500)
    for t in range(3):
        a[t, yy + t, xx + 2 * t] = rng.integers(100, 255, 500)
        a[t, yy + t, xx + 2 * t + 1] = 60
    r = ref.search_piv(a, (16, 16), (32, 32), (16, 16))
    before = (C.c_int64 * 5)()
    _lib.check(_lib.load().lspiv_rescue_stats(None, before))
    gate(piv.piv_pairs(a, (16, 16), (16, 16), search_area_size=(32, 32)), r)
    after = (C.c_int64 * 5)()
    _lib.check(_lib.load().lspiv_rescue_stats(None, after))
    print("rescued:", after[2] - before[2], after[3] - before[3], "ties:", int(r["tie"].sum()))
    assert (after[2] - before[2]) + (after[3] - before[3]) > 0


def test_fast_flow_is_recovered_with_a_search_area(gpu):
    a = fast_stack()
    u, v, _, _ = piv.piv_pairs(a, (12, 12), (16, 16), search_area_size=(32, 32))
    mu, mv, share = fast_flow_shares(u, v)
    print("12 in 32:", mu, mv, share)
    assert mu < 0.1 and mv < 0.1 and share >= 0.95
    u, v, _, _ = piv.piv_pairs(a, (12, 12), (6, 6))
    print("plain 12:", fast_flow_shares(u, v)[2])
    assert fast_flow_shares(u, v)[2] < 0.2


def test_search_area_equal_to_window_is_todays_call(gpu):
    a = particle_stack(4, 90, 120, seed=8, density=0.05)
    for g, h in zip(piv.piv_pairs(a, (32, 32), (16, 16), 0.02, return_planes=True, search_area_size=(32, 32)),
                    piv.piv_pairs(a, (32, 32), (16, 16), 0.02, return_planes=True)):
        assert np.array_equal(g, h, equal_nan=True)
    ds = frames.get_piv(a, 32, search_area_size=32)
    ds0 = frames.get_piv(a, 32)
    assert all(np.array_equal(np.asarray(ds[k]), np.asarray(ds0[k]), equal_nan=True) for k in ("v_x", "v_y", "corr", "s2n"))
    fast = frames.get_piv(fast_stack(), 12, search_area_size=32)
    assert np.asarray(fast["v_x"]).shape == (1, 9, 9) and abs(float(np.nanmedian(np.asarray(fast["v_x"]))) - 10.0) < 0.1
