"""PIV under an image mask on the GPU against tests/masked_ref.py, the float64 reference, through the C ABI
(``piv.piv_pairs_masked``: the device entry point for ``DeviceFrames``, the host-fed one for numpy stacks) and through ``get_ffpiv``.
Gate: NaN masks identical to the reference's; u, v and corr within 1e-4, s2n within 1e-4 max(1, |s2n|), planes within 2e-6, on EVERY
window -- tests/test_masked_host.py shows from the reference alone that the parity inputs hold no tie and no fragile window.  The rescue
inputs hold fragile windows by construction, most of them on partially covered windows: there the float64 rescue pass under the mask is
what holds the gate."""
import ctypes as C

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import deform_ref, lazy_doubles, multipass_ref
from tests import masked_ref as ref
from tests.test_gpu_multipass import KEYS, _Lazy

pytestmark = pytest.mark.gpu
TOL, TOL_PLANE = 1e-4, 2e-6
CASES = list(ref.PASS_CASES)
IDS = ["u8", "f32", "f64"]
WORST = {}


def abs_err(got, want, scale=None):
    with np.errstate(all="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - want)
        if scale is not None:
            e = e / scale
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


def same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True), (what, k)


def gate(got, r, planes=None, ok=None, names=("u", "v", "corr", "s2n"), what=""):
    """Every window (or those of ``ok``) against the reference; prints each figure before it asserts."""
    got = dict(zip(("u", "v", "corr", "s2n"), (np.asarray(q) for q in got)))
    ok = np.ones(r["corr"].shape, bool) if ok is None else ok
    for name in names:
        g, x = got[name], r[name]
        assert g.dtype == np.float32 and g.shape == x.shape
        with np.errstate(invalid="ignore"):
            err = abs_err(g[ok], x[ok], np.maximum(1.0, np.abs(x[ok])) if name == "s2n" else None)
        WORST[name] = max(WORST.get(name, 0.0), err)
        print(what, name, err)
        assert np.array_equal(np.isnan(g)[ok], np.isnan(x)[ok]), f"{name}: NaN mask differs"
        assert err <= TOL, name
    if planes is not None:
        flat = ok.reshape(ok.shape[0], -1)
        assert planes.dtype == np.float32 and planes.shape == r["planes"].shape
        err = abs_err(planes[flat], r["planes"][flat])
        WORST["planes"] = max(WORST.get("planes", 0.0), err)
        print(what, "planes", err)
        assert np.array_equal(np.isnan(planes)[flat], np.isnan(r["planes"])[flat])
        assert err <= TOL_PLANE


def run_public(a, n, ov, **kw):
    nr, nc = window.get_array_shape(a.shape[1:], (n, n), (ov, ov))
    return velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), np.ones(len(a) - 1), (n, n), (ov, ov), (n, n), 1.0, 1.0, **kw)


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES)
def test_pairs_match_the_reference_on_every_window(gpu, case, dtype):
    n, ov, _ = ref.PASS_CASES[case]
    a, m, r = deform_ref.pass_stack(case, dtype), ref.case_mask(case), ref.pass_ref(case, dtype)
    assert np.isnan(r["corr"]).any() and np.isfinite(r["corr"]).any()
    *dev, dplanes = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, return_planes=True)
    gate(dev, r, dplanes, what=f"{case} {np.dtype(dtype).name} device")
    *host, planes = piv.piv_pairs_masked(a, (n, n), (ov, ov), m, return_planes=True)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(host + [planes], dev + [dplanes], "host-fed and device entry points differ")
    else:
        gate(host, r, planes, what=f"{case} float64 host-fed")
    same_bits(piv.piv_pairs_masked(a, (n, n), (ov, ov), m), host, "without planes")
    pub = run_public(a, n, ov, image_mask=m)
    same_bits([np.asarray(pub[k]) for k in KEYS], host, "get_ffpiv")
    assert np.nanmax(dplanes) <= 1.0 and np.nanmin(dplanes) >= 0.0
    print("worst so far", WORST)


@pytest.mark.parametrize("case", CASES)
def test_signal_threshold_is_the_share_among_the_valid_samples(gpu, case):
    n, ov, _ = ref.PASS_CASES[case]
    m, r = ref.case_mask(case), ref.signal_ref(case)
    for dtype in ref.PASS_DTYPES:       # (the float stacks hold the same sample values: an affine map would move the zeros)
        got = piv.piv_pairs_masked(DeviceFrames.from_host(deform_ref.signal_stack(case).astype(dtype)), (n, n), (ov, ov), m,
                                   signal_threshold=ref.SIGNAL_THR, return_planes=True)
        gate(got[:4], r, got[4], what=f"{case} signal {np.dtype(dtype).name}")
    host = piv.piv_pairs_masked(deform_ref.signal_stack(case), (n, n), (ov, ov), m, signal_threshold=ref.SIGNAL_THR, return_planes=True)
    gate(host[:4], r, host[4], what=f"{case} signal host-fed")
    pub = run_public(deform_ref.signal_stack(case), n, ov, image_mask=m, signal_threshold=ref.SIGNAL_THR)
    same_bits([np.asarray(pub[k]) for k in KEYS], host[:4], "get_ffpiv")


@pytest.mark.parametrize("option,value", [("border_peak", 1), ("border_peak", 2), ("std_ddof", 1), ("v_sign", 1), ("signal_positive", 1)])
def test_options_flipped_in_library_and_reference(gpu, option, value):
    n, ov, _ = ref.PASS_CASES[16]
    a, m = deform_ref.signal_stack(16), ref.case_mask(16)
    thr = ref.SIGNAL_THR if option == "signal_positive" else None
    _lib.set_option(option, value)
    try:
        for dtype in (np.uint8, np.float32):
            got = piv.piv_pairs_masked(DeviceFrames.from_host(a.astype(dtype)), (n, n), (ov, ov), m, signal_threshold=thr, return_planes=True)
            with po.semantics(**{option: value}):
                r = ref.piv(a.astype(dtype), n, ov, m, signal_threshold=thr)
            gate(got[:4], r, got[4], what=f"{option}={value} {np.dtype(dtype).name}")
    finally:
        _lib.set_option(option, 0)
    base = ref.piv(a, n, ov, m, signal_threshold=thr)
    changed = {"border_peak": "u", "std_ddof": "corr", "v_sign": "v", "signal_positive": None}[option]
    if changed:
        assert not np.array_equal(r[changed], base[changed], equal_nan=True)


def test_unsupported_options_are_refused(gpu):
    a, m = deform_ref.pass_stack(16), ref.case_mask(16)
    for opt, val, back in (("norm_clip", 0, 1), ("signal_mode", 1, 0)):
        _lib.set_option(opt, val)
        try:
            for call in (lambda: piv.piv_pairs_masked(a, (16, 16), (8, 8), m), lambda: piv.piv_pairs_masked(DeviceFrames.from_host(a), (16, 16), (8, 8), m),
                         lambda: frames.get_piv(a, 16, image_mask=m, signal_threshold=0.05)):
                with pytest.raises(ValueError, match=opt) as e:
                    call()
                assert e.value.code == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, back)


@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES)
def test_a_constant_valid_region_gives_an_exactly_zero_plane(gpu, case, dtype):
    """k equal samples: the float64 reference finds zero variance and an all-zero plane for any k; float32 sums over a k that is no power
    of two do so only around a pivot (piv_masked_impl.h, center_clip_masked)."""
    n, ov, dim = ref.PASS_CASES[case]
    a, m = deform_ref.pass_stack(case, dtype).copy(), ref.case_mask(case)
    a[:, :n] = 37 if dtype == np.uint8 else np.float32(-11.3)       # the top row of windows, in every frame
    a[1, :n, ::3] = 5                                               # ... but not in frame 1: pairs 0 and 1 are dead there, pair 2 is
    _, k = ref.window_masks(m, n, ov)
    cols = window.get_array_shape(dim, (n, n), (ov, ov))[1]
    top = np.flatnonzero((k[:cols] >= ref.k_min(n)))
    assert ((k[top] & (k[top] - 1)) != 0).any()                     # some k is no power of two
    r = ref.piv(a, n, ov, m)
    got = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, return_planes=True)
    gate(got[:4], r, got[4], what="constant valid region")
    assert not got[4][:, top].any() and not r["planes"][:, top].any() and (got[2][:, 0, top] == 0).all() and np.isnan(got[3][:, 0, top]).all()


# ---- 2. the float64 rescue pass under the mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=IDS[:2])
@pytest.mark.parametrize("n,ov", ref.RESCUE_GEOMETRIES)
def test_rescue_pass_holds_the_gate_on_partially_covered_windows(gpu, n, ov, dtype):
    a, m, r = multipass_ref.rescue_stack(dtype), ref.rescue_mask(), ref.rescue_ref(n, ov, dtype)
    kept = np.isfinite(r["corr"])
    fragile = r["fragile"] & kept
    assert fragile.any() and not r["tie"].any()
    d = DeviceFrames.from_host(a)
    lib = _lib.load()
    before = np.zeros(5, np.int64)
    _lib.check(lib.lspiv_rescue_stats(None, before.ctypes.data_as(C.POINTER(C.c_int64))))
    on = piv.piv_pairs_masked(d, (n, n), (ov, ov), m, return_planes=True)
    after = np.zeros(5, np.int64)
    _lib.check(lib.lspiv_rescue_stats(None, after.ctypes.data_as(C.POINTER(C.c_int64))))
    print(n, ov, np.dtype(dtype).name, "records of this pass: fit", after[0], "amb", after[1], "fragile windows", int(fragile.sum()))
    assert after[0] + after[1] > 0
    gate(on[:4], r, on[4], what=f"rescue on {n} @ {ov}")
    same_bits(piv.piv_pairs_masked(a, (n, n), (ov, ov), m, return_planes=True), on, "host-fed entry point")
    _lib.set_option("rescue", 0)
    try:
        off = piv.piv_pairs_masked(d, (n, n), (ov, ov), m, return_planes=True)
    finally:
        _lib.set_option("rescue", 1)
    gate(off[:4], r, off[4], ok=~fragile, what=f"rescue off, non-fragile {n} @ {ov}")
    same_bits(off[2:], on[2:], "the pass rewrites u and v alone")
    with np.errstate(invalid="ignore"):
        worst = max(abs_err(off[k][fragile], r[name][fragile]) for k, name in ((0, "u"), (1, "v")))
        nan_differs = not np.array_equal(np.isnan(off[0])[fragile], np.isnan(r["u"])[fragile])
    print(n, ov, np.dtype(dtype).name, "rescue off, worst u / v error on the fragile windows", worst, "NaN decisions differ", nan_differs)
    if (n, ov) == (16, 8):
        assert worst > TOL or nan_differs      # the pass does work here


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=IDS[:2])
def test_rescue_pass_settles_two_candidates_under_the_mask(gpu, dtype):
    """"rescue_tau" at its widest (1e-3): the 17 windows of the 16 @ 8 rescue input whose second-largest sample lies within 1e-3 of the
    maximum (counted from the reference) are listed with both candidates, and the pass compares their two float64 sums under the mask."""
    n, ov = 16, 8
    a, m, r = multipass_ref.rescue_stack(dtype), ref.rescue_mask(), ref.rescue_ref(n, ov, dtype)
    pl = np.nan_to_num(r["planes"].reshape(-1, n * n))
    near = (pl >= pl.max(axis=1, keepdims=True) * (1 - 1e-3)).sum(axis=1)[pl.max(axis=1) > 0]
    assert (near == 2).sum() == 17 and (near > 2).sum() == 0
    _lib.set_option("rescue_tau", 1000000)
    try:
        got = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, return_planes=True)
        stats = np.zeros(5, np.int64)
        _lib.check(_lib.load().lspiv_rescue_stats(None, stats.ctypes.data_as(C.POINTER(C.c_int64))))
    finally:
        _lib.set_option("rescue_tau", 4000)
    print(np.dtype(dtype).name, "records: fit", stats[0], "amb", stats[1])
    assert stats[0] >= 145 and stats[1] == 0
    gate(got[:4], r, got[4], what="two candidates")


@pytest.mark.parametrize("case", CASES)
def test_rescue_pass_re_evaluates_whole_planes_under_the_mask(gpu, case):
    """Three candidates within "rescue_tau" (at its widest, 1e-3) of the maximum: the window goes to the whole-plane kernel, which
    normalises both windows over their valid samples, zeroes the excluded ones and takes the first float64 maximum."""
    n, ov, _ = ref.PASS_CASES[case]
    a, m, r = ref.amb_stack(case), ref.case_mask(case), ref.amb_ref(case)
    assert (ref.near_maximum(r["planes"], 0.7e-3) >= 3).any()
    for stack in (a, a.astype(np.float64)):
        _lib.set_option("rescue_tau", 1000000)
        try:
            got = piv.piv_pairs_masked(DeviceFrames.from_host(stack), (n, n), (ov, ov), m, return_planes=True)
            stats = np.zeros(5, np.int64)
            _lib.check(_lib.load().lspiv_rescue_stats(None, stats.ctypes.data_as(C.POINTER(C.c_int64))))
        finally:
            _lib.set_option("rescue_tau", 4000)
        print(case, stack.dtype.name, "records: fit", stats[0], "amb", stats[1])
        assert stats[1] >= 1
        gate(got[:4], r, got[4], what="whole-plane rescue")
    b = a.copy()
    b[:, ~m] = np.nan
    _lib.set_option("rescue_tau", 1000000)
    try:
        same_bits(piv.piv_pairs_masked(DeviceFrames.from_host(b), (n, n), (ov, ov), m, return_planes=True),
                  piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, return_planes=True), "excluded samples in the whole-plane kernel")
    finally:
        _lib.set_option("rescue_tau", 4000)


# ---- 3. excluded samples never enter the arithmetic ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES)
def test_excluded_samples_change_no_bit(gpu, case, dtype):
    n, ov, _ = ref.PASS_CASES[case]
    a, m = deform_ref.pass_stack(case, dtype), ref.case_mask(case)
    clean = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, signal_threshold=0.01, return_planes=True)
    b = a.copy()
    rng = np.random.default_rng(7)
    if dtype == np.uint8:
        b[:, ~m] = rng.integers(0, 256, size=(len(a), int((~m).sum())), dtype=np.uint8)
    else:
        junk = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0], dtype=dtype)
        b[:, ~m] = junk[rng.integers(0, len(junk), size=(len(a), int((~m).sum())))]
    assert not np.array_equal(a, b, equal_nan=True)
    for rescue in (1, 0):
        _lib.set_option("rescue", rescue)
        try:
            base = clean if rescue else piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, signal_threshold=0.01, return_planes=True)
            same_bits(piv.piv_pairs_masked(DeviceFrames.from_host(b), (n, n), (ov, ov), m, signal_threshold=0.01, return_planes=True), base,
                      f"excluded samples leak, rescue {rescue}")
        finally:
            _lib.set_option("rescue", 1)
    if dtype != np.float64:
        same_bits(piv.piv_pairs_masked(b, (n, n), (ov, ov), m, signal_threshold=0.01, return_planes=True), clean, "host-fed entry point")
    # a non-finite VALID sample takes out the windows that hold it, and only those
    if dtype != np.uint8:
        c = a.copy()
        y, x = np.argwhere(m)[len(np.argwhere(m)) // 2]
        c[1, y, x] = np.nan
        gate(piv.piv_pairs_masked(DeviceFrames.from_host(c), (n, n), (ov, ov), m)[:4], ref.piv(c, n, ov, m), what="NaN on a valid sample")


def test_excluded_samples_change_no_bit_of_a_rescued_window(gpu):
    """The rescue inputs: their flagged windows are re-evaluated from the frames, where the excluded samples are junk now."""
    n, ov = 16, 8
    a, m = multipass_ref.rescue_stack(np.float32), ref.rescue_mask()
    clean = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (ov, ov), m, return_planes=True)
    b = a.copy()
    junk = np.array([np.nan, np.inf, -np.inf, 1e30], dtype=np.float32)
    b[:, ~m] = junk[np.random.default_rng(8).integers(0, 4, size=(len(a), int((~m).sum())))]
    same_bits(piv.piv_pairs_masked(DeviceFrames.from_host(b), (n, n), (ov, ov), m, return_planes=True), clean, "rescue pass reads excluded samples")
    u8 = multipass_ref.rescue_stack(np.uint8)
    c = u8.copy()
    c[:, ~m] = np.random.default_rng(9).integers(0, 256, size=(len(a), int((~m).sum())), dtype=np.uint8)
    same_bits(piv.piv_pairs_masked(DeviceFrames.from_host(c), (n, n), (ov, ov), m, return_planes=True),
              piv.piv_pairs_masked(DeviceFrames.from_host(u8), (n, n), (ov, ov), m, return_planes=True), "uint8")


# ---- 4. locality ---------------------------------------------------------------------------------------------------------------------------
def footprints(dim, n, ov):
    y0, x0 = (np.asarray(q) for q in po.window_origins(dim, (n, n), (ov, ov)))
    return y0, x0


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=IDS[:2])
@pytest.mark.parametrize("case", CASES)
def test_a_window_depends_on_its_own_samples_and_its_own_mask_alone(gpu, case, dtype):
    n, ov, dim = ref.PASS_CASES[case]
    a, m = deform_ref.pass_stack(case, dtype), ref.case_mask(case)
    d = DeviceFrames.from_host(a)
    base = piv.piv_pairs_masked(d, (n, n), (ov, ov), m, return_planes=True)
    y0, x0 = footprints(dim, n, ov)
    rows, cols = len(y0), len(x0)
    _, k = ref.window_masks(m, n, ov)
    # flip three pixels inside the footprint of one partially covered window
    w = int(np.flatnonzero((k >= ref.k_min(n)) & (k < n * n))[len(np.flatnonzero((k >= ref.k_min(n)) & (k < n * n))) // 2])
    wr, wc = divmod(w, cols)
    m2 = m.copy()
    pix = [(y0[wr] + 1, x0[wc] + 2), (y0[wr] + n // 2, x0[wc] + n // 2 + 1), (y0[wr] + n - 2, x0[wc] + n - 1)]
    for y, x in pix:
        m2[y, x] = ~m2[y, x]
    got = piv.piv_pairs_masked(d, (n, n), (ov, ov), m2, return_planes=True)
    touched = np.zeros((rows, cols), bool)
    for y, x in pix:
        touched |= ((y0[:, None] <= y) & (y < y0[:, None] + n) & (x0[None, :] <= x) & (x < x0[None, :] + n))
    assert touched[wr, wc] and not touched.all()
    for q in range(4):
        assert np.array_equal(got[q][:, ~touched], base[q][:, ~touched], equal_nan=True), q
    assert np.array_equal(got[4][:, ~touched.reshape(-1)], base[4][:, ~touched.reshape(-1)], equal_nan=True)
    assert not np.array_equal(got[4][:, w], base[4][:, w], equal_nan=True)
    # fully covered windows: the bits of the all-ones-mask run
    ones = piv.piv_pairs_masked(d, (n, n), (ov, ov), np.ones(dim, bool), return_planes=True)
    full = (k == n * n).reshape(rows, cols)
    assert full.any()
    for q in range(4):
        assert np.array_equal(base[q][:, full], ones[q][:, full], equal_nan=True), q
    assert np.array_equal(base[4][:, full.reshape(-1)], ones[4][:, full.reshape(-1)])
    # an all-ones mask against the shifted kernel at zero offsets (the same job, without the mask): inside the gate, bits reported
    shifted = piv.piv_pairs_shifted(d, (n, n), (ov, ov), None, return_planes=True)
    r = ref.piv(a, n, ov, np.ones(dim, bool))
    gate(ones[:4], r, ones[4], what="all-ones mask")
    for q, name in enumerate(("u", "v", "corr", "s2n")):
        assert np.array_equal(np.isnan(ones[q]), np.isnan(np.asarray(shifted[q]))), name
        with np.errstate(invalid="ignore"):
            scale = np.maximum(1.0, np.abs(np.asarray(shifted[q], np.float64))) if name == "s2n" else None
        assert abs_err(ones[q], np.asarray(shifted[q], np.float64), scale) <= TOL, name
    equal =[bool(np.array_equal(np.asarray(ones[q]), np.asarray(shifted[q]), equal_nan=True)) for q in range(5)]
    print(case, np.dtype(dtype).name, "all-ones mask bit-equal to the shifted kernel at zero offsets (u, v, corr, s2n, planes):", equal,
          "largest plane difference", abs_err(ones[4], np.asarray(shifted[4], np.float64)))
    assert abs_err(ones[4], np.asarray(shifted[4], np.float64)) <= TOL_PLANE


# ---- 5. the coverage edge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=IDS)
@pytest.mark.parametrize("n", ref.MASK_WINDOWS)
def test_coverage_edge_k_min_and_one_below(gpu, n, dtype):
    """2 x 3 windows without overlap on a frame they fill exactly (the last ones end on the frame's edge): exactly k_min valid samples,
    k_min - 1, all of them; none, one short of all, k_min in scattered places."""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, (3, 2 * n, 3 * n)).astype(dtype)
    for cov in (0.25, 0.031):
        kmin = ref.k_min(n, cov)
        m = np.zeros((2 * n, 3 * n), bool)
        flat = lambda cnt: (np.arange(n * n) < cnt).reshape(n, n)
        m[:n, :n] = flat(kmin)
        m[:n, n:2 * n] = flat(kmin - 1)
        m[:n, 2 * n:] = True
        m[n:, n:2 * n] = flat(n * n - 1)
        scattered = np.zeros(n * n, bool)
        scattered[rng.permutation(n * n)[:kmin]] = True
        m[n:, 2 * n:] = scattered.reshape(n, n)
        _, k = ref.window_masks(m, n, 0)
        assert list(k) == [kmin, kmin - 1, n * n, 0, n * n - 1, kmin]
        got = piv.piv_pairs_masked(DeviceFrames.from_host(a), (n, n), (0, 0), m, cov, return_planes=True)
        r = ref.piv(a, n, 0, m, cov)
        finite = np.isfinite(got[2]).reshape(2, -1)
        assert (finite == np.array([True, False, True, False, True, True])).all(), finite
        assert np.isfinite(got[3]).reshape(2, -1)[:, [0, 2, 4, 5]].all() and np.isfinite(got[4][:, [0, 2, 4, 5]]).all()
        assert np.isnan(got[4][:, [1, 3]]).all() and all(np.isnan(got[q]).reshape(2, -1)[:, [1, 3]].all() for q in range(4))
        gate(got[:4], r, got[4], ok=~r["fragile"], names=("corr", "s2n"), what=f"coverage edge {n} {cov}")


@pytest.mark.parametrize("case", CASES)
def test_nothing_valid_anywhere_is_all_nan(gpu, case):
    n, ov, dim = ref.PASS_CASES[case]
    for dtype in ref.PASS_DTYPES:
        a = deform_ref.pass_stack(case, dtype)
        for stack in (a, DeviceFrames.from_host(a)):
            got = piv.piv_pairs_masked(stack, (n, n), (ov, ov), np.zeros(dim, np.uint8), return_planes=True)
            assert all(np.isnan(np.asarray(q)).all() for q in got)
    # one valid pixel in the frame's last corner: still below k_min everywhere
    m = np.zeros(dim, bool)
    m[-1, -1] = True
    got = piv.piv_pairs_masked(deform_ref.pass_stack(case), (n, n), (ov, ov), m, 1e-9, return_planes=True)
    assert all(np.isnan(np.asarray(q)).all() for q in got)


# ---- 6. the paths ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_chunking_devices_device_stacks_and_lazy_stacks_give_the_same_bits(gpu, case):
    from tests import ensemble_multipass_ref as emp

    n, ov, dim = ref.PASS_CASES[case]
    a, m = emp.pass_stack(case, 7), ref.case_mask(case)               # six pairs
    whole = piv.piv_pairs_masked(a, (n, n), (ov, ov), m, return_planes=True)
    d = DeviceFrames.from_host(a)
    same_bits(piv.piv_pairs_masked(d, (n, n), (ov, ov), m, return_planes=True), whole, "DeviceFrames")
    spec = window.masked_spec((n, n), m, 0.25, dim)
    same_bits(piv.piv_pairs(d, spec, (ov, ov), return_planes=True), whole, "piv_pairs dispatches on a MaskedWindow")
    for size in (1, 2, 3):
        for start in (0, 1):                  # start = 1: every chunk but the first begins on an odd pair
            cuts = [0] + list(range(start, 6, size))[(1 if start == 0 else 0):] + [6]
            for stack in (a, d):
                parts = [piv.piv_pairs(stack[p0:p1 + 1], spec, (ov, ov), return_planes=True, pair_offset=p0) for p0, p1 in zip(cuts, cuts[1:])]
                same_bits([np.concatenate([p[k] for p in parts]) for k in range(5)], whole, (size, start))
    assert len(spec._device_masks) == 1       # one upload for all those chunks
    pub = run_public(a, n, ov, image_mask=m)
    same_bits([np.asarray(pub[k]) for k in KEYS], whole[:4], "get_ffpiv")
    for kw in (dict(chunksize=2), dict(chunksize=3), dict(chunksize=4), dict(devices=[0, 0]), dict(devices=[0, 0], chunksize=3)):
        same_bits([np.asarray(run_public(a, n, ov, image_mask=m, **kw)[k]) for k in KEYS], whole[:4], kw)
    same_bits([np.asarray(run_public(d, n, ov, image_mask=m, chunksize=3)[k]) for k in KEYS], whole[:4], "DeviceFrames through get_ffpiv")
    same_bits([np.asarray(run_public(_Lazy(a), n, ov, image_mask=m, chunksize=3)[k]) for k in KEYS], whole[:4], "lazy stack")
    for block, kw in ((2, dict()), (3, dict(chunksize=4)), (4, dict(devices=[0, 0], chunksize=3))):
        lazy = lazy_doubles.from_frames(a, block=block)
        got = run_public(lazy, n, ov, image_mask=m, time=np.arange(len(a)), **kw)
        same_bits([np.asarray(got[k]) for k in KEYS], whole[:4], ("lazy double", block, kw))


def test_no_mask_is_todays_path_bit_for_bit(gpu):
    n, ov, _ = ref.PASS_CASES[32]
    a = deform_ref.pass_stack(32)
    plain = run_public(a, n, ov)
    same_bits([np.asarray(run_public(a, n, ov, image_mask=None, mask_coverage_min=0.7)[k]) for k in KEYS], [np.asarray(plain[k]) for k in KEYS], "None")
    same_bits(piv.piv_pairs_masked(a, (n, n), (ov, ov), None, return_planes=True), piv.piv_pairs(a, (n, n), (ov, ov), return_planes=True), "piv_pairs")
    assert not np.array_equal(np.asarray(run_public(a, n, ov, image_mask=ref.case_mask(32))["corr"]), np.asarray(plain["corr"]), equal_nan=True)


def test_scale_and_out_arguments(gpu):
    n, ov, _ = ref.PASS_CASES[32]
    a, m = deform_ref.pass_stack(32), ref.case_mask(32)
    u, v, cm, sn = piv.piv_pairs_masked(a, (n, n), (ov, ov), m)
    out = [np.empty_like(u) for _ in range(4)]
    dt = np.array([0.5, 0.25, 2.0])
    for stack in (a, DeviceFrames.from_host(a)):
        got = piv.piv_pairs_masked(stack, (n, n), (ov, ov), m, out=out, scale=(0.02, 0.03, dt))
        assert all(g is o for g, o in zip(got, out))
        same_bits(got, ((u * 0.02 / dt[:, None, None]).astype(np.float32), (v * 0.03 / dt[:, None, None]).astype(np.float32), cm, sn), "scale")


def test_frames_get_piv_and_the_wrapped_accessor(gpu, monkeypatch):
    """``frames.get_piv(..., image_mask=)`` and ``Frames.get_piv(engine="hip", image_mask=)`` are ``piv_pairs_masked``."""
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    a, m = deform_ref.pass_stack(16), ref.case_mask(16)
    direct = piv.piv_pairs_masked(a, (16, 16), (8, 8), m)
    half = piv.piv_pairs_masked(a, (16, 16), (8, 8), m, 0.5)
    assert np.isnan(half[2]).sum() > np.isnan(direct[2]).sum()
    same_bits([np.asarray(frames.get_piv(a, 16, image_mask=m)[k]) for k in KEYS], direct, "frames.get_piv")
    same_bits([np.asarray(frames.get_piv(a, 16, image_mask=m.astype(np.float32), chunksize=2)[k]) for k in KEYS], direct, "frames.get_piv, chunks")
    same_bits([np.asarray(frames.get_piv(a, 16, image_mask=m, mask_coverage_min=0.5)[k]) for k in KEYS], half, "frames.get_piv, coverage")
    plain = frames.get_piv(a, 16)
    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(16, engine="hip", image_mask=m)
        same_bits([np.asarray(via[k]) for k in KEYS], direct, "wrapped accessor")
        via = rd.Frames(a).get_piv(**{"window_size": 16, "engine": "hip", "image_mask": m, "mask_coverage_min": 0.5})
        same_bits([np.asarray(via[k]) for k in KEYS], half, "wrapped accessor, keywords")
        # (without a mask the wrapped accessor runs the reference's own method body, which this double does not have)
        same_bits([np.asarray(frames.get_piv(a, 16, image_mask=None, mask_coverage_min=0.5)[k]) for k in KEYS], [np.asarray(plain[k]) for k in KEYS],
                  "frames.get_piv, no mask")
        with pytest.raises(ValueError, match=r"mask_coverage_min must lie in \(0, 1\]"):
            rd.Frames(a).get_piv(16, engine="hip", image_mask=m, mask_coverage_min=0.0)
        with pytest.raises(NotImplementedError, match="image_mask together with ensemble_corr=True"):
            rd.Frames(a).get_piv(16, engine="hip", image_mask=m, ensemble_corr=True)
    finally:
        plugin.uninstall()


# ---- 7. what the mask gains, on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ov", ref.BANK_WINDOWS)
def test_bank_scene_share_is_the_references(gpu, n, ov):
    a, m = ref.bank_scene(5, 0.03), ref.bank_mask()
    r = ref.bank_ref(5, 0.03, n, ov, True)
    sel = ref.partial_select(r["k"], n, r["u"].shape)
    got = piv.piv_pairs_masked(a, (n, n), (ov, ov), m)
    s_dev, s_ref = ref.share_within(got[0], got[1], sel), ref.share_within(r["u"], r["v"], sel)
    plain = piv.piv_pairs(a, (n, n), (ov, ov))
    print(f"{n} @ {ov}: device {s_dev:.3f} reference {s_ref:.3f} plain path on the device {ref.share_within(plain[0], plain[1], sel):.3f}")
    assert abs(s_dev - s_ref) <= 1.0 / sel.sum() + 1e-12
