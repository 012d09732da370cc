"""Vector validation on the GPU against tests/validate_ref.py, the float32 numpy restatement of the rule:
``lspiv_validate`` (host pointers) and ``lspiv_validate_dev`` (device pointers) through ``pyorc_amd.validate``, then ``get_ffpiv(validate=)``
on every kind of stack.  The gate is EXACT -- equality by value, NaN positions included (``np.array_equal(..., equal_nan=True)``; the sign
of a zero is not compared) -- because the rule is built from selections and single correctly rounded float32 operations.
tests/test_validate_host.py shows from the reference alone that the shared inputs hold every flag class, every neighbour count, judged
and unjudged centres and substituted vectors that fall in a later iteration."""
import ctypes as C
import itertools

import numpy as np
import pytest

from pyorc_amd import _lib, frames, piv, validate, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import deform_ref, lazy_doubles, masked_ref, peak2_ref
from tests import validate_ref as ref
from tests.test_gpu_multipass import _Lazy

pytestmark = pytest.mark.gpu
COMBOS = list(itertools.product(("nan", "median"), (False, True), (1, 2, 3), (1, 3, 8)))     # replace, peak2, iterations, min_neighbours
PAD = 64


def same(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), (what, k)


def _to_device(a):
    d = DeviceFrames.empty((1, 1, a.nbytes), np.uint8)
    _lib.check(_lib.load().lspiv_memcpy_h2d(d.c_ptr, _lib.ptr(a), a.nbytes))
    return d


def _to_host(d, like):
    out = np.empty_like(like)
    _lib.check(_lib.load().lspiv_memcpy_d2h(_lib.ptr(out), d.c_ptr, out.nbytes))
    return out


def run_dev(u, v, p2, with_flag=True, **kw):
    """``lspiv_validate_dev`` on a result block [u | v | corr | s2n] in HBM with canaries around and inside it (corr and s2n hold a
    pattern), a canary-framed peak2 and a canary-framed flag buffer: ``(u, v, flag or None)`` after checking that nothing else moved."""
    spec = validate.validate_spec(True, **kw)
    N = u.size
    rng = np.random.default_rng(N)
    blk = rng.random(4 * N + 2 * PAD).astype(np.float32)
    blk[PAD:PAD + N], blk[PAD + N:PAD + 2 * N] = u.ravel(), v.ravel()
    sec = rng.random(4 * N + 2 * PAD).astype(np.float32)
    if p2 is not None:
        sec[PAD:PAD + 4 * N] = p2.ravel()
    fl = rng.integers(0, 256, N + 2 * PAD).astype(np.uint8)
    d_blk, d_sec, d_fl = _to_device(blk), _to_device(sec), _to_device(fl)
    at = lambda d, off: C.c_void_p(d.ptr + off)
    validate.run_dev(spec, at(d_blk, 4 * PAD), at(d_blk, 4 * (PAD + N)), at(d_sec, 4 * PAD) if p2 is not None else None, u.shape,
                     at(d_fl, PAD) if with_flag else None)
    blk2, sec2, fl2 = _to_host(d_blk, blk), _to_host(d_sec, sec), _to_host(d_fl, fl)
    assert np.array_equal(blk2[:PAD], blk[:PAD]) and np.array_equal(blk2[PAD + 2 * N:], blk[PAD + 2 * N:]), "corr, s2n or a canary of the block moved"
    assert np.array_equal(sec2, sec, equal_nan=True), "peak2 or its canaries moved"
    assert np.array_equal(fl2[:PAD], fl[:PAD]) and np.array_equal(fl2[PAD + N:], fl[PAD + N:]), "a canary of the flags moved"
    if not with_flag:
        assert np.array_equal(fl2, fl), "flags written without a flag buffer"
    return blk2[PAD:PAD + N].reshape(u.shape), blk2[PAD + N:PAD + 2 * N].reshape(u.shape), fl2[PAD:PAD + N].reshape(u.shape) if with_flag else None


def run_host(u, v, p2, with_flag=True, **kw):
    """``lspiv_validate`` on copies of the host arrays: ``(u, v, flag or None)``; peak2 must come back as it went in."""
    spec = validate.validate_spec(True, **kw)
    uu, vv = np.array(u), np.array(v)
    sec = None if p2 is None else np.array(p2)
    flag = np.full(u.shape, 0xAB, np.uint8) if with_flag else None
    validate.run_host(spec, uu, vv, sec, flag)
    if p2 is not None:
        assert np.array_equal(sec, p2, equal_nan=True), "peak2 moved"
    return uu, vv, flag


# ---- 1. the two entry points against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ref.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_both_entry_points_equal_the_reference(gpu, grid):
    u, v, p2 = ref.field(grid)
    for replace, second, it, m in COMBOS:
        want = ref.expected(grid, second, replace, it, m)
        kw = dict(replace=replace, iterations=it, min_neighbours=m)
        same(run_host(u, v, p2 if second else None, **kw), want, ("host", kw, second))
        same(run_dev(u, v, p2 if second else None, **kw), want, ("dev", kw, second))
        same(validate.median_test(u, v, p2 if second else None, **kw), want, ("median_test", kw, second))
    # flag NULL: the same fields
    for replace, second in itertools.product(("nan", "median"), (False, True)):
        want = ref.expected(grid, second, replace, 3, 3)[:2]
        kw = dict(replace=replace, iterations=3)
        same(run_host(u, v, p2 if second else None, with_flag=False, **kw)[:2], want, ("host, no flags", kw, second))
        same(run_dev(u, v, p2 if second else None, with_flag=False, **kw)[:2], want, ("dev, no flags", kw, second))


def test_other_thresholds_and_epsilons(gpu):
    u, v, p2 = ref.field((3, 37, 131))
    for thr, eps in ((1.0, 0.0), (3.5, 0.25), (0.3, 0.1)):
        want = ref.median_test(u, v, p2, threshold=thr, epsilon=eps, iterations=2, replace="median")
        same(run_dev(u, v, p2, threshold=thr, epsilon=eps, iterations=2, replace="median"), want, (thr, eps))
        same(validate.median_test(u, v, p2, threshold=thr, epsilon=eps, iterations=2, replace="median"), want, (thr, eps))


def test_two_dimensional_fields_and_new_arrays(gpu):
    u, v, p2 = ref.field((2, 5, 7))
    got = validate.median_test(u[0], v[0], p2[0], replace="median")
    same(got, [q[0] for q in ref.median_test(u[:1], v[:1], p2[:1], replace="median")], "(R, C)")
    assert got[0].shape == (5, 7) and got[2].dtype == np.uint8
    assert not any(np.shares_memory(g, q) for g in got for q in (u, v, p2))      # (the inputs are read-only: a write would have raised)
    same(validate.median_test(u.astype(np.float64), v.astype(np.float64), p2.astype(np.float64)), ref.expected((2, 5, 7), True, "nan", 1, 3), "float64 in")


def test_wrap_field_has_no_flags(gpu):
    u, v = ref.wrap_field()
    for kw in (dict(), dict(replace="median", iterations=3), dict(min_neighbours=1)):
        for got in (run_host(u, v, None, **kw), run_dev(u, v, None, **kw)):
            assert not got[2].any(), kw
            same(got[:2], (u, v), kw)


def test_two_runs_give_equal_results(gpu):
    u, v, p2 = ref.field((3, 37, 131))
    for kw in (dict(iterations=3, replace="median"), dict(iterations=2)):
        same(run_dev(u, v, p2, **kw), run_dev(u, v, p2, **kw), kw)
        same(run_host(u, v, p2, **kw), run_host(u, v, p2, **kw), kw)
    # a larger call in between grows the library's workspace: the next small call is still the reference's
    big = np.tile(u, (4, 2, 2)), np.tile(v, (4, 2, 2))
    same(run_dev(big[0], big[1], None, iterations=2), ref.median_test(big[0], big[1], iterations=2), "grown workspace")
    same(run_dev(u, v, p2, iterations=3), ref.expected((3, 37, 131), True, "nan", 3, 3), "after growing")


def test_entry_points_refuse_bad_arguments(gpu):
    lib = gpu
    buf = DeviceFrames.empty((1, 1, 256), np.uint8)
    q = buf.c_ptr
    call = lambda T=1, R=2, C=2, thr=2.0, eps=0.1, m=3, rep=0, it=1: lib.lspiv_validate_dev(q, q, None, T, R, C, thr, eps, m, rep, it, None, None)
    for kw in (dict(T=0), dict(R=0), dict(C=0), dict(thr=-1.0), dict(eps=-0.5), dict(m=0), dict(m=9), dict(rep=2), dict(it=0), dict(it=9)):
        assert call(**kw) == _lib.LSPIV_EINVAL, kw


# ---- 2. what it gains, on the device's own fields -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5])
def test_sparse_scene_on_the_devices_own_fields(gpu, seed):
    n, ov = peak2_ref.SPARSE_WINDOW
    u, v, cm, sn, p2 = piv.piv_pairs_peak2(peak2_ref.sparse_stack(seed), (n, n), (ov, ov))
    for replace in ("nan", "median"):
        same(validate.median_test(u, v, p2, replace=replace), ref.median_test(u, v, p2, replace=replace), replace)
    un, vn, fn = validate.median_test(u, v, p2)
    fin, still, sub = np.isfinite(u) & np.isfinite(v), np.isfinite(un) & np.isfinite(vn), fn == 2
    before, after = ref.share_within(u, v, peak2_ref.TRUTH, fin), ref.share_within(un, vn, peak2_ref.TRUTH, still)
    good_sub = int((peak2_ref.within_half_px(un, vn) & sub).sum())
    print(f"seed {seed}: before {before:.3f} after {after:.3f} rejected {int((fn == 1).sum())} substituted {int(sub.sum())}, within 0.5 px {good_sub}")
    assert after > before
    assert sub.sum() >= 1 and good_sub == sub.sum()


# ---- 3. get_ffpiv(validate=) -------------------------------------------------------------------------------------------------------------------
DT = np.array([0.5, 0.25, 2.0])
RES_X, RES_Y = 0.02, 0.03
scaled = lambda q, res: (q * res / DT[:, None, None]).astype(np.float32)


def _mode(mode):
    """(stack, n, ov, get_ffpiv keywords, the unvalidated run in pixels: (u, v, corr, s2n[, peak2]))."""
    if mode == "image_mask":
        a, m = deform_ref.pass_stack(16), masked_ref.case_mask(16)
        return a, 16, 8, dict(image_mask=m), piv.piv_pairs_masked(a, (16, 16), (8, 8), m)
    a = peak2_ref.sparse_stack(5)
    n, ov = peak2_ref.SPARSE_WINDOW
    if mode == "plain":
        return a, n, ov, dict(), piv.piv_pairs(a, (n, n), (ov, ov))
    if mode == "peak_ratio":
        return a, n, ov, dict(peak_ratio=True), piv.piv_pairs_peak2(a, (n, n), (ov, ov))
    return a, n, ov, dict(spectral_filter="spof"), piv.piv_pairs_filtered(a, (n, n), (ov, ov), "spof")


@pytest.mark.parametrize("mode", ["plain", "peak_ratio", "image_mask", "spof"])
def test_get_ffpiv_validates_in_pixels_on_every_kind_of_stack(gpu, mode):
    a, n, ov, kw, px = _mode(mode)
    assert len(a) == 4
    nr, nc = window.get_array_shape(a.shape[1:], (n, n), (ov, ov))
    run = lambda f, **more: velocimetry.get_ffpiv(f, np.arange(nr), np.arange(nc), DT, (n, n), (ov, ov), (n, n), RES_Y, RES_X, **kw, **more)
    second = px[4] if mode == "peak_ratio" else None
    for v_kw in (True, dict(replace="median", iterations=2, min_neighbours=2)):
        opts = {} if v_kw is True else v_kw
        un, vn, fn = ref.median_test(px[0], px[1], second, **opts)
        same(validate.median_test(px[0], px[1], second, **opts), (un, vn, fn), "median_test on the unvalidated fields")
        print(mode, v_kw, "flags", np.bincount(fn.ravel(), minlength=4).tolist())
        want = {"v_x": scaled(un, RES_X), "v_y": scaled(vn, RES_Y), "corr": px[2], "s2n": px[3], "flag": fn}
        if second is not None:
            want.update(v_x2=scaled(second[..., 0], RES_X), v_y2=scaled(second[..., 1], RES_Y), corr2=second[..., 2], peak_ratio=second[..., 3])
        t = np.arange(len(a))
        for f, more in ((a, dict()), (DeviceFrames.from_host(a), dict()), (_Lazy(a), dict()), (a, dict(chunksize=2)), (a, dict(chunksize=3)),
                        (a, dict(devices=[0, 0])), (DeviceFrames.from_host(a), dict(chunksize=2)), (_Lazy(a), dict(chunksize=3)),
                        (lazy_doubles.from_frames(a, block=2), dict(time=t)), (lazy_doubles.from_frames(a, block=3), dict(time=t, devices=[0, 0], chunksize=2))):
            got = run(f, validate=v_kw, **more)
            assert set(got) == set(want), (type(f).__name__, more)
            assert np.asarray(got["flag"]).dtype == np.uint8
            same([np.asarray(got[k]) for k in want], list(want.values()), (mode, type(f).__name__, more))
    if mode != "image_mask":
        assert (fn == 3).any() and (ref.median_test(px[0], px[1], second)[2] != 0).any()     # the validation had something to do
    # validate=None is today's result, bit for bit, without the new variable
    plain, none = run(a), run(a, validate=None)
    assert set(none) == set(plain) and "flag" not in none
    for k in plain:
        assert np.asarray(plain[k]).tobytes() == np.asarray(none[k]).tobytes(), k
    same([np.asarray(plain[k]) for k in ("v_x", "v_y", "corr", "s2n")], [scaled(px[0], RES_X), scaled(px[1], RES_Y), px[2], px[3]], "the unvalidated run")


def test_search_area_and_numpy_scalar_resolutions(gpu):
    """A search area of its own, and resolutions of numpy's float64 type (the host keeps numpy's own arithmetic then)."""
    a = peak2_ref.sparse_stack(6)
    u, v, cm, sn = piv.piv_pairs(a, (16, 16), (16, 16), search_area_size=(32, 32))
    un, vn, fn = ref.median_test(u, v)
    assert (fn == 1).any()
    nr, nc = u.shape[1:]
    got = velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), DT, (16, 16), (16, 16), (32, 32), RES_Y, RES_X, validate=True)
    same([np.asarray(got[k]) for k in ("v_x", "v_y", "corr", "s2n", "flag")], [scaled(un, RES_X), scaled(vn, RES_Y), cm, sn, fn], "search area")
    n, ov = peak2_ref.SPARSE_WINDOW
    u, v, cm, sn = piv.piv_pairs(a, (n, n), (ov, ov))
    un, vn, fn = ref.median_test(u, v)
    nr, nc = u.shape[1:]
    for f in (a, DeviceFrames.from_host(a)):
        got = velocimetry.get_ffpiv(f, np.arange(nr), np.arange(nc), DT, (n, n), (ov, ov), (n, n), np.float64(RES_Y), np.float64(RES_X), validate=True)
        same([np.asarray(got[k]) for k in ("v_x", "v_y", "flag")],
             [(un * np.float64(RES_X) / DT[:, None, None]).astype(np.float32), (vn * np.float64(RES_Y) / DT[:, None, None]).astype(np.float32), fn], "float64 resolutions")


def test_per_pair_calls_return_the_flags_last(gpu):
    a = peak2_ref.sparse_stack(5)
    n, ov = peak2_ref.SPARSE_WINDOW
    u, v, cm, sn, p2 = piv.piv_pairs_peak2(a, (n, n), (ov, ov))
    want = ref.median_test(u, v, p2, replace="median")
    for stack in (a, DeviceFrames.from_host(a)):
        got = piv.piv_pairs_peak2(stack, (n, n), (ov, ov), validate={"replace": "median"}, return_planes=True)
        assert len(got) == 7
        same((got[0], got[1], got[6], got[2], got[3], got[4]), (*want, cm, sn, p2), type(stack).__name__)
        got = piv.piv_pairs_peak2(stack, (n, n), (ov, ov), validate={"replace": "median"}, scale=(RES_X, RES_Y, DT))
        same((got[0], got[1], got[5], got[4][..., 0], got[4][..., 2]), (scaled(want[0], RES_X), scaled(want[1], RES_Y), want[2], scaled(p2[..., 0], RES_X), p2[..., 2]),
             (type(stack).__name__, "scaled"))
    u, v, cm, sn = piv.piv_pairs(a, (n, n), (ov, ov))
    out = [np.empty_like(u) for _ in range(4)]
    for stack in (a, DeviceFrames.from_host(a)):
        got = piv.piv_pairs(stack, (n, n), (ov, ov), validate=True, out=out, scale=(RES_X, RES_Y, DT))
        assert len(got) == 5 and all(g is o for g, o in zip(got, out))
        w = ref.median_test(u, v)
        same(got, (scaled(w[0], RES_X), scaled(w[1], RES_Y), cm, sn, w[2]), type(stack).__name__)


def test_frames_get_piv_and_the_wrapped_accessor(gpu, monkeypatch):
    """``frames.get_piv(..., validate=)`` and ``Frames.get_piv(engine="hip", validate=)`` run the median test of ``get_ffpiv``."""
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    a = peak2_ref.sparse_stack(5)
    u, v, cm, sn, p2 = piv.piv_pairs_peak2(a, (32, 32), (16, 16))
    keys = ("v_x", "v_y", "corr", "s2n", "flag")
    w1, w2 = ref.median_test(u, v, p2), ref.median_test(u, v, p2, replace="median", iterations=2)
    assert not ref.same(w1[0], w2[0])
    same([np.asarray(frames.get_piv(a, 32, peak_ratio=True, validate=True)[k]) for k in keys], (w1[0], w1[1], cm, sn, w1[2]), "frames.get_piv")
    opts = {"replace": "median", "iterations": 2}
    same([np.asarray(frames.get_piv(a, 32, peak_ratio=True, validate=opts, chunksize=2)[k]) for k in keys], (w2[0], w2[1], cm, sn, w2[2]), "frames.get_piv, dict")
    plain = frames.get_piv(a, 32)
    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(32, engine="hip", peak_ratio=True, validate=True)
        same([np.asarray(via[k]) for k in keys], (w1[0], w1[1], cm, sn, w1[2]), "wrapped accessor")
        via = rd.Frames(a).get_piv(**{"window_size": 32, "engine": "hip", "peak_ratio": True, "validate": opts})
        same([np.asarray(via[k]) for k in keys], (w2[0], w2[1], cm, sn, w2[2]), "wrapped accessor, keywords")
        p = piv.piv_pairs(a, (32, 32), (16, 16))
        wp = ref.median_test(p[0], p[1])
        via = rd.Frames(a).get_piv(32, engine="hip", validate=True)
        same([np.asarray(via[k]) for k in keys], (wp[0], wp[1], p[2], p[3], wp[2]), "wrapped accessor, plain path")
        # (without the keyword the wrapped accessor runs the reference's own method body, which this double does not have)
        none = frames.get_piv(a, 32, validate=None)
        assert set(none) == set(plain) and all(np.asarray(none[k]).tobytes() == np.asarray(plain[k]).tobytes() for k in plain)
        with pytest.raises(ValueError, match="min_neighbours"):
            rd.Frames(a).get_piv(32, engine="hip", validate={"min_neighbours": 0})
        with pytest.raises(NotImplementedError, match="validate together with ensemble_corr=True"):
            rd.Frames(a).get_piv(32, engine="hip", validate=True, ensemble_corr=True)
    finally:
        plugin.uninstall()
