"""PIV under an image mask, host side (CPU): the reference (tests/masked_ref.py) at full coverage, the CPU checks of the inputs
tests/test_gpu_masked.py relies on (window classes, no ties, fragile windows on partially covered windows), what the mask gains on the
bank scene, the keyword validation and the new refusals, the plugin's TypeError for another engine, the new symbols and the planner."""
import os
import re

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, shard, velocimetry, window
from tests import deform_ref, multipass_ref
from tests import masked_ref as ref
from tests import recipe_doubles as rd


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ref.PASS_CASES))
def test_full_coverage_is_the_plain_plane_exactly(case):
    n, ov, _ = ref.PASS_CASES[case]
    st = po.sliding_window_stack(deform_ref.pass_stack(case).astype(np.float64), (n, n), (ov, ov))
    ones = np.ones((n, n), dtype=bool)
    for w in range(st.shape[1]):
        assert np.array_equal(ref.plane(st[0, w], st[1, w], ones, n * n), po.ncc(st[0, w], st[1, w]))
    # ... and through piv(): an all-ones mask is the oracle's own per-pair result
    r = ref.piv(deform_ref.pass_stack(case), n, ov, np.ones(ref.PASS_CASES[case][2], bool))
    _, _, corr = po.cross_corr(deform_ref.pass_stack(case), (n, n), (ov, ov))
    assert np.array_equal(r["planes"], corr)


def test_excluded_samples_never_enter_the_reference():
    n, ov, dim = ref.PASS_CASES[32]
    a = deform_ref.pass_stack(32, np.float32).astype(np.float64)
    m = ref.case_mask(32)
    b = a.copy()
    b[:, ~m] = np.nan
    ra, rb = ref.piv(a, n, ov, m), ref.piv(b, n, ov, m)
    for key in ("u", "v", "corr", "s2n", "planes"):
        assert np.array_equal(ra[key], rb[key], equal_nan=True), key
    # a non-finite VALID sample takes its windows out
    c = a.copy()
    y, x = np.argwhere(m)[len(np.argwhere(m)) // 2]
    c[1, y, x] = np.inf
    rc = ref.piv(c, n, ov, m)
    y0, x0 = (np.asarray(q) for q in po.window_origins(dim, (n, n), (ov, ov)))
    hit = ((y0[:, None] <= y) & (y < y0[:, None] + n) & (x0[None, :] <= x) & (x < x0[None, :] + n))
    assert hit.any() and np.isnan(rc["corr"][0][hit]).all() and np.isnan(rc["corr"][1][hit]).all()
    assert np.array_equal(rc["corr"][2], ra["corr"][2], equal_nan=True)
    assert np.array_equal(rc["corr"][0][~hit], ra["corr"][0][~hit], equal_nan=True)


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
CLASSES = {16: (4, 16, 5), 32: (7, 20, 8), 64: (2, 14, 4)}


@pytest.mark.parametrize("case", sorted(ref.PASS_CASES))
def test_parity_inputs_have_every_window_class_and_no_tie_or_fragile_window(case):
    n, ov, _ = ref.PASS_CASES[case]
    _, k = ref.window_masks(ref.case_mask(case), n, ov)
    assert ref.classes(k, n) == CLASSES[case]
    for dtype in (np.uint8, np.float32):
        r = ref.pass_ref(case, dtype)
        kept = np.isfinite(r["corr"])
        assert kept.sum() == (r["corr"].shape[0]) * (CLASSES[case][0] + CLASSES[case][1])
        assert int(r["tie"].sum()) == 0 and int((r["fragile"] & kept).sum()) == 0
    s = ref.signal_ref(case)
    dropped = np.isnan(s["corr"]) & np.isfinite(ref.pass_ref(case)["corr"])
    print(case, "signal threshold drops", int(dropped.sum()), "of", int(np.isfinite(ref.pass_ref(case)["corr"]).sum()))
    assert dropped.any() and np.isfinite(s["corr"]).any() and int(s["tie"].sum()) == 0


FRAGILE = {(16, 8): (142, 1100, 85), (32, 16): (55, 228, 51), (64, 32): (12, 48, 12), (64, 48): (32, 152, 32)}


@pytest.mark.parametrize("n,ov", ref.RESCUE_GEOMETRIES)
def test_rescue_inputs_have_fragile_windows_on_partially_covered_windows(n, ov):
    r = ref.rescue_ref(n, ov)
    kept = np.isfinite(r["corr"])
    fr = r["fragile"] & kept
    partial = np.broadcast_to((r["k"] < n * n).reshape(kept.shape[1:]), kept.shape)
    assert (int(fr.sum()), int(kept.sum()), int((fr & partial).sum())) == FRAGILE[(n, ov)]
    assert int(r["tie"].sum()) == 0
    assert multipass_ref.RESCUE_DIM == (136, 200) and multipass_ref.RESCUE_T == 5


@pytest.mark.parametrize("case", sorted(ref.PASS_CASES))
def test_whole_plane_rescue_input_has_three_candidates_on_partially_covered_windows(case):
    n, ov, _ = ref.PASS_CASES[case]
    r = ref.amb_ref(case)
    three = (ref.near_maximum(r["planes"], 0.7e-3) >= 3) & (ref.near_maximum(r["planes"], 1.3e-3) == ref.near_maximum(r["planes"], 0.7e-3))
    partial = np.tile(r["k"] < n * n, r["planes"].shape[0])
    top = np.sort(np.nan_to_num(r["planes"].reshape(-1, n * n)), axis=1)[:, -2:]
    kept = top[:, 1] > 0
    print(case, "windows with three candidates", int(three.sum()), "on partially covered windows", int((three & partial).sum()),
          "smallest gap of the top two", ((top[kept, 1] - top[kept, 0]) / top[kept, 1]).min())
    assert (three & partial).sum() >= 1 and int(r["tie"].sum()) == 0
    assert ((top[kept, 1] - top[kept, 0]) / top[kept, 1]).min() >= 1e-4         # what float64 direct sums and float64 FFTs both resolve


# ---- what the mask gains -------------------------------------------------------------------------------------------------------------------
def test_mask_keeps_the_tracers_where_a_window_straddles_the_bank():
    """160 x 200 uint8, tracers moving by (3.3, -2.4) px right of a wavy bank line, a static texture left of it, 3 pairs; share of the
    windows with coverage in [0.25, 1) within 0.5 px of the truth, plain -> masked.  Measured (seed, density | 32 @ 16, 21 windows |
    64 @ 32, 8 windows): 5, 0.03 | 0.651 -> 0.889 | 0.625 -> 1.000; 5, 0.015 | 0.429 -> 0.857 | 0.500 -> 1.000; 6, 0.03 | 0.571 -> 0.921 |
    0.625 -> 1.000; 6, 0.015 | 0.508 -> 0.841 | 0.500 -> 1.000."""
    for seed, density in ref.BANK_INPUTS:
        for n, ov in ref.BANK_WINDOWS:
            m, p = ref.bank_ref(seed, density, n, ov, True), ref.bank_ref(seed, density, n, ov, False)
            sel = ref.partial_select(m["k"], n, m["u"].shape)
            s_plain, s_masked = ref.share_within(p["u"], p["v"], sel), ref.share_within(m["u"], m["v"], sel)
            print(seed, density, f"{n} @ {ov}", int(sel[0].sum()), "windows: plain %.3f masked %.3f" % (s_plain, s_masked))
            assert int(sel[0].sum()) == (21 if n == 32 else 8)
            if n == 32:
                assert s_masked - s_plain >= 0.15
            else:
                assert s_masked >= s_plain


# ---- argument checking ------------------------------------------------------------------------------------------------------------------------
def test_windows_coverage_and_mask_shape(lib):
    for n in (16, 32, 64):
        assert window.mask_supported((n, n)) == (n, n) and window.mask_supported(n) == (n, n)
    for ws in (24, (24, 24), (16, 32), (128, 128), (8, 8)):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            window.mask_supported(ws)
    assert [lib.lspiv_mask_supported(n, n) for n in (8, 16, 24, 32, 48, 64, 128)] == [0, 1, 0, 1, 0, 1, 0]
    assert lib.lspiv_mask_supported(16, 32) == 0 and lib.lspiv_abi_version() == 5
    m = np.ones((96, 96), bool)
    spec = window.masked_spec((32, 32), m, 0.25, (96, 96))
    assert isinstance(spec, window.MaskedWindow) and tuple(spec) == (32, 32) and spec.k_min == 256 and spec.mask_coverage_min == 0.25
    assert spec.image_mask.dtype == np.uint8 and spec.image_mask.flags.c_contiguous and spec.image_mask.shape == (96, 96)
    assert window.masked_spec(spec) is spec and window.masked_spec(spec, None, 0.25, (96, 96)) is spec
    assert window.masked_spec((32, 32), None) == (32, 32) and not isinstance(window.masked_spec((32, 32), None), window.MaskedWindow)
    for kind in (np.int16, np.float32, np.uint8):     # non-zero = valid, whatever the type; NaN is non-zero
        mm = np.zeros((96, 96), kind)
        mm[:, 40:] = 3
        assert np.array_equal(window.masked_spec((16, 16), mm).image_mask, (np.arange(96) >= 40)[None].repeat(96, 0).astype(np.uint8))
    # k_min = max(2, ceil(coverage * n^2)) in float64
    for n, cov, want in ((16, 0.25, 64), (16, 1e-9, 2), (16, 1.0, 256), (32, 0.3, 308), (64, 0.1, 410), (16, 0.0078125, 2), (16, 0.01, 3)):
        assert window.masked_spec((n, n), np.ones((n, n)), cov).k_min == want == ref.k_min(n, cov)
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), "x", None):
        with pytest.raises(ValueError, match=r"mask_coverage_min must"):
            window.masked_spec((32, 32), m, bad)
    with pytest.raises(ValueError, match=r"mask_coverage_min must"):
        window.masked_spec((32, 32), None, 0.0)
    with pytest.raises(ValueError, match=r"image_mask has shape \(96, 96\), the frames are \(96, 97\)"):
        window.masked_spec((32, 32), m, 0.25, (96, 97))
    with pytest.raises(ValueError, match="image_mask must be a 2-D array"):
        window.masked_spec((32, 32), np.ones((2, 96, 96)))
    with pytest.raises(ValueError, match="image_mask given twice"):
        window.masked_spec(spec, m)


def test_keyword_validation_and_the_new_refusals():
    a = np.zeros((3, 96, 96), np.uint8)
    m = np.ones((96, 96), bool)
    run = lambda ws=(16, 16), ov=(8, 8), sa=None, **kw: velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), ws, ov, sa or ws, 1.0, 1.0, **kw)
    with pytest.raises(ValueError, match=r"image_mask has shape \(96, 95\), the frames are \(96, 96\)"):
        run(image_mask=m[:, :95])
    with pytest.raises(ValueError, match=r"image_mask has shape"):
        frames.get_piv(a, 16, image_mask=m[:95])
    with pytest.raises(ValueError, match=r"image_mask has shape"):
        piv.piv_pairs_masked(a, (16, 16), (8, 8), m[:95])
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match=r"mask_coverage_min must lie in \(0, 1\]"):
            run(image_mask=m, mask_coverage_min=bad)
        with pytest.raises(ValueError, match=r"mask_coverage_min must lie in \(0, 1\]"):
            run(mask_coverage_min=bad)
        with pytest.raises(ValueError, match=r"mask_coverage_min must lie in \(0, 1\]"):
            piv.piv_pairs_masked(a, (16, 16), (8, 8), m, bad)
    for ws, ov in (((24, 24), (12, 12)), ((16, 32), (8, 8))):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            run(ws, ov, image_mask=m)
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            piv.piv_pairs_masked(a, ws, ov, m)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        frames.get_piv(a, 24, image_mask=m)
    with pytest.raises(NotImplementedError, match="image_mask together with ensemble_corr=True is not implemented"):
        run(image_mask=m, ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="image_mask together with coarse_passes is not implemented"):
        run(image_mask=m, coarse_passes=[64])
    with pytest.raises(NotImplementedError, match="image_mask together with deform_passes is not implemented"):
        run(image_mask=m, deform_passes=1)
    with pytest.raises(NotImplementedError, match="image_mask together with a search_area_size larger than the window is not implemented"):
        run((12, 12), (16, 16), (32, 32), image_mask=m)
    with pytest.raises(NotImplementedError, match="image_mask together with spectral_filter is not implemented"):
        run(image_mask=m, spectral_filter="spof")
    with pytest.raises(NotImplementedError, match="image_mask together with ensemble_window is not implemented"):
        run(image_mask=m, ensemble_corr=True, ensemble_window=2)
    with pytest.raises(NotImplementedError, match="image_mask together with coarse_passes"):
        window.masked_spec(window.multipass_spec((16, 16), (8, 8), [64]), m)
    with pytest.raises(NotImplementedError, match="image_mask together with deform_passes"):
        window.masked_spec(window.multipass_spec((16, 16), (8, 8), None, 1), m)
    with pytest.raises(NotImplementedError, match="image_mask together with spectral_filter"):
        window.masked_spec(window.filtered_spec((16, 16), "spof"), m)
    spec = window.masked_spec((16, 16), m)
    with pytest.raises(NotImplementedError, match="image_mask together with a search_area_size"):
        piv.piv_pairs(a, spec, (8, 8), search_area_size=(32, 32))
    with pytest.raises(NotImplementedError, match="image_mask together with ensemble_corr=True is not implemented"):
        piv.Ensemble((96, 96), spec, (8, 8))

    class Comm:
        rank, world = 0, 1

    with pytest.raises(NotImplementedError, match="image_mask with pyorc_amd.shard is not implemented"):
        shard.sharded_piv(lambda f0, f1: a[f0:f1], 2, spec, (8, 8), Comm())
    with pytest.raises(NotImplementedError, match="image_mask with pyorc_amd.shard is not implemented"):
        shard.sharded_piv_dev(object(), 2, spec, (8, 8), Comm())
    # image_mask=None is today's path: the existing refusals and their messages stay
    with pytest.raises(NotImplementedError, match="coarse_passes together with a search_area_size larger than the window is not implemented"):
        run((12, 12), (16, 16), (32, 32), coarse_passes=[64], image_mask=None)
    with pytest.raises(NotImplementedError, match="deform_passes with ensemble_corr=True is not implemented"):
        run(deform_passes=1, ensemble_corr=True, image_mask=None)
    with pytest.raises(NotImplementedError, match="spectral_filter together with coarse_passes is not implemented"):
        run(spectral_filter="spof", coarse_passes=[64], image_mask=None)


def test_no_mask_reaches_the_unchanged_path(monkeypatch):
    """image_mask=None: piv_pairs_masked hands over to piv_pairs with the plain window, get_ffpiv leaves the window argument alone."""
    seen = {}

    def fake_pairs(imgs, window_size, overlap, *args, **kw):
        seen["pairs"] = (type(window_size), tuple(window_size), tuple(overlap), args, kw)
        return "plain"

    monkeypatch.setattr(piv, "piv_pairs", fake_pairs)
    a = np.zeros((3, 96, 96), np.uint8)
    assert piv.piv_pairs_masked(a, (24, 24), (12, 12), None, 0.5, 0.1, True, 7) == "plain"
    assert seen["pairs"] == (tuple, (24, 24), (12, 12), (0.1, True, 7), {"out": None, "scale": None})

    def fake_spec(window_size, image_mask=None, *args, **kw):
        raise AssertionError("masked_spec must not run without a mask")

    monkeypatch.setattr(window, "masked_spec", fake_spec)

    class Stop(Exception):
        pass

    def fake_plan(n_frames, dim_size, window_size, *args, **kw):
        seen["plan"] = (type(window_size), tuple(window_size))
        raise Stop     # far enough: the window argument of the layers below is the plain one

    monkeypatch.setattr(velocimetry, "_plan_slices", fake_plan)
    with pytest.raises(Stop):
        velocimetry.get_ffpiv(a, np.arange(11), np.arange(11), np.ones(2), (16, 16), (8, 8), (16, 16), 1.0, 1.0, image_mask=None)
    assert seen["plan"] == (tuple, (16, 16))


def test_other_engines_do_not_know_the_keywords(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((3, 96, 96), np.uint8))
        with pytest.raises(TypeError, match="image_mask is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", image_mask=np.ones((96, 96), bool))
        with pytest.raises(TypeError, match="mask_coverage_min is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", mask_coverage_min=0.5)
        with pytest.raises(TypeError, match="image_mask / mask_coverage_min is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", image_mask=None, mask_coverage_min=0.5)
    finally:
        plugin.uninstall()


def test_new_symbols_in_header_signatures_and_exports(lib):
    names = ("lspiv_mask_supported", "lspiv_piv_masked_pairs_dev_at", "lspiv_piv_masked_pairs_at")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lspiv.h")).read()
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define LSPIV_ABI_VERSION 5" in header and lib.lspiv_abi_version() == 5


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    """Host-only paths of the C entry points: the window, the options, NULL and k_min are checked before a context is asked for."""
    buf = np.zeros(16, np.uint8)
    q = _lib.ptr(buf)
    call = lambda wy, wx, mask, k: lib.lspiv_piv_masked_pairs_dev_at(q, 0, 2, 64, 64, wy, wx, 0, 0, mask, k, -1.0, 0, q, None, None)
    assert call(24, 24, q, 2) == _lib.LSPIV_EUNSUPPORTED and call(16, 32, q, 2) == _lib.LSPIV_EUNSUPPORTED
    assert call(16, 16, None, 2) == _lib.LSPIV_EINVAL
    for k in (-1, 0, 1, 257):
        assert call(16, 16, q, k) == _lib.LSPIV_EINVAL
    host = lambda wy, wx, mask, k: lib.lspiv_piv_masked_pairs_at(q, 0, 2, 64, 64, wy, wx, 0, 0, mask, k, -1.0, 0, q, q, q, q, None)
    assert host(24, 24, q, 2) == _lib.LSPIV_EUNSUPPORTED and host(32, 32, None, 2) == _lib.LSPIV_EINVAL and host(32, 32, q, 1025) == _lib.LSPIV_EINVAL
    for opt, val in (("norm_clip", 0), ("signal_mode", 1)):
        old = _lib.get_option(opt)
        _lib.set_option(opt, val)
        try:
            assert call(16, 16, q, 2) == _lib.LSPIV_EUNSUPPORTED and host(16, 16, q, 2) == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, old)


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def test_planner_answers_as_the_plain_per_pair_launch_plus_the_mask_and_cuts_at_alignment_1(lib):
    for dim, T in (((160, 200), 10), ((1080, 1920), 201)):
        m = np.ones(dim, bool)
        for n in ref.MASK_WINDOWS:
            spec = window.masked_spec((n, n), m, 0.25, dim)
            for dtype in (np.uint8, np.float32, np.float64):
                for planes in (False, True):
                    assert window.required_memory(T, dim, spec, (n // 2, n // 2), dtype=dtype, with_planes=planes) == \
                        window.required_memory(T, dim, (n, n), (n // 2, n // 2), dtype=dtype, with_planes=planes) + dim[0] * dim[1]
            assert window.chunk_alignment(spec) == 1 and window.chunk_alignment(spec, dim, (n // 2, n // 2)) == 1
            align = window.chunk_alignment(spec, dim, (n // 2, n // 2))
            assert velocimetry.aligned_slices(12, 4, align) == [(0, 4), (3, 7), (6, 10), (9, 12)]       # chunks of 3 pairs: odd starts
            assert window.chunk_alignment((n, n), dim, (n // 2, n // 2)) > 1                            # (the plain window walks)
