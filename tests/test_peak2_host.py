"""Second correlation peak, host side (CPU): the reference (tests/peak2_ref.py) on hand-made planes, the share of fragile windows of every
input tests/test_gpu_peak2.py uses, the reference's dependence on the exclusion radius, the keyword validation and the new refusals,
``peak_ratio=False`` reaching the unchanged path, the plugin's TypeError for another engine, the new symbols and the planner."""
import os
import re

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, shard, velocimetry, window
from tests import deform_ref
from tests import peak2_ref as ref
from tests import recipe_doubles as rd


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the reference on hand-made planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.HAND_SHAPES)
def test_reference_on_hand_made_planes(shape):
    wy, wx = shape
    seen = set()
    for name, pl, expected in ref.hand_planes(wy, wx):
        r = ref.plane_result(pl, 2)
        if expected == "nan":
            assert all(np.isnan(r[k]) for k in ("u2", "v2", "corr2", "ratio")), name
        elif expected is None:
            assert not r["found"] and r["corr2"] == 0.0 and r["ratio"] == np.inf and np.isnan(r["u2"]) and np.isnan(r["v2"]), name
        else:
            assert (r["found"], r["i2"], r["j2"]) == (True, *expected), name
            assert r["corr2"] == float(pl[expected]) and r["ratio"] == float(pl.max()) / float(pl[expected]), name
        seen.add(name)
    assert {"single delta", "primary in a corner", "two equal second peaks", "only the flank of the primary outside the box"} <= seen


def test_a_single_delta_has_no_candidate_and_the_flank_is_none():
    pl = np.zeros((32, 32))
    pl[16, 16] = 1.0
    assert ref.second_peak(pl, 2) == (False, -1, -1, 0.0, 0.0)
    # a sample just outside the box on the flank of the primary: above the floor, but its neighbour inside the box is higher
    name, flank, _ = [h for h in ref.hand_planes(32, 32) if h[0].startswith("only the flank")][0]
    assert flank[16, 19] > 0.1 and not ref.candidates(flank, 2)[16, 19] and not ref.candidates(flank, 2).any()
    # OpenPIV's reading, the maximum outside the box, would have taken exactly that sample
    outside = flank.astype(np.float64).copy()
    outside[14:19, 14:19] = 0
    assert outside.max() == flank[16, 19]


def test_primary_in_a_corner_clips_the_box_without_wrapping():
    pl = np.zeros((16, 16))
    pl[0, 0] = 1.0
    pl[15, 15] = 0.5      # a wrapping box of r = 2 would swallow it
    pl[2, 2] = 0.4        # inside the clipped box
    assert ref.second_peak(pl, 2)[:4] == (True, 15, 15, 0.5)
    assert ref.second_peak(pl, 1)[:4] == (True, 15, 15, 0.5) and ref.candidates(pl, 1)[2, 2] and not ref.candidates(pl, 2)[2, 2]


def test_second_peak_on_the_border_follows_the_three_border_modes():
    name, pl, (i2, j2) = [h for h in ref.hand_planes(32, 32) if h[0] == "second peak on the top border"][0]
    assert i2 == 0
    want = {0: (np.nan, np.nan), 1: (0.0, 0.0), 2: (float(j2 - 16), float(i2 - 16))}
    for mode in (0, 1, 2):
        with po.semantics(border_peak=mode):
            r = ref.plane_result(pl, 2)
        assert np.array_equal([r["u2"], r["v2"]], want[mode], equal_nan=True) and r["corr2"] == float(pl[i2, j2])
    with po.semantics(border_peak=2, v_sign=1):
        assert ref.plane_result(pl, 2)["v2"] == 16.0
    # an interior second peak is the primary's own fit: the oracle's peak_position on a plane that holds nothing else
    name, pl, (i2, j2) = [h for h in ref.hand_planes(32, 32) if h[0] == "primary in a corner"][0]
    alone = pl.astype(np.float64).copy()
    alone[:4, :4] = 0
    pi, pj = po.peak_position(alone)
    r = ref.plane_result(pl, 2)
    assert (r["v2"], r["u2"]) == (pi - 16, pj - 16)


def test_equal_second_peaks_go_to_the_first_in_row_major_order():
    pl = np.zeros((16, 16))
    pl[8, 8] = 1.0
    pl[12, 2] = pl[3, 13] = pl[3, 5] = 0.5
    assert ref.second_peak(pl, 2)[:3] == (True, 3, 5)
    assert ref.fragile_plane(pl, 2)       # ... and such a window is left out of the gates: the runner-up equals the second peak


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------------
FRAGILE = {16: (1, 75), 32: (2, 105), 64: (0, 60)}


def _capped(res):
    fr, kept = ref.fragile_share(res)
    assert kept > 0 and fr <= 0.05 * kept, (fr, kept)
    return fr, kept


@pytest.mark.parametrize("case", sorted(ref.PASS_CASES))
def test_fragile_share_of_the_parity_and_signal_inputs(case):
    assert _capped(ref.pass_ref(case, np.uint8)) == FRAGILE[case]
    for dtype in (np.float32, np.float64):
        print(case, np.dtype(dtype).name, _capped(ref.pass_ref(case, dtype)))
    s = ref.signal_ref(case)
    fr, kept = _capped(s)
    dropped = np.isnan(s["corr"])
    print(case, "signal threshold: fragile", fr, "of", kept, "dropped", int(dropped.sum()))
    assert dropped.any() and kept and all(np.isnan(s[k][dropped]).all() for k in ("u2", "v2", "corr2", "ratio"))
    assert s["found"][~dropped].any()


@pytest.mark.parametrize("case", (16, 32))
def test_fragile_share_of_the_radius_inputs_and_the_radius_matters(case):
    res = {r: ref.pass_ref(case, np.uint8, r) for r in ref.RADII}
    for r in ref.RADII:
        _capped(res[r])
    differ = (res[1]["found"] != res[4]["found"]) | (res[1]["i2"] != res[4]["i2"]) | (res[1]["j2"] != res[4]["j2"])
    print(case, "r = 1 and r = 4 differ in", int(differ.sum()), "of", differ.size)
    assert differ.sum() >= 1
    if case == 16:
        assert int(differ.sum()) == 10 and differ.size == 75


@pytest.mark.parametrize("seed", ref.SPARSE_SEEDS)
def test_fragile_share_of_the_sparse_scene_and_what_the_reference_gains(seed):
    r = ref.sparse_ref(seed)
    _capped(r)
    a_ratio, a_s2n = ref.auc_pair(r["u"], r["v"], r["ratio"], r["s2n"])
    print(seed, "AUC of the peak ratio %.3f, of s2n %.3f" % (a_ratio, a_s2n))
    assert a_ratio - a_s2n >= 0.1      # (+0.123 and +0.119: the GPU test asks +0.05 of the float32 planes)


def test_fit_motion_bounds_the_gate_on_the_runner_up_vector():
    """B of the GPU parity test on the reference's own planes for a plane deviation of the full gate: millipixels on the flat second peaks,
    which is why they get no fixed 1e-4 gate."""
    worst = 0.0
    for case in sorted(ref.PASS_CASES):
        r = ref.pass_ref(case, np.uint8)
        pl = r["planes"].reshape(r["corr"].shape + r["planes"].shape[-2:])
        for idx in zip(*np.nonzero(r["found"] & ~r["fragile2"])):
            worst = max(worst, ref.fit_motion(pl[idx], int(r["i2"][idx]), int(r["j2"][idx]), ref.PLANE_GATE))
    print("largest B at d = 2e-6: %.2e px" % worst)
    assert 1e-5 < worst < 5e-3


# ---- argument checking ------------------------------------------------------------------------------------------------------------------------
def test_windows_and_radius(lib):
    for n in (16, 32, 64):
        assert window.peak2_supported((n, n)) == (n, n) and window.peak2_supported(n) == (n, n)
        spec = window.peak_ratio_spec((n, n), True, n // 4)
        assert isinstance(spec, window.PeakRatioWindow) and tuple(spec) == (n, n) and spec.peak_exclusion == n // 4
        assert window.peak_ratio_spec(spec, True, 1) is spec
        for bad in (0, -1, n // 4 + 1, 1.5, True, None, "2"):
            with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. %d" % (n // 4)):
                window.peak_ratio_spec((n, n), True, bad)
    assert window.peak_ratio_spec((24, 24), False, 99) == (24, 24)          # peak_ratio=False: nothing is looked at
    assert window.PeakRatioWindow((32, 32)).peak_exclusion == 2
    for ws in (24, (24, 24), (16, 32), (128, 128), (8, 8)):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            window.peak_ratio_spec(ws, True)
    assert [lib.lspiv_peak2_supported(n, n) for n in (8, 16, 24, 32, 48, 64, 128)] == [0, 1, 0, 1, 0, 1, 0]
    assert lib.lspiv_peak2_supported(16, 32) == 0 and lib.lspiv_abi_version() == 5


def test_keyword_validation_and_the_new_refusals():
    a = np.zeros((3, 96, 96), np.uint8)
    m = np.ones((96, 96), bool)
    run = lambda ws=(16, 16), ov=(8, 8), sa=None, **kw: velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), ws, ov, sa or ws, 1.0, 1.0, **kw)
    for ws, ov in (((24, 24), (12, 12)), ((16, 32), (8, 8))):
        with pytest.raises(ValueError, match=r"not supported with peak_ratio.*\(16, 32, 64\)"):
            run(ws, ov, peak_ratio=True)
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            piv.piv_pairs_peak2(a, ws, ov)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        frames.get_piv(a, 24, peak_ratio=True)
    for bad in (0, 5, 2.0):
        with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. 4"):
            run(peak_ratio=True, peak_exclusion=bad)
        with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. 4"):
            piv.piv_pairs_peak2(a, (16, 16), (8, 8), bad)
        with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. 4"):
            frames.get_piv(a, 16, peak_ratio=True, peak_exclusion=bad)
    with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. 6"):
        piv.second_peak(np.zeros((1, 1, 24, 40), np.float32), 7)
    with pytest.raises(ValueError, match=r"planes must have shape"):
        piv.second_peak(np.zeros((24, 40), np.float32))
    with pytest.raises(ValueError, match=r"a side outside 4 \.\. 4096"):
        piv.second_peak(np.zeros((1, 1, 3, 40), np.float32), 1)
    with pytest.raises(NotImplementedError, match="peak_ratio together with image_mask is not implemented.*piv.second_peak"):
        run(peak_ratio=True, image_mask=m)
    with pytest.raises(NotImplementedError, match="peak_ratio together with spectral_filter is not implemented.*piv.second_peak"):
        run(peak_ratio=True, spectral_filter="spof")
    with pytest.raises(NotImplementedError, match="peak_ratio together with coarse_passes is not implemented.*piv.second_peak"):
        run(peak_ratio=True, coarse_passes=[64])
    with pytest.raises(NotImplementedError, match="peak_ratio together with deform_passes is not implemented.*piv.second_peak"):
        run(peak_ratio=True, deform_passes=1)
    with pytest.raises(NotImplementedError, match="peak_ratio together with a search_area_size larger than the window is not implemented.*piv.second_peak"):
        run((12, 12), (16, 16), (32, 32), peak_ratio=True)
    with pytest.raises(NotImplementedError, match="peak_ratio together with ensemble_corr=True is not implemented.*piv.second_peak"):
        run(peak_ratio=True, ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="peak_ratio together with ensemble_corr=True is not implemented"):
        run(peak_ratio=True, ensemble_corr=True, ensemble_window=2)
    spec = window.peak_ratio_spec((16, 16), True)
    with pytest.raises(NotImplementedError, match="peak_ratio together with ensemble_corr=True is not implemented"):
        piv.Ensemble((96, 96), spec, (8, 8))
    with pytest.raises(NotImplementedError, match="peak_ratio together with a search_area_size"):
        piv.piv_pairs(a, spec, (8, 8), search_area_size=(32, 32))
    for other, keyword in ((window.masked_spec((16, 16), m), "image_mask"), (window.filtered_spec((16, 16), "spof"), "spectral_filter"),
                           (window.multipass_spec((16, 16), (8, 8), [64]), "coarse_passes"),
                           (window.multipass_spec((16, 16), (8, 8), None, 1), "deform_passes")):
        with pytest.raises(NotImplementedError, match="peak_ratio together with " + keyword):
            window.peak_ratio_spec(other, True)
        with pytest.raises(NotImplementedError, match="peak_ratio together with " + keyword):
            piv.piv_pairs_peak2(a, other, (8, 8))

    class Comm:
        rank, world = 0, 1

    with pytest.raises(NotImplementedError, match="peak_ratio with pyorc_amd.shard is not implemented"):
        shard.sharded_piv(lambda f0, f1: a[f0:f1], 2, spec, (8, 8), Comm())
    with pytest.raises(NotImplementedError, match="peak_ratio with pyorc_amd.shard is not implemented"):
        shard.sharded_piv_dev(object(), 2, spec, (8, 8), Comm())
    # peak_ratio=False is today's path: the existing refusals and their messages stay
    with pytest.raises(NotImplementedError, match="image_mask together with spectral_filter is not implemented"):
        run(image_mask=m, spectral_filter="spof", peak_ratio=False)
    with pytest.raises(NotImplementedError, match="deform_passes with ensemble_corr=True is not implemented"):
        run(deform_passes=1, ensemble_corr=True, peak_ratio=False, peak_exclusion=99)


def test_peak_ratio_false_reaches_the_unchanged_path(monkeypatch):
    """peak_ratio=False: get_ffpiv leaves the window argument alone whatever peak_exclusion says, and no second-peak spec is formed."""
    seen = {}

    def fake_spec(window_size, *args, **kw):
        raise AssertionError("peak_ratio_spec must not run without peak_ratio")

    monkeypatch.setattr(window, "peak_ratio_spec", fake_spec)

    class Stop(Exception):
        pass

    def fake_plan(n_frames, dim_size, window_size, *args, **kw):
        seen["plan"] = (type(window_size), tuple(window_size))
        raise Stop     # far enough: the window argument of the layers below is the plain one

    monkeypatch.setattr(velocimetry, "_plan_slices", fake_plan)
    a = np.zeros((3, 96, 96), np.uint8)
    for kw in ({}, {"peak_ratio": False}, {"peak_ratio": False, "peak_exclusion": 99}):
        seen.clear()
        with pytest.raises(Stop):
            velocimetry.get_ffpiv(a, np.arange(11), np.arange(11), np.ones(2), (16, 16), (8, 8), (16, 16), 1.0, 1.0, **kw)
        assert seen["plan"] == (tuple, (16, 16))
    # the sink of a plain window allocates today's four variables and nothing else
    launch, close, result = velocimetry._timestep_sink(2, 1, np.arange(11), np.arange(11), np.ones(2), 1.0, 1.0, (16, 16), (8, 8), None)
    assert [c.cell_contents for c in launch.__closure__ if isinstance(c.cell_contents, dict)][0].keys() == {"s2n", "corr", "v_x", "v_y"}


def test_peak_ratio_true_hands_the_spec_down(monkeypatch):
    seen = {}

    class Stop(Exception):
        pass

    def fake_plan(n_frames, dim_size, window_size, *args, **kw):
        seen["plan"] = (type(window_size), tuple(window_size), window_size.peak_exclusion)
        raise Stop

    monkeypatch.setattr(velocimetry, "_plan_slices", fake_plan)
    a = np.zeros((3, 96, 96), np.uint8)
    with pytest.raises(Stop):
        velocimetry.get_ffpiv(a, np.arange(11), np.arange(11), np.ones(2), (16, 16), (8, 8), (16, 16), 1.0, 1.0, peak_ratio=True, peak_exclusion=3)
    assert seen["plan"] == (window.PeakRatioWindow, (16, 16), 3)

    def fake_peak2(imgs, spec, overlap, r, *args, **kw):
        seen["pairs"] = (type(spec), tuple(spec), tuple(overlap), r, args, kw)
        return "second"

    monkeypatch.setattr(piv, "piv_pairs_peak2", fake_peak2)
    assert piv.piv_pairs(a, window.PeakRatioWindow((32, 32), 4), (16, 16), 0.2, True, 5) == "second"
    assert seen["pairs"] == (window.PeakRatioWindow, (32, 32), (16, 16), 4, (0.2, True, 5), {"out": None, "scale": None})


def test_other_engines_do_not_know_the_keywords(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((3, 96, 96), np.uint8))
        with pytest.raises(TypeError, match="peak_ratio is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", peak_ratio=True)
        with pytest.raises(TypeError, match="peak_exclusion is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", peak_exclusion=2)
        with pytest.raises(TypeError, match="peak_ratio / peak_exclusion is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", peak_ratio=False, peak_exclusion=2)
    finally:
        plugin.uninstall()


NAMES = ("lspiv_peak2_supported", "lspiv_piv_peak2_pairs_dev_at", "lspiv_piv_peak2_pairs_at", "lspiv_second_peak_dev", "lspiv_second_peak")


def test_new_symbols_in_header_signatures_and_exports(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lspiv.h")).read()
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name       # as many arguments on both sides
    assert "#define LSPIV_ABI_VERSION 5" in header and lib.lspiv_abi_version() == 5


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    """Host-only paths of the C entry points: the window, the options, NULL, the radius and the alignment are checked before a context
    is asked for."""
    buf = np.zeros(64, np.uint8)
    q = _lib.ptr(buf)
    assert buf.ctypes.data % 16 == 0
    odd = _lib.ptr(buf[4:])
    call = lambda wy, wx, r, out=q: lib.lspiv_piv_peak2_pairs_dev_at(q, 0, 2, 64, 64, wy, wx, 0, 0, -1.0, 0, r, q, out, None, None)
    host = lambda wy, wx, r, out=q: lib.lspiv_piv_peak2_pairs_at(q, 0, 2, 64, 64, wy, wx, 0, 0, -1.0, 0, r, q, q, q, q, out, None)
    for f in (call, host):
        assert f(24, 24, 2) == _lib.LSPIV_EUNSUPPORTED and f(16, 32, 2) == _lib.LSPIV_EUNSUPPORTED
        assert f(16, 16, 2, None) == _lib.LSPIV_EINVAL
        for n in (16, 32, 64):
            for r in (-1, 0, n // 4 + 1):
                assert f(n, n, r) == _lib.LSPIV_EINVAL
    assert call(16, 16, 2, odd) == _lib.LSPIV_EINVAL
    planes = lambda n, wy, wx, r, src=q, out=q: lib.lspiv_second_peak_dev(src, n, wy, wx, r, out, None)
    assert planes(1, 16, 16, 2, None) == _lib.LSPIV_EINVAL and planes(1, 16, 16, 2, q, None) == _lib.LSPIV_EINVAL
    assert planes(-1, 16, 16, 2) == _lib.LSPIV_EINVAL and planes(1 << 31, 16, 16, 2) == _lib.LSPIV_EINVAL
    assert planes(1, 3, 16, 1) == _lib.LSPIV_EINVAL and planes(1, 16, 4097, 1) == _lib.LSPIV_EINVAL
    assert planes(1, 24, 40, 7) == _lib.LSPIV_EINVAL and planes(1, 24, 40, 0) == _lib.LSPIV_EINVAL
    hp = lambda P, n_win, wy, wx, r: lib.lspiv_second_peak(q, P, n_win, wy, wx, r, q)
    assert hp(1, 1, 16, 16, 5) == _lib.LSPIV_EINVAL and hp(-1, 1, 16, 16, 2) == _lib.LSPIV_EINVAL and hp(1 << 20, 1 << 20, 16, 16, 2) == _lib.LSPIV_EINVAL
    assert hp(0, 5, 16, 16, 2) == _lib.LSPIV_OK        # nothing to do
    for opt, val in (("norm_clip", 0), ("signal_mode", 1)):
        old = _lib.get_option(opt)
        _lib.set_option(opt, val)
        try:
            assert call(16, 16, 2) == _lib.LSPIV_EUNSUPPORTED and host(16, 16, 2) == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, old)


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def test_planner_answers_as_the_plain_per_pair_launch_plus_the_block_and_cuts_at_alignment_1(lib):
    for dim, T in (((160, 200), 10), ((1080, 1920), 201)):
        for n in ref.PEAK2_WINDOWS:
            spec = window.peak_ratio_spec((n, n), True)
            rows, cols = window.get_array_shape(dim, (n, n), (n // 2, n // 2))
            for dtype in (np.uint8, np.float32, np.float64):
                for planes in (False, True):
                    assert window.required_memory(T, dim, spec, (n // 2, n // 2), dtype=dtype, with_planes=planes) == \
                        window.required_memory(T, dim, (n, n), (n // 2, n // 2), dtype=dtype, with_planes=planes) + 16 * (T - 1) * rows * cols
            assert window.chunk_alignment(spec) == 1 and window.chunk_alignment(spec, dim, (n // 2, n // 2)) == 1
            assert velocimetry.aligned_slices(12, 4, window.chunk_alignment(spec, dim, (n // 2, n // 2))) == [(0, 4), (3, 7), (6, 10), (9, 12)]
            assert window.chunk_alignment((n, n), dim, (n // 2, n // 2)) > 1                            # (the plain window walks)


def test_ensemble_docstring_is_a_docstring():
    assert piv.Ensemble.__init__.__doc__ and "sliding=(M, s)" in piv.Ensemble.__init__.__doc__
