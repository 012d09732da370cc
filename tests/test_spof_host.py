"""SPOF phase-filtered correlation, host side (CPU): what the reference (tests/spof_ref.py) gains on textured imagery, the properties of
its planes, the CPU checks of the inputs tests/test_gpu_spof.py relies on (fragile shares, masks clear of their thresholds), the keyword
validation, the plugin's TypeError for another engine, the new symbols and the planner."""
import os
import re

import numpy as np
import pytest

from pyorc_amd import _lib, frames, piv, shard, velocimetry, window
from tests import recipe_doubles as rd
from tests import spof_ref as ref


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_filter_keeps_the_tracers_where_a_static_texture_outweighs_them_per_pair():
    """160 x 200 uint8, uniform shift (3.3, -2.4) px, texture amplitude 80, density 0.02, three pairs, 32 @ 16; share of windows within
    0.5 px of the truth.  Measured: NCC 0.468, SPOF 0.983."""
    ncc, spof = ref.textured_ref("pairs", False), ref.textured_ref("pairs", True)
    s_ncc, s_spof = ref.within_half_px(ncc["u"], ncc["v"]), ref.within_half_px(spof["u"], spof["v"])
    print("NCC", s_ncc, "SPOF", s_spof, "median peak", np.nanmedian(ncc["corr"]), np.nanmedian(spof["corr"]))
    assert s_ncc <= 0.6 and s_spof >= 0.9


def test_filter_keeps_the_tracers_in_the_ensemble_where_averaging_reinforces_the_texture():
    """The same at density 0.012 over six pairs, ensembles at 32 @ 16 (masks TEX_KW).  Measured: NCC 0.313, SPOF 0.960."""
    ncc, spof = ref.textured_ref("ensemble", False), ref.textured_ref("ensemble", True)
    s_ncc, s_spof = ref.within_half_px(ncc["u"], ncc["v"]), ref.within_half_px(spof["u"], spof["v"])
    print("NCC", s_ncc, "SPOF", s_spof, "counts", np.bincount(spof["count"].astype(int)))
    assert s_ncc <= 0.45 and s_spof >= 0.9


def test_planes_stay_inside_0_1_and_identical_windows_peak_at_the_centre():
    rng = np.random.default_rng(3)
    for n in ref.SPOF_WINDOWS:
        a = rng.integers(0, 256, (5, n, n)).astype(np.float64)
        same = ref.plane(a, a)
        assert same.min() >= 0.0 and same.max() <= 1.0
        assert (same.reshape(5, -1).argmax(axis=1) == (n // 2) * n + n // 2).all()
        other = ref.plane(a, np.roll(a, (2, -3), axis=(-2, -1)))
        assert (other.reshape(5, -1).argmax(axis=1) == (n // 2 + 2) * n + n // 2 - 3).all()
        assert not ref.plane(np.full((1, n, n), 7.0), a[:1]).any()              # a zero-variance window: an exactly zero plane
    for case in list(ref.PASS_CASES) + list(ref.GRID_CASES):
        pl = ref.pass_ref(case)["planes"]
        assert np.nanmin(pl) >= 0.0 and np.nanmax(pl) <= 1.0
        # the lower clip does real work: a filtered plane has negative lobes (an NCC plane of non-negative windows has none) -- every
        # tenth sample at least is clipped away here
        assert (pl == 0.0).mean() > 0.1


def test_reference_is_nan_below_the_signal_threshold_and_on_non_finite_samples():
    for case in ref.PASS_CASES:
        r = ref.signal_ref(case)
        nan = np.isnan(r["corr"])
        assert 0.1 < nan.mean() < 0.6 and np.array_equal(nan, np.isnan(r["s2n"])) and np.array_equal(nan.reshape(nan.shape[0], -1), np.isnan(r["planes"]).all(axis=(-2, -1)))
    n, ov, _ = ref.PASS_CASES[16]
    a = ref.deform_ref.pass_stack(16, np.float32).copy()
    a[1, 5, 5] = np.nan
    r = ref.piv(a, n, ov)
    assert np.isnan(r["corr"][0, 0, 0]) and np.isnan(r["corr"][1, 0, 0]) and np.isfinite(r["corr"][2]).all()


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------
def test_parity_inputs_have_no_fragile_windows():
    """A window is fragile when a second sample lies within 1e-4 (relative) of the plane maximum or a neighbour of an interior peak
    lies below 1e-5.  Measured: 0 on all nine pass_stack cases and both grid cases; the GPU tests may leave out at most 1 %."""
    for case in ref.PASS_CASES:
        for dtype in ref.PASS_DTYPES:
            assert ref.pass_ref(case, dtype)["fragile"].mean() <= 0.01, (case, dtype)
        assert ref.signal_ref(case)["fragile"].mean() <= 0.01
        for dtype in ref.PASS_DTYPES:
            assert ref.ens_ref(case, dtype)["fragile"].mean() <= 0.01
    for case in ref.GRID_CASES:
        assert ref.pass_ref(case)["fragile"].mean() <= 0.01
    r = ref.ens_signal_ref()
    assert r["fragile"].mean() <= 0.01 and 0.1 < np.isnan(r["u"]).mean() < 0.6 and r["count"].min() == 0 and r["count"].max() == ref.ENS_T - 1
    finite = np.isfinite(r["pair_corr"])
    assert np.abs(r["pair_corr"][finite] / ref.ens_kw(32)["corr_min"] - 1).min() > 1e-3
    for name in ref.TEXTURED:
        assert ref.textured_ref(name)["fragile"].mean() <= 0.01


def test_ensemble_parity_masks_bite_and_sit_clear_of_every_pair():
    """The masks of the ensemble parity inputs drop some planes of some windows (the sums are no plain sums), and no per-pair value lies
    within 1e-3 (relative) of its threshold: float32 and float64 take the same decisions."""
    for case in ref.PASS_CASES:
        r = ref.ens_ref(case)
        kw = ref.ens_kw(case)
        counts = r["count"]
        assert counts.min() < ref.ENS_T - 1 and counts.max() == ref.ENS_T - 1, (case, np.bincount(counts.astype(int)))
        assert np.abs(r["pair_corr"] / kw["corr_min"] - 1).min() > 1e-3 and np.abs(r["pair_s2n"] / kw["s2n_min"] - 1).min() > 1e-3


# ---- validation -----------------------------------------------------------------------------------------------------------------------
def test_filter_names_and_windows(lib):
    assert window.spectral_filter_spec(None) is None and window.spectral_filter_spec("none") is None
    assert window.spectral_filter_spec("spof") == "spof"
    for bad in ("SPOF", "phase", 1, True, ""):
        with pytest.raises(ValueError, match=r"\('none', 'spof'\)"):
            window.spectral_filter_spec(bad)
    for n in (16, 32, 64):
        assert window.spectral_filter_supported((n, n)) == (n, n) and window.spectral_filter_supported(n) == (n, n)
    for ws in (24, (24, 24), (16, 32), (128, 128), (8, 8)):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            window.spectral_filter_supported(ws)
    assert [lib.lspiv_spof_supported(n, n) for n in (8, 16, 24, 32, 48, 64, 128)] == [0, 1, 0, 1, 0, 1, 0]
    assert lib.lspiv_spof_supported(16, 32) == 0 and lib.lspiv_abi_version() == 5
    spec = window.filtered_spec((32, 32), "spof")
    assert isinstance(spec, window.FilteredWindow) and tuple(spec) == (32, 32) and spec.spectral_filter == "spof"
    assert window.filtered_spec(spec) is spec and window.filtered_spec(spec, "spof") is spec
    assert window.filtered_spec((32, 32), None) == (32, 32) and not isinstance(window.filtered_spec((32, 32), "none"), window.FilteredWindow)
    assert window.chunk_alignment(spec) == 1 and window.chunk_alignment(spec, (160, 200), (16, 16)) == 1


def test_keyword_validation():
    a = np.zeros((3, 96, 96), np.uint8)
    run = lambda ws=(16, 16), ov=(8, 8), sa=None, **kw: velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), ws, ov, sa or ws, 1.0, 1.0, **kw)
    with pytest.raises(ValueError, match=r"\('none', 'spof'\)"):
        run(spectral_filter="phase")
    with pytest.raises(ValueError, match=r"\('none', 'spof'\)"):
        frames.get_piv(a, 16, spectral_filter="SPOF")
    with pytest.raises(ValueError, match=r"\('none', 'spof'\)"):
        piv.piv_pairs_filtered(a, (16, 16), (8, 8), "phase")
    for ws, ov in (((24, 24), (12, 12)), ((16, 32), (8, 8))):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            run(ws, ov, spectral_filter="spof")
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            piv.piv_pairs_filtered(a, ws, ov)
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            run(ws, ov, spectral_filter="spof", ensemble_corr=True)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        frames.get_piv(a, 24, spectral_filter="spof")
    for ens in (False, True):
        with pytest.raises(NotImplementedError, match="spectral_filter together with coarse_passes"):
            run(spectral_filter="spof", coarse_passes=[64], ensemble_corr=ens)
        with pytest.raises(NotImplementedError, match="spectral_filter together with a search_area_size"):
            run((12, 12), (16, 16), (32, 32), spectral_filter="spof", ensemble_corr=ens)
    with pytest.raises(NotImplementedError, match="spectral_filter together with deform_passes"):
        run(spectral_filter="spof", deform_passes=1)
    with pytest.raises(NotImplementedError, match="spectral_filter together with ensemble_window"):
        run(spectral_filter="spof", ensemble_corr=True, ensemble_window=2)
    with pytest.raises(NotImplementedError, match="spectral_filter together with coarse_passes"):
        window.filtered_spec(window.multipass_spec((16, 16), (8, 8), [64]), "spof")
    with pytest.raises(NotImplementedError, match="spectral_filter together with deform_passes"):
        window.filtered_spec(window.multipass_spec((16, 16), (8, 8), None, 1), "spof")
    with pytest.raises(NotImplementedError, match="spectral_filter together with a search_area_size"):
        piv.piv_pairs(a, window.filtered_spec((32, 32), "spof"), (16, 16), search_area_size=(64, 64))

    class Comm:
        rank, world = 0, 1

    spec = window.filtered_spec((16, 16), "spof")
    with pytest.raises(NotImplementedError, match="spectral_filter with pyorc_amd.shard is not implemented"):
        shard.sharded_piv(lambda f0, f1: a[f0:f1], 2, spec, (8, 8), Comm())
    with pytest.raises(NotImplementedError, match="spectral_filter with pyorc_amd.shard is not implemented"):
        shard.sharded_piv_dev(object(), 2, spec, (8, 8), Comm())
    # "none" and None are today's path: the existing refusals and their messages stay
    with pytest.raises(NotImplementedError, match="coarse_passes together with a search_area_size larger than the window is not implemented"):
        run((12, 12), (16, 16), (32, 32), coarse_passes=[64], spectral_filter="none")
    with pytest.raises(NotImplementedError, match="deform_passes with ensemble_corr=True is not implemented"):
        run(deform_passes=1, ensemble_corr=True, spectral_filter=None)


def test_other_engines_do_not_know_the_keyword(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((3, 96, 96), np.uint8))
        for value in ("spof", "none"):
            with pytest.raises(TypeError, match="spectral_filter is a keyword of engine='hip' only"):
                acc.get_piv(16, engine="numba", spectral_filter=value)
    finally:
        plugin.uninstall()


def test_new_symbols_in_header_signatures_and_exports(lib):
    names = ("lspiv_spof_supported", "lspiv_piv_spof_pairs_dev_at", "lspiv_piv_spof_pairs_at", "lspiv_ensemble_set_spectral_filter",
             "lspiv_ensemble_get_spectral_filter")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lspiv.h")).read()
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define LSPIV_ABI_VERSION 5" in header and lib.lspiv_abi_version() == 5
    assert re.search(r"#define LSPIV_FILTER_SPOF 1\b", header) and window.SPECTRAL_FILTERS.index("spof") == 1


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def test_planner_answers_as_for_the_plain_per_pair_launch(lib):
    for dim, T in (((160, 200), 10), ((1080, 1920), 201)):
        for n in ref.SPOF_WINDOWS:
            spec = window.filtered_spec((n, n), "spof")
            for dtype in (np.uint8, np.float32, np.float64):
                for planes in (False, True):
                    assert window.required_memory(T, dim, spec, (n // 2, n // 2), dtype=dtype, with_planes=planes) == \
                        window.required_memory(T, dim, (n, n), (n // 2, n // 2), dtype=dtype, with_planes=planes)
