"""Vector validation without a GPU: what tests/validate_ref.py -- the float32 numpy restatement of the rule --
says about the shared inputs (every class the GPU tests rely on occurs in them), what the median test gains on the sparse noisy scene of
tests/peak2_ref.py, the refusals of the Python layer, and the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

from pyorc_amd import _lib, frames, piv, shard, validate, velocimetry
from tests import peak2_ref
from tests import recipe_doubles as rd
from tests import validate_ref as ref


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _histories(replace, min_neighbours=3):
    out = {}
    for grid in ref.GRIDS:
        u, v, p2 = ref.field(grid)
        h = []
        ref.median_test(u, v, p2, replace=replace, iterations=3, min_neighbours=min_neighbours, history=h)
        out[grid] = h
    return out


@pytest.mark.parametrize("replace", ["nan", "median"])
def test_inputs_hold_every_flag_class_neighbour_count_and_judged_state(replace):
    hist = _histories(replace)
    flags = np.concatenate([h[-1][2].ravel() for h in hist.values()])
    wanted = {0, 2, 1 if replace == "nan" else 3}
    assert set(np.unique(flags).tolist()) == wanted
    counts = np.concatenate([h[0][3].ravel() for h in hist.values()])
    assert set(np.unique(counts).tolist()) == set(range(9))
    judged = unjudged_finite = unjudged_nan = 0
    for grid, h in hist.items():
        u, v, _ = ref.field(grid)
        fin = np.isfinite(u) & np.isfinite(v)
        judged += int((fin & (h[0][3] >= 3)).sum())
        unjudged_finite += int((fin & (h[0][3] < 3)).sum())
        unjudged_nan += int((~fin).sum())
        # an unjudged centre keeps value and flag
        keep = ~(fin & (h[0][3] >= 3))
        assert ref.same(h[0][0][keep], u[keep]) and ref.same(h[0][1][keep], v[keep]) and not h[0][2][keep].any()
    assert judged and unjudged_finite and unjudged_nan
    # the inputs hold NaN and both infinities, and a runner-up of every kind on the outliers
    big = ref.field(ref.GRIDS[-1])
    assert np.isnan(big[0]).any() and np.isnan(big[1]).any() and np.isposinf(big[0]).any() and np.isneginf(big[0]).any()
    assert np.isnan(big[2][..., 0]).any()


def test_a_substituted_vector_is_judged_again_and_falls():
    """Iteration 2 re-judges flag-2 vectors: somewhere one of them falls to action 2 / 3, and the flag is the last action taken."""
    fell = {"nan": 0, "median": 0}
    for replace in fell:
        for h in _histories(replace).values():
            was2 = h[0][2] == 2
            fell[replace] += int((was2 & (h[1][2] == (1 if replace == "nan" else 3))).sum())
            # flag 2 is only ever given to a vector that was still the primary one
            assert not ((h[1][2] == 2) & (h[0][2] != 2) & (h[0][2] != 0)).any()
    print("flag-2 vectors that fell in iteration 2:", fell)
    assert fell["nan"] + fell["median"] > 0


def test_min_neighbours_moves_the_judged_set():
    u, v, p2 = ref.field((2, 5, 7))
    f1, f3, f8 = (ref.median_test(u, v, p2, min_neighbours=m)[2] for m in (1, 3, 8))
    assert (f8 != 0).sum() < (f3 != 0).sum() <= (f1 != 0).sum()


def test_wrap_field_has_no_flags_and_a_wrap_would_flip_some():
    u, v = ref.wrap_field()
    T, R, C = u.shape
    for kw in (dict(), dict(replace="median", iterations=3), dict(min_neighbours=1)):
        assert not ref.median_test(u, v, **kw)[2].any(), kw
    assert np.allclose(u[:, :-1, -1] - u[:, 1:, 0], 10.0) and np.allclose(v[:-1, -1] - v[1:, 0], 10.0)
    # time steps glued together: the last row of a step becomes the neighbour of the first row of the next
    assert ref.median_test(u.reshape(1, T * R, C), v.reshape(1, T * R, C))[2].any()
    # rows glued together: a column on either side that holds the end of the row above / the start of the row below
    uu = np.concatenate([u[:, :, -1:], u, u[:, :, :1]], axis=2)
    vv = np.concatenate([v[:, :, -1:], v, v[:, :, :1]], axis=2)
    uu[:, 1:, 0], uu[:, :-1, -1] = u[:, :-1, -1], u[:, 1:, 0]
    vv[:, 1:, 0], vv[:, :-1, -1] = v[:, :-1, -1], v[:, 1:, 0]
    uu[:, 0, 0] = uu[:, -1, -1] = vv[:, 0, 0] = vv[:, -1, -1] = np.nan
    assert ref.median_test(uu, vv)[2][:, :, 1:-1].any()


@pytest.mark.parametrize("seed", peak2_ref.SPARSE_SEEDS)
def test_sparse_scene_gain(seed):
    """What one iteration gains on ``peak2_ref.sparse_stack`` (160 x 200, density 0.004, sigma 8, 32 @ 16, r = 2, 297 windows), measured
    on the float64 reference's u, v, u2, v2 cast to float32 -- the truth is a uniform shift, which flatters median replacement:

        seed                                                   5        6
        within 0.5 px before, all windows                     0.838    0.936
        within 0.5 px before, among the finite vectors        0.853    0.939
        after, replace="nan", among the vectors still finite  0.996    0.989
        rejected / substituted                                55 / 5   33 / 2
        substituted vectors within 0.5 px                     5 of 5   2 of 2
        after, replace="median", all windows                  0.980    0.987"""
    r = peak2_ref.sparse_ref(seed)
    u, v = r["u"].astype(np.float32), r["v"].astype(np.float32)
    second = np.stack([r["u2"], r["v2"], r["corr2"], r["ratio"]], axis=-1).astype(np.float32)
    fin = np.isfinite(u) & np.isfinite(v)
    before = ref.share_within(u, v, peak2_ref.TRUTH, fin)
    before_all = ref.share_within(u, v, peak2_ref.TRUTH, np.ones(u.shape, bool))
    un, vn, fn = ref.median_test(u, v, second)
    still = np.isfinite(un) & np.isfinite(vn)
    after = ref.share_within(un, vn, peak2_ref.TRUTH, still)
    sub = fn == 2
    good_sub = int((peak2_ref.within_half_px(un, vn) & sub).sum())
    um, vm, fm = ref.median_test(u, v, second, replace="median")
    after_median = ref.share_within(um, vm, peak2_ref.TRUTH, np.ones(u.shape, bool))
    print(f"seed {seed}: before {before_all:.3f} (finite: {before:.3f}) after {after:.3f} rejected {int((fn == 1).sum())} substituted {int(sub.sum())} "
          f"of which within 0.5 px {good_sub}; replace=median, all windows {after_median:.3f}")
    assert after > before
    assert sub.sum() >= 1 and good_sub == sub.sum()
    assert ref.same(fm == 2, sub) and ref.same(fm == 3, fn == 1)
    assert after_median > before_all


def test_value_errors_of_median_test():
    z = np.zeros((2, 3, 4), np.float32)
    for kw, msg in ((dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"),
                    (dict(epsilon=-0.1), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(min_neighbours=0), "min_neighbours"),
                    (dict(min_neighbours=9), "min_neighbours"), (dict(min_neighbours=2.5), "min_neighbours"), (dict(iterations=0), "iterations"),
                    (dict(iterations=9), "iterations"), (dict(replace="mean"), "replace")):
        with pytest.raises(ValueError, match=msg):
            validate.median_test(z, z, **kw)
    with pytest.raises(ValueError, match="one shape"):
        validate.median_test(z, z[:, :, :3])
    with pytest.raises(ValueError, match="one shape"):
        validate.median_test(z[0, 0], z[0, 0])
    with pytest.raises(ValueError, match="one shape"):
        validate.median_test(z[:, :0], z[:, :0])
    with pytest.raises(ValueError, match="second must have shape"):
        validate.median_test(z, z, np.zeros((2, 3, 4, 2), np.float32))
    with pytest.raises(ValueError, match="unknown keyword"):
        validate.validate_spec({"tau": 2.0})
    with pytest.raises(ValueError, match="validate must be"):
        validate.validate_spec(3)
    assert validate.validate_spec(None) is None and validate.validate_spec(False) is None
    assert validate.validate_spec(True) == validate.ValidateSpec(2.0, 0.1, 3, 0, 1)
    assert validate.validate_spec({"replace": "median", "iterations": 2}) == validate.ValidateSpec(2.0, 0.1, 3, 1, 2)


def test_refusals_point_to_median_test():
    a = np.zeros((3, 96, 96), np.uint8)
    run = lambda **kw: velocimetry.get_ffpiv(a, np.arange(11), np.arange(11), np.ones(2), (16, 16), (8, 8), (16, 16), 1.0, 1.0, **kw)
    with pytest.raises(NotImplementedError, match=r"validate together with ensemble_corr=True.*validate\.median_test"):
        run(validate=True, ensemble_corr=True)
    with pytest.raises(NotImplementedError, match=r"validate together with coarse_passes / deform_passes.*validate\.median_test"):
        run(validate={"iterations": 2}, coarse_passes=[64])
    with pytest.raises(NotImplementedError, match=r"validate together with coarse_passes / deform_passes.*validate\.median_test"):
        run(validate=True, deform_passes=1)
    with pytest.raises(ValueError, match="iterations"):
        run(validate={"iterations": 0})
    with pytest.raises(NotImplementedError, match=r"validate together with ensemble_corr=True"):
        frames.get_piv(a, 16, validate=True, ensemble_corr=True)
    with pytest.raises(NotImplementedError, match=r"validate with pyorc_amd\.shard is not implemented.*validate\.median_test"):
        shard.sharded_piv(lambda a, b: None, 2, (16, 16), (8, 8), None, validate=True)
    with pytest.raises(NotImplementedError, match=r"validate with pyorc_amd\.shard is not implemented"):
        shard.sharded_piv_dev(None, 2, (16, 16), (8, 8), None, validate={"replace": "median"})
    from pyorc_amd import window

    with pytest.raises(NotImplementedError, match=r"validate together with coarse_passes / deform_passes"):
        piv.piv_pairs(a, window.multipass_spec((16, 16), (8, 8), [(64, 32)]), (8, 8), validate=True)


def test_other_engines_do_not_know_the_keyword(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        with pytest.raises(TypeError, match="validate is a keyword of engine='hip' only"):
            rd.Frames(np.zeros((3, 96, 96), np.uint8)).get_piv(16, engine="numba", validate=True)
    finally:
        plugin.uninstall()


def test_validate_none_reaches_the_unchanged_path(monkeypatch):
    """validate=None: the sink is made without the keyword, piv_pairs takes the fused host entry point and hands no spec down."""
    seen = {}

    class Stop(Exception):
        pass

    def fake_sink(*args, **kw):
        seen["sink"] = kw
        raise Stop

    monkeypatch.setattr(velocimetry, "_timestep_sink", fake_sink)
    monkeypatch.setattr(velocimetry, "_plan_slices", lambda n_frames, *args, **kw: (n_frames, [(0, n_frames)], [(0, n_frames)]))
    a = np.zeros((3, 96, 96), np.uint8)
    run = lambda **kw: velocimetry.get_ffpiv(a, np.arange(11), np.arange(11), np.ones(2), (16, 16), (8, 8), (16, 16), 1.0, 1.0, **kw)
    for kw in (dict(), dict(validate=None), dict(validate=False)):
        with pytest.raises(Stop):
            run(**kw)
        assert seen["sink"] == {}, kw
    with pytest.raises(Stop):
        run(validate=True)
    assert seen["sink"] == {"validate": validate.ValidateSpec()}

    def fake_run(imgs, ws, ov, signal_threshold, return_planes, pair_offset, out, scale, entry, args, **kw):
        seen["run"] = (entry, kw)
        return "ran"

    monkeypatch.setattr(piv, "_run_pairs", fake_run)
    scale = (1.0, 1.0, np.ones(2))
    assert piv.piv_pairs(a, (16, 16), (8, 8), scale=scale) == "ran"
    assert seen["run"] == (("lspiv_piv_velocity_at",), {"fused": True, "validate": None})
    assert piv.piv_pairs(a, (16, 16), (8, 8), scale=scale, validate=None) == "ran"
    assert seen["run"] == (("lspiv_piv_velocity_at",), {"fused": True, "validate": None})
    # with a validation the host call must not scale by itself: the median test runs on pixels
    assert piv.piv_pairs(a, (16, 16), (8, 8), scale=scale, validate=True) == "ran"
    assert seen["run"] == (("lspiv_piv_pairs_at", "lspiv_piv_pairs_dev_at"), {"fused": False, "validate": validate.ValidateSpec()})


def test_new_symbols_in_header_signatures_and_exports(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lspiv.h")).read()
    for name in ("lspiv_validate_dev", "lspiv_validate"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define LSPIV_VALIDATE_NAN 0" in header and "#define LSPIV_VALIDATE_MEDIAN 1" in header
    assert validate.REPLACE == ("nan", "median")
    assert "#define LSPIV_ABI_VERSION 5" in header and lib.lspiv_abi_version() == 5
    assert len(_lib.SIGNATURES["lspiv_validate_dev"][1]) == 13 and len(_lib.SIGNATURES["lspiv_validate"][1]) == 12


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    buf = np.zeros(16, np.float32)
    q = _lib.ptr(buf)
    dev = lambda T=1, R=2, C=2, thr=2.0, eps=0.1, m=3, rep=0, it=1, u=q: lib.lspiv_validate_dev(u, q, None, T, R, C, thr, eps, m, rep, it, None, None)
    host = lambda T=1, R=2, C=2, thr=2.0, eps=0.1, m=3, rep=0, it=1, u=q: lib.lspiv_validate(u, q, None, T, R, C, thr, eps, m, rep, it, None)
    for call in (dev, host):
        for kw in (dict(T=0), dict(R=0), dict(C=-1), dict(thr=0.0), dict(thr=float("nan")), dict(eps=-1.0), dict(m=0), dict(m=9), dict(rep=2),
                   dict(rep=-1), dict(it=0), dict(it=9), dict(u=None)):
            assert call(**kw) == _lib.LSPIV_EINVAL, kw
            assert lib.lspiv_last_error()


def test_the_c_example_still_builds(tmp_path):
    from tests.test_c_example import build

    assert os.path.exists(build(tmp_path))
