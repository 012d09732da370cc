"""CPU tests of pyramidal Lucas-Kanade point tracking: the conditions that the GPU tests lean on, checked on
the reference tests/track_ref.py where no GPU is needed (no decision of the shared inputs sits on its threshold; the order of the float64
sums does not matter), what the method buys on synth.particle_stack, the argument checks of pyorc_amd.track and of the C entry points,
and the C-ABI surface.  No kernel runs here."""
import os
import re

import numpy as np
import pytest

from pyorc_amd import _lib, track
from tests import track_inputs as ti
from tests import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT_RUNS = [(c, m) for c in ti.VARIANT_CASES for m in ti.VARIANT_MODES]
ALL_RUNS = [(c, m) for c in ti.CASES for m in ti.MODES] + VARIANT_RUNS + ti.EXTRA_RUNS
RUN_IDS = [f"{ti.case_id(c)}-{m}" for c, m in ALL_RUNS]


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", ALL_RUNS, ids=RUN_IDS)
def test_no_decision_of_a_shared_input_sits_on_its_threshold(case, mode):
    """A condition on the INPUTS, not a tolerance: |delta|^2 against eps^2, det against its bound, lambda against min_eig and the position
    against the borders keep a relative distance of 1e-8 on every point of every shared input (the float64 sums differ by 1e-15 between
    two orders), so status and n_iter of the GPU must be the reference's on every point -- none is left out on the GPU side."""
    m = ti.reference(case, mode)["margins"]
    print(ti.case_id(case), mode, m)
    assert m.smallest() > 1e-8, m


@pytest.mark.parametrize("case,mode", ALL_RUNS, ids=RUN_IDS)
def test_the_order_of_the_float64_sums_moves_nothing_that_counts(case, mode):
    """numpy's pairwise sums against the kernel's order (64 lanes, k ascending on a lane, then the halving tree): the same status and
    n_iter on every point, d within 1e-9 px (measured: at most 7e-16 on CASES, 1.1e-15 on the variant, non-finite and far-guess runs)."""
    a, b = ti.reference(case, mode), ti.reference(case, mode, "lanes")
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["n_iter"], b["n_iter"])
    worst = 0.0
    for name in ("u", "v", "err", "min_eig"):
        assert np.array_equal(np.isnan(a[name]), np.isnan(b[name]))
        if name in ("u", "v") and np.isfinite(a[name]).any():
            worst = max(worst, float(np.nanmax(np.abs(a[name] - b[name]))))
    print(ti.case_id(case), mode, f"largest |d - d'| between the two orders: {worst:.1e} px")
    assert worst < 1e-9


def test_the_shared_inputs_cover_every_status_and_kind_of_point():
    seen = np.zeros(6, dtype=np.int64)
    for case, mode in ALL_RUNS:
        seen += np.bincount(ti.reference(case, mode)["status"].ravel(), minlength=6)
    assert (seen[:5] > 0).all(), seen        # (status 5, a point that is not finite, exists through the C ABI only)
    shape = (48, 64)
    p = ti.points(shape, 65)
    H, W = shape
    for corner in ((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)):
        assert (p == corner).all(axis=1).any()
    assert (p == np.floor(p)).all(axis=1).sum() >= 6             # integer positions: fx = fy = 0
    one_level = ti.CASES[4]                                      # (at one level: higher levels see past the constant block)
    assert one_level[5] == 1
    r = ti.reference(one_level, "converge")
    assert r["status"][0, 3] == tr.STATUS_LOST                   # the corner (0, 0) on the constant block
    assert r["status"][0, 6] == tr.STATUS_OUT                    # the point next to the right border walks out
    assert np.isnan(r["u"][0, [3, 6]]).all() and np.isnan(r["err"][0, [3, 6]]).all()
    nan_case = ti.CASES[7]
    assert nan_case[1] == "float32-nan" and (ti.reference(nan_case, "converge")["status"] == tr.STATUS_NOT_FINITE).any()
    lost_more = (ti.reference(ti.CASES[2], "converge-min-eig")["status"] == 2).sum() - (ti.reference(ti.CASES[2], "converge")["status"] == 2).sum()
    assert lost_more > 0                                         # min_eig > 0 drops points that the determinant test keeps
    bad = tr.track_pairs(ti.scene(shape, 2, "uint8"), np.array([[5.0, np.nan], [20.0, 20.0]]), window=9, levels=2)
    assert bad["status"][0, 0] == tr.STATUS_BAD_POINT and np.isnan(bad["min_eig"][0, 0]) and bad["status"][0, 1] < 2


def test_the_variant_cases_cover_every_instance_of_the_kernel_and_keep_their_points():
    """The 28 (window, dtype) instances once each; five levels in both families and both dtypes; and caps on the lost points that the
    reference alone must meet: in mode "converge" at least half of every case's points are tracked, 60 % at five levels."""
    pairs = [(c[4], c[1]) for c in ti.VARIANT_CASES]
    assert sorted(pairs) == sorted((w, kind) for w in range(tr.MIN_WINDOW, tr.MAX_WINDOW + 1, 2) for kind in ("uint8", "float32")) and len(pairs) == 28
    assert tr.MAX_LEVELS == 5
    for kind in ("uint8", "float32"):
        assert any(c[1] == kind and c[5] == 5 and c[4] <= ti.REG_WINDOW for c in ti.VARIANT_CASES), kind
        assert any(c[1] == kind and c[5] == 5 and c[4] > ti.REG_WINDOW for c in ti.VARIANT_CASES), kind
    assert ti.FIVE_LEVEL_CASE in ti.VARIANT_CASES and ti.FIVE_LEVEL_CASE[5] == 5 and ti.FIVE_LEVEL_CASE[2] == 3
    assert {c[5] for c in ti.VARIANT_CASES} == {1, 2, 3, 4, 5} and {c[2] for c in ti.VARIANT_CASES} == {2, 3}
    for case in ti.VARIANT_CASES:
        shape, kind, T, N, w, L = case
        assert N == ti.VARIANT_N == 65 and max(shape) <= 128           # (the scene's periodic canvas has 128 samples a side)
        tracked = float((ti.reference(case, "converge")["status"] < 2).mean())
        print(ti.case_id(case), f"tracked in mode converge: {tracked:.3f}")
        assert tracked >= (0.6 if L == 5 else 0.5), (case, tracked)


@pytest.mark.parametrize("case", ti.VARIANT_CASES, ids=ti.case_id)
def test_the_variant_cases_min_eig_splits_the_points(case):
    """A condition on the input: of the points that pass the determinant test without min_eig (status other than 2 in mode "converge"),
    the case's own min_eig loses at least 10 % (status 2) and keeps at least 10 %, so `lam < min_eig` is taken both ways."""
    plain, own = ti.reference(case, "converge")["status"], ti.reference(case, "converge-min-eig")["status"]
    assert ti.kwargs(case, "converge-min-eig")["min_eig"] == ti.min_eig_for(case) > 0.0
    passed = plain != tr.STATUS_LOST
    lost = float((own[passed] == tr.STATUS_LOST).mean())
    print(ti.case_id(case), f"min_eig {ti.min_eig_for(case):.4g}: loses {lost:.3f} of {passed.sum()} points")
    assert lost >= 0.1 and 1.0 - lost >= 0.1
    assert not (own[~passed] != tr.STATUS_LOST).any()                 # (min_eig only ever loses points)
    assert all(ti.kwargs(c, "converge-min-eig")["min_eig"] == 30.0 for c in ti.CASES)


@pytest.mark.parametrize("case", ti.NOT_FINITE_CASES, ids=ti.case_id)
def test_a_sample_that_is_not_finite_reaches_some_windows_and_spares_others(case):
    """Conditions on the non-finite scenes: in every mode some point has status 4 and at least a third of the points are tracked."""
    shape, kind, T, N, w, L = case
    value, at = ti.NOT_FINITE[kind]
    f = ti.scene(shape, T, kind)
    bad = ~np.isfinite(f)
    assert bad.sum() == 1 and bad[(1,) + at(*shape)] and T == 3 and L in (1, 2)
    assert np.isnan(value) or f[(1,) + at(*shape)] == value
    for mode in ti.VARIANT_MODES:
        st = ti.reference(case, mode)["status"]
        print(ti.case_id(case), mode, "points per status:", np.bincount(st.ravel(), minlength=6))
        assert (st == tr.STATUS_NOT_FINITE).any(axis=1).all()           # in pair 0 (the sample is in J) and in pair 1 (in the template)
        assert (st < 2).mean() >= 1.0 / 3.0


def test_the_non_finite_and_far_guess_runs_cover_both_families():
    for kind in ti.NOT_FINITE:
        ws = [c[4] for c in ti.NOT_FINITE_CASES if c[1] == kind]
        assert len(ws) == 2 and min(ws) <= ti.REG_WINDOW < max(ws), kind
    assert {c[5] for c in ti.NOT_FINITE_CASES if c[4] <= ti.REG_WINDOW} == {1, 2} == {c[5] for c in ti.NOT_FINITE_CASES if c[4] > ti.REG_WINDOW}
    assert len(ti.FAR_CASES) == 2 and min(c[4] for c in ti.FAR_CASES) <= ti.REG_WINDOW < max(c[4] for c in ti.FAR_CASES)
    for case in ti.FAR_CASES:
        assert case in ti.VARIANT_CASES and case[5] == 3
        far = sorted(ti.FAR_POINTS)
        g = ti.kwargs(case, "far-guess")["guess"]
        assert np.abs(g[:, far]).max() == 1e12 and np.abs(np.ldexp(g[:, far], -2)).max(axis=2).min() > 2.0 ** 29   # (split() clamps at 2^30)
        near, r = ti.reference(case, "converge-guess"), ti.reference(case, "far-guess")
        assert (near["status"][:, far] < 2).all()                       # tracked with the plain guess
        assert (r["status"][:, far] == tr.STATUS_OUT).all() and (r["n_iter"][:, far] == 1).all()
        rest = np.setdiff1d(np.arange(case[3]), far)
        assert all(np.array_equal(near[n][:, rest], r[n][:, rest], equal_nan=n != "n_iter" and n != "status") for n in ("u", "v", "status", "n_iter"))
    # the reference's own clamp holds up to the largest guesses: no error, the same status
    case = ti.FAR_CASES[0]
    shape, kind, T, N, w, L = case
    g = ti.guess_for(case)
    g[:, 0], g[:, 8] = (1e300, -1e300), (-1e300, 0.3)
    r = tr.track_pairs(ti.scene(shape, T, kind), ti.points(shape, N), window=w, levels=L, guess=g)
    assert (r["status"][:, [0, 8]] == tr.STATUS_OUT).all() and (r["n_iter"][:, [0, 8]] == 1).all()


def test_trajectories_of_the_reference_at_five_levels_keep_their_margins():
    shape, kind, T, N, w, L = ti.FIVE_LEVEL_CASE
    r = ti.reference_trajectories(ti.FIVE_LEVEL_CASE)
    print(ti.case_id(ti.FIVE_LEVEL_CASE), r["margins"], "points per status:", np.bincount(r["status"].ravel(), minlength=6))
    assert r["margins"].smallest() > 1e-8
    assert (r["status"][-1] < 2).mean() >= 0.5 and (r["status"] == tr.STATUS_BAD_POINT).any()


def test_trajectories_of_the_reference_chain_the_pairs():
    shape, kind, T, N, w, L = ti.TRAJ_CASE
    r = tr.trajectories(ti.scene(shape, T, kind), ti.points(shape, N), window=w, levels=L)
    assert np.array_equal(r["xy"][0], ti.points(shape, N))
    lost = r["status"] >= 2
    assert lost.any() and not lost.all()
    for t in range(T - 1):
        assert np.isnan(r["xy"][t + 1][lost[t]]).all() and np.isfinite(r["xy"][t + 1][~lost[t]]).all()
        if t:
            assert (r["status"][t][lost[t - 1]] == tr.STATUS_BAD_POINT).all()      # lost stays lost
    assert r["margins"].smallest() > 1e-8
    ok = ~lost.any(axis=0)
    travelled = r["xy"][-1, ok] - r["xy"][0, ok]
    np.testing.assert_allclose(np.median(travelled, axis=0), (T - 1) * np.array(ti.SHIFT), atol=0.1)


# ---- what the method buys -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.012])
@pytest.mark.parametrize("flow", ["shift", "sine"])
def test_accuracy_study(flow, density):
    """synth.particle_stack, 160 x 200; the uniform 9.3 / -6.4 px shift and the default sine flow (3 +- 2 / +- 1.5 px); the grids 32 @ 16
    and 16 @ 8; w in {15, 21, 31}; 1, 3 and 4 levels.  INTEGRATION.md section 2n has the table.  The claims, on the large shift: one
    level fails (the reference: at most 0.040 of the points within 0.5 px; asserted < 0.1); four levels recover it on the 32 @ 16 grid
    (at least 0.949; asserted >= 0.9 -- on the 16 @ 8 grid more centres sit within reach of the border and walk out: 0.838 .. 0.923,
    asserted >= 0.8); the median error of four levels is 0.017 .. 0.022 px (asserted < 0.05).  On the sine flow, whose 1 .. 5 px one
    level mostly reaches, the pyramid keeps the share at 0.98 or above on the 32 @ 16 grid (asserted >= 0.95)."""
    f = ti.study_scene(flow, density)
    for ws, ov in ((32, 16), (16, 8)):
        pts, _ = tr.grid_points(*ti.STUDY_SHAPE, ws, ov)
        truth = ti.study_truth(flow, pts)
        for w in (15, 21, 31):
            for levels in (1, 3, 4):
                r = tr.track_pairs(f, pts, window=w, levels=levels)
                share, median, lost = ti.study_figures(r, truth)
                print(f"{flow} density {density} grid {ws}@{ov} w {w} levels {levels}: {share:.3f} within 0.5 px, median error {median:.4f} px, "
                      f"{lost} of {len(pts)} lost, mean n_iter {r['n_iter'].mean():.1f}")
                if flow == "shift":
                    if levels == 1:
                        assert share < 0.1
                    if levels == 4:
                        assert share >= (0.9 if ws == 32 else 0.8) and median < 0.05
                elif levels >= 3 and ws == 32:
                    assert share >= 0.95


# ---- argument checks of the module ----------------------------------------------------------------------------------------------------------
H, W = 33, 47
PTS = np.array([[0.0, 0.0], [W - 1.0, H - 1.0], [10.5, 7.25]])


def _runs_or_lacks_a_device(call):
    """The arguments pass the checks: with a GPU the call runs, without one the only error is the missing device (never a ValueError)."""
    try:
        call()
    except _lib.LspivError as e:
        assert e.code == _lib.LSPIV_ENODEV and not isinstance(e, ValueError), e


def test_points_on_the_frames_edge_are_accepted_and_one_beyond_is_not():
    frames = np.zeros((3, H, W), dtype=np.uint8)
    _runs_or_lacks_a_device(lambda: track.track_pairs(frames, PTS))
    for bad in ([W - 1.0 + 1e-9, 5.0], [-1e-9, 2.0], [np.nan, 2.0], [1.0, H - 1.0 + 1e-9], [1.0, -1e-9], [np.inf, 2.0]):
        p = PTS.copy()
        p[2] = bad
        with pytest.raises(ValueError, match="point 2 "):
            track.track_pairs(frames, p)
        with pytest.raises(ValueError, match="point 2 "):
            track.trajectories(frames, p)
        per_pair = np.stack([PTS, p])
        with pytest.raises(ValueError, match="point 2 of pair 1"):
            track.track_pairs(frames, per_pair)


def test_type_shape_and_range_errors():
    frames = np.zeros((3, H, W), dtype=np.uint8)
    with pytest.raises(TypeError, match="float64"):
        track.track_pairs(frames.astype(np.float64), PTS)
    with pytest.raises(TypeError, match="int16"):
        track.pyr_down(frames.astype(np.int16))
    with pytest.raises(TypeError, match="uint16"):
        track.trajectories(frames.astype(np.uint16), PTS)
    with pytest.raises(ValueError, match=r"\(T, H, W\)"):
        track.track_pairs(frames[0], PTS)
    with pytest.raises(ValueError, match="at least 2"):
        track.track_pairs(frames[:1], PTS)
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        track.track_pairs(frames, PTS[:, :1])
    with pytest.raises(ValueError, match=r"\(2, N, 2\)"):
        track.track_pairs(frames, np.stack([PTS] * 3))
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        track.trajectories(frames, np.stack([PTS] * 2))
    for w in (3, 4, 20, 33, -5):
        with pytest.raises(ValueError, match=f"window {w}"):
            track.track_pairs(frames, PTS, window=w)
    with pytest.raises(TypeError, match="window"):
        track.track_pairs(frames, PTS, window=9.0)
    for n in (0, 101):
        with pytest.raises(ValueError, match=f"max_iter {n}"):
            track.track_pairs(frames, PTS, max_iter=n)
    for lv in (0, 6):
        with pytest.raises(ValueError, match=f"levels {lv}"):
            track.track_pairs(frames, PTS, levels=lv)
    with pytest.raises(ValueError, match="eps"):
        track.track_pairs(frames, PTS, eps=-1e-3)
    with pytest.raises(ValueError, match="eps"):
        track.track_pairs(frames, PTS, eps=float("nan"))
    with pytest.raises(ValueError, match="min_eig"):
        track.track_pairs(frames, PTS, min_eig=-1.0)
    with pytest.raises(ValueError, match="guess"):
        track.track_pairs(frames, PTS, guess=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="guess: point 1"):
        track.track_pairs(frames, PTS, guess=np.array([[0.0, 0.0], [np.nan, 0.0], [0.0, 0.0]]))
    with pytest.raises(ValueError, match="guess"):
        track.track_grid(frames, 16, guess=np.zeros((3, 3, 2)))
    with pytest.raises(ValueError, match="smaller than 3 x 3"):
        track.pyr_down(frames[:, :2])
    # a stack too small for its levels: the message says which level fails
    assert track.level_shapes(33, 47, 5) == [(33, 47), (17, 24), (9, 12), (5, 6), (3, 3)] == tr.level_shapes(33, 47, 5)
    _runs_or_lacks_a_device(lambda: track.track_pairs(frames, PTS, levels=5, window=5))
    small = np.zeros((2, 9, 40), dtype=np.uint8)            # 9 -> 5 -> 3 -> 2: level 3 can be the last level, not a source
    _runs_or_lacks_a_device(lambda: track.track_pairs(small, PTS[:1], levels=4, window=5))
    with pytest.raises(ValueError, match="level 3 "):
        track.track_pairs(small, PTS[:1], levels=5, window=5)
    with pytest.raises(ValueError, match="level 0 "):
        track.track_pairs(small[:, :2], PTS[:1], levels=2, window=5)     # 2 rows cannot be a source of pyr_down
    _runs_or_lacks_a_device(lambda: track.track_pairs(small[:, :2], PTS[:1], levels=1, window=5))
    for Hh, Ww, lv in ((9, 40, 5), (2, 40, 2), (33, 47, 5), (3, 3, 2), (1, 9, 1)):
        lvl = tr.failing_level(Hh, Ww, lv)
        if lvl is None:
            track._check_levels(Hh, Ww, lv)
        else:
            with pytest.raises(ValueError, match=f"level {lvl} "):
                track._check_levels(Hh, Ww, lv)


# ---- argument checks of the C entry points --------------------------------------------------------------------------------------------------
def _c_track(lib, frames, pts, dtype=None, window=9, levels=2, max_iter=5, eps=0.01, min_eig=0.0, chain=0, per_pair=0, xy=True):
    T, Hh, Ww = frames.shape
    N = pts.shape[-2]
    out = [np.zeros((T - 1, N)) for _ in range(4)]
    n_iter, status = np.zeros((T - 1, N), dtype=np.int32), np.zeros((T - 1, N), dtype=np.uint8)
    traj = np.zeros((T, N, 2))
    return lib.lspiv_lk_track(_lib.ptr(frames), _lib.DTYPE_CODES[frames.dtype] if dtype is None else dtype, T, Hh, Ww, _lib.ptr(pts), N, per_pair, None, 0,
                              window, levels, max_iter, eps, min_eig, chain, *(_lib.ptr(q) for q in out), _lib.ptr(n_iter), _lib.ptr(status),
                              _lib.ptr(traj) if xy else None)


def test_c_entry_points_refuse_bad_arguments_and_never_launch(lib):
    frames = np.zeros((3, H, W), dtype=np.uint8)
    pts = np.ascontiguousarray(PTS)
    assert _c_track(lib, frames, pts) in (_lib.LSPIV_OK, _lib.LSPIV_ENODEV)
    for kw, word in ((dict(window=8), b"window 8"), (dict(window=3), b"window 3"), (dict(window=33), b"window 33"), (dict(levels=0), b"levels 0"),
                     (dict(levels=6), b"levels 6"), (dict(max_iter=0), b"max_iter 0"), (dict(max_iter=101), b"max_iter 101"), (dict(eps=-1.0), b"eps"),
                     (dict(eps=float("nan")), b"eps"), (dict(min_eig=-1.0), b"min_eig"), (dict(dtype=2), b"dtype 2"),
                     (dict(chain=1, xy=False), b"chain"), (dict(chain=1, per_pair=1), b"chain")):
        assert _c_track(lib, frames, pts, **kw) == _lib.LSPIV_EINVAL, kw
        assert word in lib.lspiv_last_error(), (kw, lib.lspiv_last_error())
    assert _c_track(lib, frames[:1], pts) == _lib.LSPIV_EINVAL                        # one frame is no pair
    small = np.zeros((2, 9, 40), dtype=np.uint8)
    assert _c_track(lib, small, pts[:1], window=5, levels=5) == _lib.LSPIV_EINVAL and b"level 3 " in lib.lspiv_last_error()
    assert _c_track(lib, small[:, :2], pts[:1], window=5, levels=2) == _lib.LSPIV_EINVAL and b"level 0 " in lib.lspiv_last_error()
    out = np.zeros((3, 2, 2), dtype=np.float32)
    assert lib.lspiv_pyr_down(_lib.ptr(frames[:, :2]), 0, 3, 2, W, _lib.ptr(out)) == _lib.LSPIV_EINVAL
    assert lib.lspiv_pyr_down(_lib.ptr(frames), 2, 3, H, W, _lib.ptr(out)) == _lib.LSPIV_EINVAL
    assert lib.lspiv_pyr_down(None, 0, 3, H, W, _lib.ptr(out)) == _lib.LSPIV_EINVAL
    assert lib.lspiv_pyr_down_dev(None, 0, 3, H, W, None, None) == _lib.LSPIV_EINVAL
    assert lib.lspiv_lk_track_dev(None, 0, 3, H, W, None, 3, 0, None, 0, 9, 2, 5, 0.01, 0.0, 0, None, None, None, None, None, None, None,
                                  None) == _lib.LSPIV_EINVAL


def test_the_four_entry_points_are_declared_bound_and_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lspiv.h")).read(), flags=re.S)
    for name in ("lspiv_pyr_down_dev", "lspiv_pyr_down", "lspiv_lk_track_dev", "lspiv_lk_track"):
        assert re.search(rf"\bint {name}\s*\(", txt), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        n_args = txt[txt.index(name + "("):].split(");")[0].count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert lib.lspiv_abi_version() == 5 and "#define LSPIV_ABI_VERSION 5" in txt
    import pyorc_amd

    assert pyorc_amd.track is track
    for name in ("track_pairs", "track_grid", "trajectories", "pyr_down", "Tracks"):
        assert hasattr(track, name)
    mk = open(os.path.join(ROOT, "pyorc_amd", "csrc", "Makefile")).read()
    assert "api_track.hip" in mk and " track.hip" in mk
    assert (track.MIN_WINDOW, track.MAX_WINDOW, track.MAX_LEVELS, track.MAX_ITER) == (tr.MIN_WINDOW, tr.MAX_WINDOW, tr.MAX_LEVELS, tr.MAX_ITER)
