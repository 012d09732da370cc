"""Second correlation peak on the GPU against tests/peak2_ref.py, the float64 reference: the fused kernels
through ``piv.piv_pairs_peak2`` (the device entry point for ``DeviceFrames``, the host-fed one for numpy stacks), the generic kernel on
planes through ``piv.second_peak``, and ``get_ffpiv(peak_ratio=True)``.

Gates.  u, v, corr_max, s2n and the planes are the bits of the shifted kernel without offsets; the planes lie within 2e-6 of the
reference's (the project's plane gate; d = the measured deviation).  On the windows the reference does not call fragile (tests/
test_peak2_host.py caps their share at 5 % for every input used here): the second peak exists where the reference's does and sits on
the same sample; |corr2 - ref| <= 2e-6; peak_ratio within 2 * ratio_ref * 2e-6 * (1 / p1 + 1 / corr2) -- two plane errors at a factor of
two, which also covers one ulp of the division --; u2, v2 within 1e-5 + B, B the largest motion of the reference's own fit when its five
samples move by +-2 d over all 32 sign patterns (the second peaks are flat: B reaches millipixels, which is why no fixed 1e-4 holds)."""
import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import deform_ref, lazy_doubles
from tests import peak2_ref as ref
from tests.test_gpu_multipass import KEYS, _Lazy

pytestmark = pytest.mark.gpu
CASES = sorted(ref.PASS_CASES)
IDS = ["u8", "f32", "f64"]
KEYS2 = KEYS + ("peak_ratio", "corr2", "v_x2", "v_y2")


def same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True), (what, k)


def positions(p2, wy, wx):
    """The integer position the runner-up vector points at (the fit moves it by at most half a sample: read only where :func:`clear` says
    the reference's own offsets stay away from that half); -1 where the vector is NaN."""
    with np.errstate(invalid="ignore"):
        i = np.where(np.isnan(p2[..., 1]), -1, np.rint(p2[..., 1] + wy // 2)).astype(np.int64)
        j = np.where(np.isnan(p2[..., 0]), -1, np.rint(p2[..., 0] + wx // 2)).astype(np.int64)
    return i, j


def clear(u2, v2, i2, j2, wy, wx):
    """Do the reference's sub-pixel offsets at (i2, j2) stay below 0.49, so that rounding the vector gives the sample back?  (A second peak
    with a neighbour of its own height is fitted half way between the two, whichever of them holds it.)"""
    return abs(u2 + wx // 2 - j2) < 0.49 and abs(v2 + wy // 2 - i2) < 0.49


def gate(p2, planes, r, what):
    """``p2`` (P, rows, cols, 4) and the call's own ``planes`` against the reference ``r``; prints each figure before it asserts."""
    shape = r["corr"].shape
    n = planes.shape[-1]
    assert p2.dtype == np.float32 and p2.shape == shape + (4,) and planes.shape == r["planes"].shape
    pl = planes.reshape(shape + (n, n))
    ref_pl = r["planes"].reshape(shape + (n, n))
    skipped = np.isnan(r["corr"])
    with np.errstate(invalid="ignore"):
        d = float(np.nanmax(np.abs(pl.astype(np.float64) - ref_pl))) if (~skipped).any() else 0.0
    print(what, "planes: largest deviation d =", d)
    assert np.array_equal(np.isnan(pl), np.isnan(ref_pl)) and d <= ref.PLANE_GATE
    u2, v2, c2, ratio = (p2[..., k] for k in range(4))
    # skipped windows: NaN in all four, nowhere else in corr2 and peak_ratio
    for q in (u2, v2, c2, ratio):
        assert np.isnan(q[skipped]).all()
    assert not np.isnan(c2[~skipped]).any() and not np.isnan(ratio[~skipped]).any()
    ok = ~skipped & ~r["fragile2"]
    print(what, "windows", int((~skipped).sum()), "left out as fragile", int((~skipped & r["fragile2"]).sum()))
    assert (~skipped & r["fragile2"]).sum() <= 0.05 * (~skipped).sum()
    found = c2 > 0
    assert np.array_equal(found[ok], r["found"][ok]), "existence of the second peak"
    none = ok & ~r["found"]
    assert (c2[none] == 0).all() and np.isposinf(ratio[none]).all() and np.isnan(u2[none]).all() and np.isnan(v2[none]).all()
    gi, gj = positions(p2, n, n)
    worst = dict(corr2=0.0, ratio=0.0, uv=0.0, B=0.0)
    for idx in zip(*np.nonzero(ok & r["found"])):
        i2, j2 = int(r["i2"][idx]), int(r["j2"][idx])
        assert pl[idx][i2, j2] == c2[idx], (what, idx, "corr2 is not the sample at the reference's position")
        border = i2 in (0, n - 1) or j2 in (0, n - 1)
        if not border and clear(r["u2"][idx], r["v2"][idx], i2, j2, n, n):
            assert (gi[idx], gj[idx]) == (i2, j2), (what, idx, "position")
        p1 = float(ref_pl[idx].max())
        e_c = abs(float(c2[idx]) - r["corr2"][idx])
        tol_r = 2.0 * r["ratio"][idx] * ref.PLANE_GATE * (1.0 / p1 + 1.0 / r["corr2"][idx])
        e_r = abs(float(ratio[idx]) - r["ratio"][idx])
        B = ref.fit_motion(ref_pl[idx], i2, j2, d)
        with np.errstate(invalid="ignore"):
            e_uv = max(abs(float(u2[idx]) - r["u2"][idx]), abs(float(v2[idx]) - r["v2"][idx]))
        assert np.isnan(u2[idx]) == np.isnan(r["u2"][idx]) and np.isnan(v2[idx]) == np.isnan(r["v2"][idx]), (what, idx, "NaN mask")
        worst = dict(corr2=max(worst["corr2"], e_c), ratio=max(worst["ratio"], e_r / tol_r), uv=max(worst["uv"], 0.0 if np.isnan(e_uv) else e_uv),
                     B=max(worst["B"], B))
        assert e_c <= ref.PLANE_GATE, (what, idx, "corr2", e_c)
        assert e_r <= tol_r, (what, idx, "peak_ratio", e_r, tol_r)
        assert np.isnan(e_uv) or e_uv <= 1e-5 + B, (what, idx, "u2 / v2", e_uv, B)
    print(what, "largest |corr2 - ref| %.2e, peak_ratio error / its bound %.3f, largest |u2, v2 - ref| %.2e px (largest B %.2e)"
          % (worst["corr2"], worst["ratio"], worst["uv"], worst["B"]))


def run_public(a, n, ov, **kw):
    nr, nc = window.get_array_shape(a.shape[1:], (n, n), (ov, ov))
    return velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), np.ones(len(a) - 1), (n, n), (ov, ov), (n, n), 1.0, 1.0, **kw)


# ---- 1. parity, 2. the register path against the simple path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", deform_ref.PASS_DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_shifted_kernel_and_the_reference(gpu, case, dtype):
    n, ov, _ = ref.PASS_CASES[case]
    a, r = deform_ref.pass_stack(case, dtype), ref.pass_ref(case, dtype)
    d = DeviceFrames.from_host(a)
    *res, p2, planes = piv.piv_pairs_peak2(d, (n, n), (ov, ov), return_planes=True)
    same_bits(res + [planes], piv.piv_pairs_shifted(d, (n, n), (ov, ov), None, return_planes=True), "the shifted kernel without offsets")
    gate(p2, planes, r, f"{case} {np.dtype(dtype).name} device")
    # the generic kernel on the fused kernel's own planes: same plane, same rule, same fit function -- every window, no fragile set
    same_bits([piv.second_peak(planes).reshape(p2.shape)], [p2], "register path against the simple path")
    *host, hp2, hplanes = piv.piv_pairs_peak2(a, (n, n), (ov, ov), return_planes=True)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(host + [hp2, hplanes], res + [p2, planes], "host-fed and device entry points differ")
    else:
        gate(hp2, hplanes, r, f"{case} float64 host-fed")
    same_bits(piv.piv_pairs_peak2(a, (n, n), (ov, ov)), host + [hp2], "without planes")


# ---- 3. signal threshold ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_signal_threshold_skips_all_four_outputs(gpu, case):
    n, ov, _ = ref.PASS_CASES[case]
    r = ref.signal_ref(case)
    a = deform_ref.signal_stack(case)
    for dtype in deform_ref.PASS_DTYPES:       # (the float stacks hold the same sample values: an affine map would move the zeros)
        d = DeviceFrames.from_host(a.astype(dtype))
        u, v, cm, sn, p2, planes = piv.piv_pairs_peak2(d, (n, n), (ov, ov), signal_threshold=deform_ref.SIGNAL_THR, return_planes=True)
        skipped = np.isnan(cm)
        assert skipped.any() and (~skipped).any() and np.array_equal(skipped, np.isnan(r["corr"]))
        for k in range(4):
            assert np.isnan(p2[..., k][skipped]).all()
        assert np.array_equal(np.isnan(p2[..., 2]), skipped) and np.array_equal(np.isnan(p2[..., 3]), skipped)
        assert np.array_equal(np.isnan(planes).all(axis=(-2, -1)).reshape(skipped.shape), skipped)
        same_bits([u, v, cm, sn, planes], piv.piv_pairs_shifted(d, (n, n), (ov, ov), None, deform_ref.SIGNAL_THR, return_planes=True), "shifted")
        gate(p2, planes, r, f"{case} signal {np.dtype(dtype).name}")
        same_bits([piv.second_peak(planes).reshape(p2.shape)], [p2], "simple path, NaN planes included")
    host = piv.piv_pairs_peak2(a, (n, n), (ov, ov), signal_threshold=deform_ref.SIGNAL_THR)
    same_bits(host[:5], piv.piv_pairs_peak2(DeviceFrames.from_host(a), (n, n), (ov, ov), signal_threshold=deform_ref.SIGNAL_THR), "host-fed")


# ---- 4. exclusion radius ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_excl", ref.RADII)
@pytest.mark.parametrize("case", (16, 32))
def test_exclusion_radius(gpu, case, r_excl):
    n, ov, _ = ref.PASS_CASES[case]
    d = DeviceFrames.from_host(deform_ref.pass_stack(case))
    *_, p2, planes = piv.piv_pairs_peak2(d, (n, n), (ov, ov), r_excl, return_planes=True)
    gate(p2, planes, ref.pass_ref(case, np.uint8, r_excl), f"{case} r = {r_excl}")
    same_bits([piv.second_peak(planes, r_excl).reshape(p2.shape)], [p2], "simple path")
    same_bits([piv.piv_pairs(d, window.PeakRatioWindow((n, n), r_excl), (ov, ov))[4]], [p2], "piv_pairs dispatches on a PeakRatioWindow")


@pytest.mark.parametrize("mode", (1, 2))
def test_border_modes_in_the_fused_kernel(gpu, mode):
    """"border_peak" flipped in library and reference: the primary and the runner-up vector follow it, on the 16 px input, whose planes
    put second peaks on the border."""
    n, ov, _ = ref.PASS_CASES[16]
    a = deform_ref.pass_stack(16)
    with po.semantics(border_peak=mode):
        r = ref.piv(a, n, ov, 4)
        on_border = r["found"] & ((r["i2"] == 0) | (r["i2"] == n - 1) | (r["j2"] == 0) | (r["j2"] == n - 1)) & ~r["fragile2"]
        assert on_border.any() and np.isfinite(r["u2"][on_border]).all()
        _lib.set_option("border_peak", mode)
        try:
            *res, p2, planes = piv.piv_pairs_peak2(DeviceFrames.from_host(a), (n, n), (ov, ov), 4, return_planes=True)
            simple = piv.second_peak(planes, 4)
        finally:
            _lib.set_option("border_peak", 0)
        gate(p2, planes, r, f"border_peak = {mode}")
    same_bits([simple.reshape(p2.shape)], [p2], "simple path")
    assert np.array_equal(p2[..., 0][on_border], r["u2"][on_border]) and np.array_equal(p2[..., 1][on_border], r["v2"][on_border])


# ---- 5. hand-made planes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("shape", ref.HAND_SHAPES)
def test_hand_made_planes_through_second_peak(gpu, shape, mode):
    wy, wx = shape
    hand = ref.hand_planes(wy, wx)
    planes = np.stack([pl for _, pl, _ in hand])[None]
    _lib.set_option("border_peak", mode)
    try:
        got = piv.second_peak(planes, 2)[0]
        flipped = None
        if mode == 2:
            _lib.set_option("v_sign", 1)
            flipped = piv.second_peak(planes, 2)[0]
    finally:
        _lib.set_option("border_peak", 0)
        _lib.set_option("v_sign", 0)
    assert got.shape == (len(hand), 4) and got.dtype == np.float32
    gi, gj = positions(got, wy, wx)
    borders = 0
    for k, (name, pl, expected) in enumerate(hand):
        u2, v2, c2, ratio = (float(x) for x in got[k])
        with po.semantics(border_peak=mode):
            want = ref.plane_result(pl, 2)
        if expected == "nan":
            assert all(np.isnan(x) for x in (u2, v2, c2, ratio)), name
            continue
        if expected is None:
            assert c2 == 0.0 and ratio == np.inf and np.isnan(u2) and np.isnan(v2), name
            continue
        i2, j2 = expected
        assert c2 == float(pl[i2, j2]) and abs(ratio - want["ratio"]) <= 2e-7 * want["ratio"], (name, c2, ratio)
        border = i2 in (0, wy - 1) or j2 in (0, wx - 1)
        borders += border
        if border and mode == 0:
            assert np.isnan(u2) and np.isnan(v2), name
        elif border:
            assert (u2, v2) == ((0.0, 0.0) if mode == 1 else (float(j2 - wx // 2), float(i2 - wy // 2))), name
        else:
            if clear(want["u2"], want["v2"], i2, j2, wy, wx):
                assert (gi[k], gj[k]) == (i2, j2), (name, "position")
            assert abs(u2 - want["u2"]) <= 1e-4 and abs(v2 - want["v2"]) <= 1e-4, (name, u2, v2, want)
    assert borders == 2
    if flipped is not None:     # "v_sign": v2 negated, nothing else moves
        same_bits([flipped[:, 0], -flipped[:, 1], flipped[:, 2], flipped[:, 3]], [got[:, k] for k in range(4)], "v_sign")


# ---- 6. ensemble mean planes ----------------------------------------------------------------------------------------------------------------
def test_ensemble_mean_planes_through_second_peak(gpu):
    n, ov, dim = ref.PASS_CASES[32]
    a = deform_ref.pass_stack(32)
    e = piv.Ensemble(dim, (n, n), (ov, ov))
    try:
        e.accumulate(a, 0.2, 3.0)
        *_, mean = e.finish(0.2, 1, return_mean=True)
    finally:
        e.close()
    got = piv.second_peak(mean, 2)
    want = ref.on_planes(mean.astype(np.float64), 2, with_fragile=False)       # the reference, read on those same float32 planes
    finite = np.isfinite(mean).all(axis=(-2, -1))
    assert finite.any() and got.shape == mean.shape[:2] + (4,)
    assert np.isnan(got[~finite]).all()
    assert np.array_equal(got[..., 2] > 0, want["found"]) and want["found"].any()
    assert np.array_equal(got[..., 2][finite], want["corr2"][finite].astype(np.float32))
    sel = finite & want["found"]
    with np.errstate(invalid="ignore"):
        exact = (mean.max(axis=(-2, -1)).astype(np.float64) / got[..., 2])[sel]
    assert (np.abs(got[..., 3][sel] - exact) <= 1.2e-7 * exact).all()          # (one float32 rounding of the quotient)
    gi, gj = positions(got, n, n)
    inner = want["found"] & (want["i2"] > 0) & (want["i2"] < n - 1) & (want["j2"] > 0) & (want["j2"] < n - 1)
    for idx in zip(*np.nonzero(inner)):
        i2, j2 = int(want["i2"][idx]), int(want["j2"][idx])
        assert mean[idx][i2, j2] == got[..., 2][idx]
        if clear(want["u2"][idx], want["v2"][idx], i2, j2, n, n):
            assert (gi[idx], gj[idx]) == (i2, j2), idx
    assert np.isnan(got[..., 0][want["found"] & ~inner]).all()
    with np.errstate(invalid="ignore"):
        print("ensemble mean planes: windows", int(finite.sum()), "with a second peak", int(want["found"].sum()), "largest |u2, v2 - ref|",
              float(np.nanmax(np.abs(got[..., :2] - np.stack([want["u2"], want["v2"]], axis=-1)))))


# ---- 7. chunks and callers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_chunks_and_callers_give_the_same_bits(gpu, case):
    n, ov, _ = ref.PASS_CASES[case]
    a = deform_ref.pass_stack(case)
    d = DeviceFrames.from_host(a)
    whole = piv.piv_pairs_peak2(a, (n, n), (ov, ov), return_planes=True)
    for stack in (a, d):
        parts = [piv.piv_pairs_peak2(stack[f0:f1], (n, n), (ov, ov), return_planes=True, pair_offset=f0) for f0, f1 in ((0, 3), (2, 4))]
        same_bits([np.concatenate([p[k] for p in parts]) for k in range(6)], whole, "chunks [0:3] + [2:4]")
    pub = run_public(a, n, ov, peak_ratio=True)
    want = [whole[0], whole[1], whole[2], whole[3], whole[4][..., 3], whole[4][..., 2], whole[4][..., 0], whole[4][..., 1]]
    same_bits([np.asarray(pub[k]) for k in KEYS2], want, "get_ffpiv")
    assert set(pub) == set(KEYS2)
    for stack, kw in ((d, dict()), (a, dict(devices=[0, 0])), (a, dict(chunksize=2)), (d, dict(chunksize=2)), (_Lazy(a), dict(chunksize=3)),
                      (lazy_doubles.from_frames(a, block=2), dict(time=np.arange(len(a)))),
                      (lazy_doubles.from_frames(a, block=3), dict(time=np.arange(len(a)), devices=[0, 0], chunksize=2))):
        same_bits([np.asarray(run_public(stack, n, ov, peak_ratio=True, **kw)[k]) for k in KEYS2], want, (type(stack).__name__, kw))
    plain = run_public(a, n, ov)
    assert set(plain) == set(KEYS)
    same_bits([np.asarray(run_public(a, n, ov, peak_ratio=False, peak_exclusion=99)[k]) for k in KEYS], [np.asarray(plain[k]) for k in KEYS], "False")


def test_scaling_v_sign_and_out_arguments(gpu):
    n, ov, _ = ref.PASS_CASES[32]
    a = deform_ref.pass_stack(32)
    u, v, cm, sn, p2 = piv.piv_pairs_peak2(a, (n, n), (ov, ov))
    dt = np.array([0.5, 0.25, 2.0])
    scaled = lambda q, res: (q * res / dt[:, None, None]).astype(np.float32)
    out = [np.empty_like(u) for _ in range(4)]
    for stack in (a, DeviceFrames.from_host(a)):
        got = piv.piv_pairs_peak2(stack, (n, n), (ov, ov), out=out, scale=(0.02, 0.03, dt))
        assert all(g is o for g, o in zip(got, out))
        same_bits(list(got[:4]) + [got[4][..., k] for k in range(4)],
                  [scaled(u, 0.02), scaled(v, 0.03), cm, sn, scaled(p2[..., 0], 0.02), scaled(p2[..., 1], 0.03), p2[..., 2], p2[..., 3]], "scale")
    nr, nc = u.shape[1:]
    run = lambda **kw: velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), dt, (n, n), (ov, ov), (n, n), 0.03, 0.02, peak_ratio=True, **kw)
    pub = run()
    same_bits([np.asarray(pub[k]) for k in ("v_x", "v_y", "v_x2", "v_y2", "corr2", "peak_ratio")],
              [scaled(u, 0.02), scaled(v, 0.03), scaled(p2[..., 0], 0.02), scaled(p2[..., 1], 0.03), p2[..., 2], p2[..., 3]], "get_ffpiv scales v_x2, v_y2")
    assert np.isfinite(p2[..., 1]).any()
    _lib.set_option("v_sign", 1)
    try:
        flipped = run()
        f2 = piv.piv_pairs_peak2(DeviceFrames.from_host(a), (n, n), (ov, ov))[4]
    finally:
        _lib.set_option("v_sign", 0)
    same_bits([np.asarray(flipped[k]) for k in ("v_x", "v_x2", "corr2", "peak_ratio")], [np.asarray(pub[k]) for k in ("v_x", "v_x2", "corr2", "peak_ratio")], "v_sign")
    same_bits([-np.asarray(flipped["v_y"]), -np.asarray(flipped["v_y2"]), -f2[..., 1]], [np.asarray(pub["v_y"]), np.asarray(pub["v_y2"]), p2[..., 1]], "v_sign on v, v2")


def test_frames_get_piv_and_the_wrapped_accessor(gpu, monkeypatch):
    """``frames.get_piv(..., peak_ratio=True)`` and ``Frames.get_piv(engine="hip", peak_ratio=True)`` are ``piv_pairs_peak2``."""
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    a = deform_ref.pass_stack(16)
    whole = {r: piv.piv_pairs_peak2(a, (16, 16), (8, 8), r) for r in (2, 4)}
    want = lambda r: list(whole[r][:4]) + [whole[r][4][..., 3], whole[r][4][..., 2], whole[r][4][..., 0], whole[r][4][..., 1]]
    assert not np.array_equal(whole[2][4], whole[4][4], equal_nan=True)
    same_bits([np.asarray(frames.get_piv(a, 16, peak_ratio=True)[k]) for k in KEYS2], want(2), "frames.get_piv")
    same_bits([np.asarray(frames.get_piv(a, 16, peak_ratio=True, peak_exclusion=4, chunksize=2)[k]) for k in KEYS2], want(4), "frames.get_piv, radius")
    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(16, engine="hip", peak_ratio=True)
        same_bits([np.asarray(via[k]) for k in KEYS2], want(2), "wrapped accessor")
        via = rd.Frames(a).get_piv(**{"window_size": 16, "engine": "hip", "peak_ratio": True, "peak_exclusion": 4})
        same_bits([np.asarray(via[k]) for k in KEYS2], want(4), "wrapped accessor, keywords")
        with pytest.raises(ValueError, match=r"peak_exclusion must be a whole number in 1 \.\. 4"):
            rd.Frames(a).get_piv(16, engine="hip", peak_ratio=True, peak_exclusion=5)
        with pytest.raises(NotImplementedError, match="peak_ratio together with ensemble_corr=True"):
            rd.Frames(a).get_piv(16, engine="hip", peak_ratio=True, ensemble_corr=True)
    finally:
        plugin.uninstall()


# ---- 8. what it gains ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ref.SPARSE_SEEDS)
def test_peak_ratio_separates_wrong_vectors_better_than_s2n(gpu, seed):
    n, ov = ref.SPARSE_WINDOW
    u, v, cm, sn, p2 = piv.piv_pairs_peak2(ref.sparse_stack(seed), (n, n), (ov, ov))
    a_ratio, a_s2n = ref.auc_pair(u, v, p2[..., 3], sn)
    r = ref.sparse_ref(seed)
    print(seed, "AUC of the peak ratio %.3f, of s2n %.3f (reference: %.3f, %.3f)" % ((a_ratio, a_s2n) + ref.auc_pair(r["u"], r["v"], r["ratio"], r["s2n"])))
    assert a_ratio - a_s2n >= 0.05
