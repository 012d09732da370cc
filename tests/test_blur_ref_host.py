"""The float64 blur reference of tests/blur_ref.py on its own (no GPU): against scipy's mirror correlation, its non-finite supports from
index arithmetic, the restated dispatch rule, and the condition that its gate is passable at all -- the project's float32 oracle, a
correct float32 filter, stays inside it on every stack the GPU tests use (largest share of the gate: 0.223, printed by the test)."""
import numpy as np
import pytest

from oracle import filters_oracle as fo
from tests import blur_ref as br


def test_reference_is_scipy_mirror_correlation_in_float64():
    from scipy.ndimage import correlate1d

    rng = np.random.default_rng(3)
    for shape in ((37, 53), (5, 7), (1, 1), (1, 9), (9, 1)):            # (5, 7) at k = 31: far smaller than the halo
        img = (rng.random(shape) * 300 - 100).astype(np.float32)
        for ks in (1, 3, 5, 7, 9, 21, 31):
            k = fo.gaussian_kernel(ks).astype(np.float64)
            ref = correlate1d(correlate1d(img.astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
            got = br.blur(img, ks)
            assert got.dtype == np.float64 and got.shape == shape
            assert np.abs(got - ref).max() <= 1e-12 * 300, (shape, ks)                 # of the range: samples in [-100, 200)
    st = (rng.random((3, 9, 11)) * 255).astype(np.float64)               # stacks, and float64 frames are narrowed first
    assert np.array_equal(br.smooth(st, 2)[1], br.blur(st[1].astype(np.float32), 5))
    assert np.array_equal(br.edge_detect(st, 1, 4), br.blur(st, 9) - br.blur(st, 3))
    x = np.array([np.nan, -3.0, 0.5, 9.0, np.inf, -np.inf])
    assert np.array_equal(br.clip(x, -1.0, 2.0), np.array([np.nan, -1.0, 0.5, 2.0, 2.0, -1.0]), equal_nan=True)


def test_gate_values():
    assert br.gate(15, None, 1.0) == 36 * 2.0 ** -24 and abs(br.gate(15, None, 1.0) - 2.1e-6) < 0.05e-6
    assert br.gate(2, 4, 10.0) == (8 + 12 + 3) * 2.0 ** -24 * 10.0
    assert br.gate(2, 3, 255.0, np.uint8) == 0 and br.gate(3, None, 255.0, np.uint8) == 0 and br.gate(0, 2, 255.0, np.uint8) == 0
    assert br.gate(2, 4, 255.0, np.uint8) > 0 and br.gate(3, None, 255.0, np.float32) > 0
    fr = np.array([[[0.5, np.nan]], [[-300.0, np.inf]]])
    assert br.max_abs(fr).tolist() == [[[1.0]], [[300.0]]]


def _wrap(i, n):
    """BORDER_REFLECT_101 of one index, by walking (nothing shared with the reference's modular form)."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def _support(shape, y, x, R):
    """Outputs whose (2R + 1)^2 reflected support contains the sample (y, x)."""
    H, W = shape
    rows = np.array([any(_wrap(o + d, H) == y for d in range(-R, R + 1)) for o in range(H)])
    cols = np.array([any(_wrap(o + d, W) == x for d in range(-R, R + 1)) for o in range(W)])
    return rows[:, None] & cols[None, :]


@pytest.mark.parametrize("shape,pos", [((40, 45), (17, 20)), ((40, 45), (1, 2)), ((40, 45), (38, 44)), ((6, 9), (2, 3))])
def test_one_non_finite_sample_reaches_exactly_its_reflected_support(shape, pos):
    img = (np.random.default_rng(8).random(shape) * 200 - 50).astype(np.float32)
    for w in (0, 1, 3, 4, 10, 15):
        for bad in (np.nan, np.inf):
            a = img.copy()
            a[pos] = bad
            got = br.smooth(a[None], w)[0]
            sup = _support(shape, *pos, w)
            assert np.array_equal(np.isnan(got) if bad != bad else got == np.inf, sup), (w, bad)
            assert np.isfinite(got[~sup]).all()
    for w1, w2 in ((1, 2), (0, 4), (2, 4), (6, 10), (3, 12), (5, 5)):
        a = img.copy()
        a[pos] = np.nan
        assert np.array_equal(np.isnan(br.edge_detect(a[None], w1, w2)[0]), _support(shape, *pos, w2)), (w1, w2)     # the larger kernel's
        a[pos] = np.inf
        got = br.edge_detect(a[None], w1, w2)[0]
        inner, outer = _support(shape, *pos, w1), _support(shape, *pos, w2)
        assert np.array_equal(np.isnan(got), inner) and np.array_equal(got == np.inf, outer & ~inner), (w1, w2)      # Inf - Inf | Inf - finite
        assert np.isfinite(got[~outer]).all()


def test_non_finite_points_of_the_gpu_cases_have_disjoint_supports():
    T, H, W = br.NONFINITE_SHAPE
    for row, rmax in (("strip", 3), ("stripr", 10), ("ring", 15)):
        nans, pinf, ninf = br.nonfinite_points(row)
        for t in range(T):
            pts = [p[1:] for p in nans if p[0] == t]
            a, b = [p[1:] for p in pinf if p[0] == t][0], [p[1:] for p in ninf if p[0] == t][0]
            sa, sb = _support((H, W), *a, rmax), _support((H, W), *b, rmax)
            assert not (sa & sb).any()
            for p in pts:
                sp = _support((H, W), *p, rmax)
                assert not (sp & sa).any() and not (sp & sb).any(), (row, t, p)
        s = br.SEAM[row]
        assert {p[1] for p in nans} >= {s - 1, s} and {p[2] for p in nans} >= {63, 64}
        fr = br.nonfinite_stack(row, "float32")
        assert np.isnan(fr).sum() == len(nans) and (fr == np.inf).sum() == 2 and (fr == -np.inf).sum() == 2


def test_family_restates_the_dispatch_rule():
    assert [br.family(np.uint8, 2, None, W) for W in (8, 12, 13, 16)] == ["strip", "strip4", "strip", "strip4"]
    assert [br.family(np.float32, w, None, 64) for w in (3, 4, 5, 6, 10, 11, 15)] == ["strip", "stripr5", "stripr5", "stripr10", "stripr10",
                                                                                   "ring", "ring"]
    assert br.family(np.float32, 2, 4, 64) == "stripr5" and br.family(np.uint8, 2, 4, 64) == "stripr5"
    assert br.family(np.uint8, 2, 3, 16) == "strip4" and br.family(np.float64, 2, 3, 16) == "strip"
    assert br.family(np.uint8, 3, 3, 16) == "stripr5" and br.family(np.uint8, 0, 2, 16) == "stripr5"                  # not "unrolled"
    assert br.family(np.float32, 6, 10, 64) == "stripr10" and br.family(np.float32, 3, 12, 64) == "ring"
    for row, (windows, shapes) in br.TABLE.items():                                                                     # the table means what it says
        for shape, dtypes in shapes:
            for dt in dtypes:
                for w, fam in windows.items():
                    assert br.family(dt, *br.split(w), shape[2]) == fam, (row, shape, dt, w)
                    assert fam.startswith(row)


def test_float32_oracle_stays_inside_the_gate_on_every_gpu_case():
    """What the reference alone must pass: a correct float32 filter (the project's oracle: float32 throughout, no fused operations) is
    inside the derived gate on every stack of the GPU tests, and exact where the gate is equality."""
    worst = 0.0

    def check(kind, key, dt, w):
        nonlocal worst
        fr = br.STACKS[kind](key, dt)
        w1, w2 = br.split(w)
        with np.errstate(invalid="ignore"):
            got = fo.smooth(fr, w1) if w2 is None else fo.edge_detect(fr, w1, w2)
        masks, ratio = br.compare(got, br.reference(kind, key, dt, w), fr, w)
        assert masks and ratio <= 1.0, (kind, key, dt, w, ratio)
        worst = max(worst, ratio)

    for row, (windows, shapes) in br.TABLE.items():
        for shape, dtypes in shapes:
            for dt in dtypes:
                for w in windows:
                    check("table", shape, dt, w)
    for row in ("strip", "stripr", "ring"):
        for dt in br.F:
            for w in br.TABLE[row][0]:
                check("nonfinite", row, dt, w)
    for dt in br.F + br.U8:
        for w in (2, (2, 3), 4, (6, 10), 12, (11, 15)):
            check("frames", None, dt, w)
    print(f"float32 oracle: largest error / gate = {worst:.3f}")
    assert worst > 0.0                                                  # the gate is not vacuous: float32 does round
