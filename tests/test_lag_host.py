"""The per-window frame lag on the CPU: the numpy restatement of the integer predictor on hand-made fields,
the clip at the end of the stack, the argument checks and refusals, the parity inputs of tests/test_gpu_lag.py (tie shares, the lags
and the clamped offsets the adaptive inputs yield, how far their lag-1 fields are from a rounding boundary of the predictor), the halo
planner, and the benefit on the gentle river profile by the float64 reference."""
import numpy as np
import pytest

from pyorc_amd import velocimetry, window
from tests import lag_ref as ref
from tests import multipass_ref as mp

FORMS = ("int", "array", "adaptive")


# ---- 1. the predictor restatement on hand-made fields -------------------------------------------------------------------------------------
def hand(k_max=4, target=None, clamp=True):
    u, v = ref.hand_fields()
    return ref.predict_lag(u, v, ref.HAND_DIM, ref.HAND_N, ref.HAND_OV, ref.HAND_T, k_max, target, clamp)


def test_predictor_by_hand():
    u, v = ref.hand_fields()
    lag, sh = hand(k_max=8, target=4.0)
    assert lag.dtype == np.uint8 and sh.dtype == np.int16 and lag.shape == u.shape and sh.shape == u.shape + (2,)
    # an empty neighbourhood: median 0 -> mag 0 -> the largest lag the stack leaves, zero offset
    assert lag[0, 4, 5] == 5 and tuple(sh[0, 4, 5]) == (0, 0)
    # mag = 0 in the rows whose whole neighbourhood is exactly zero (row 0: rows 0 and 1): k = min(K, frames left), zero offsets
    assert (lag[2, 0] == 3).all() and not sh[2, 0].any()
    # one window worked by hand: pair 1, window (10, 7), far from the planted entries
    p, r, c = 1, 9, 3
    q = np.rint(np.float32(64) * u[p, r - 1:r + 2, c - 1:c + 2]).astype(np.int64).ravel()
    qv = np.rint(np.float32(64) * v[p, r - 1:r + 2, c - 1:c + 2]).astype(np.int64).ravel()
    m2u, m2v = 2 * int(np.sort(q)[4]), 2 * int(np.sort(qv)[4])
    k = min(max(512 // max(abs(m2u), abs(m2v), 1), 1), 8, ref.HAND_T - 1 - p)
    assert lag[p, r, c] == k and tuple(sh[p, r, c]) == ((k * m2v + 64) // 128, (k * m2u + 64) // 128)
    # a corner keeps 3 valid neighbours of 4 (its own vector is NaN): the middle one, doubled
    q = np.sort(np.rint(np.float32(64) * np.array([u[1, 0, 1], u[1, 1, 0], u[1, 1, 1]])).astype(np.int64))
    _, raw = hand(k_max=1, target=4.0, clamp=False)
    assert raw[1, 0, 0, 1] == (2 * q[1] + 64) // 128
    # rint is half to even on the exact 1 / 128 px: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert [int(np.rint(np.float32(64) * x)) for x in u[2, 8, 3:6]] == [0, 2, 2]
    # the clamp of q: a vector of 3e9 px counts as 32767 px and cannot overflow anything
    big = ref.predict_lag(np.full((1, 1, 1), 3.0e9, np.float32), np.zeros((1, 1, 1), np.float32), (16, 16), 16, 8, 9, 16, 8.0, clamp=False)
    assert big[0][0, 0, 0] == 1 and big[1][0, 0, 0, 1] == 32767


def test_end_of_stack_clip():
    lag, _ = hand(k_max=16, target=8.0)
    left = ref.HAND_T - 1 - np.arange(ref.HAND_T - 1)
    assert (lag <= left[:, None, None]).all() and (lag >= 1).all()
    assert (lag[-1] == 1).all() and lag[0].max() == 5             # the last pair has one frame left; the first one reaches the clip
    assert ref.table(3, 5, 4, (2, 3))[:, 0, 0].tolist() == [3, 3, 2, 1]
    assert ref.table(np.array([[1, 16], [4, 2]]), 6, 5, (2, 2))[:, 0, 1].tolist() == [5, 4, 3, 2, 1]
    # more frames behind the pairs (a chunk with its halo): the clip counts the frames of the call
    assert ref.table(3, 7, 4, (1, 1)).ravel().tolist() == [3, 3, 3, 3]


def test_the_frame_clamp_changes_offsets():
    lag, sh = hand(k_max=4, target=8.0)
    _, raw = hand(k_max=4, target=8.0, clamp=False)
    changed = (raw != sh).any(axis=-1)
    assert changed.any() and np.array_equal(sh, mp.clamp_shift(raw, ref.HAND_DIM, ref.HAND_N, ref.HAND_OV))
    assert changed[3, :, 0].all() and changed[3, :, -1].all() and changed[3, 0, :].all() and changed[0, -1, :].all()   # the planted edges
    y0, x0 = mp.grid_origins(ref.HAND_DIM, ref.HAND_N, ref.HAND_OV)
    assert ((y0[:, None] + sh[..., 0]) >= 0).all() and ((y0[:, None] + sh[..., 0]) <= ref.HAND_DIM[0] - ref.HAND_N).all()
    assert ((x0[None, :] + sh[..., 1]) >= 0).all() and ((x0[None, :] + sh[..., 1]) <= ref.HAND_DIM[1] - ref.HAND_N).all()


def test_target_and_k_max_steer_the_lag():
    u = np.full((1, 3, 3), 0.5, np.float32)
    v = np.zeros_like(u)
    for target, k_max, want in ((4.0, 16, 8), (4.0, 4, 4), (1.0, 16, 2), (0.4, 16, 1), (0.51, 16, 1), (8.0, 16, 16)):
        lag, sh = ref.predict_lag(u, v, (32, 32), 16, 8, 40, k_max, target)
        assert (lag == want).all(), (target, k_max)
        assert (sh[0, 1, 1] == (0, (want * 64 + 64) // 128)).all()


# ---- 2. arguments ------------------------------------------------------------------------------------------------------------------------
def test_lag_spec_checks():
    assert window.lag_spec(None, (32, 32)) is None and window.lag_spec(1, (24, 24)) is None       # today's path, any window
    s = window.lag_spec(3, (32, 32))
    assert (s.form, s.k, s.halo) == (window.LAG_UNIFORM, 3, 3)
    s = window.lag_spec(np.array([[1, 2], [4, 1]]), (16, 16), (2, 2))
    assert s.form == window.LAG_WINDOW and s.array.dtype == np.uint8 and s.halo == 4
    s = window.lag_spec("adaptive", (64, 64), None, 8)
    assert (s.form, s.k, s.target128, s.halo) == (window.LAG_ADAPTIVE, 8, 128 * 16, 8)
    assert window.lag_spec("adaptive", (16, 16), None, 4, 0.3).target128 == 38
    for bad in (0, 17, -1, True, 2.0, "fast", np.ones((2, 2)), np.ones((2, 2, 2), int), np.ones(4, int)):
        with pytest.raises(ValueError, match="pair_step"):
            window.lag_spec(bad, (32, 32), (2, 2))
    for bad in (np.zeros((2, 2), int), np.full((2, 2), 17)):
        with pytest.raises(ValueError, match=r"1 \.\. 16"):
            window.lag_spec(bad, (32, 32), (2, 2))
    with pytest.raises(ValueError, match="grid's shape"):
        window.lag_spec(np.ones((3, 2), int), (32, 32), (2, 2))
    for ws in ((24, 24), (32, 16), (128, 128)):
        for ps in (2, np.ones((2, 2), int), "adaptive"):
            with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
                window.lag_spec(ps, ws, (2, 2))
    for bad in (0, 17, 2.5, None):
        with pytest.raises(ValueError, match="pair_step_max"):
            window.lag_spec("adaptive", (32, 32), None, bad)
    for bad in (0, -1.0, 16.5, "x", np.nan):
        with pytest.raises(ValueError, match="pair_step_target"):
            window.lag_spec("adaptive", (32, 32), None, 4, bad)
    with pytest.raises(ValueError, match="pair_step_target"):
        window.lag_spec(3, (32, 32), None, 4, 2.0)


REFUSED = dict(ensemble_corr=True, ensemble_window=4, coarse_passes=[64], deform_passes=1, spectral_filter="spof",
               image_mask=np.ones((96, 131), bool), peak_ratio=True, validate=True, search_area_size=(64, 64), devices=[0])


@pytest.mark.parametrize("kw", sorted(REFUSED))
@pytest.mark.parametrize("pair_step", [2, "adaptive"])
def test_get_ffpiv_refusals_name_both_keywords(kw, pair_step):
    a = ref.pass_stack(32)
    y, x = (np.arange(q) for q in ref.grid_shape(32))
    args = dict(window_size=(32, 32), overlap=(16, 16), search_area_size=(32, 32), res_y=0.01, res_x=0.01)
    args.update({kw: REFUSED[kw]})
    if kw == "ensemble_window":
        args["ensemble_corr"] = True
    with pytest.raises(NotImplementedError, match="pair_step") as e:
        velocimetry.get_ffpiv(a, y, x, np.ones(len(a) - 1), pair_step=pair_step, **args)
    assert ("search_area_size" if kw == "search_area_size" else kw) in str(e.value)


class _LazyDouble:
    """The least a dask-backed stack shows the host code: a shape, slices, ``load()`` and a ``.data`` that is no ndarray."""

    def __init__(self, a, loads):
        self._a, self.loads, self.dtype, self.shape, self.data = a, loads, a.dtype, a.shape, object()

    def __len__(self):
        return len(self._a)

    def __getitem__(self, key):
        return _LazyDouble(self._a[key], self.loads) if isinstance(key, slice) else self._a[key]

    def load(self):
        self.loads.append(self.shape)
        return self._a


@pytest.mark.parametrize("pair_step", [2, "adaptive", np.full((5, 7), 3)], ids=["int", "adaptive", "array"])
def test_a_lazy_stack_is_refused_before_anything_is_loaded(pair_step):
    """What a real pyorc hands the wrapped accessor is dask-backed: the refusal users meet first.  Both doubles -- the minimal one and the
    lazy stack of the drop-in suites, whose graph counts every block it computes -- are refused by name, and nothing was computed."""
    from tests import lazy_doubles

    a = ref.pass_stack(32)
    y, x = (np.arange(q) for q in ref.grid_shape(32))
    kw = dict(window_size=(32, 32), overlap=(16, 16), search_area_size=(32, 32), res_y=0.01, res_x=0.01, pair_step=pair_step)
    loads = []
    with pytest.raises(NotImplementedError, match="pair_step") as e:
        velocimetry.get_ffpiv(_LazyDouble(a, loads), y, x, np.ones(len(a) - 1), **kw)
    assert "lazy" in str(e.value) and loads == []
    lazy = lazy_doubles.from_frames(a, block=3).map_time(lambda blk: blk, "touch")
    assert velocimetry._is_lazy(lazy)
    with pytest.raises(NotImplementedError, match="pair_step") as e:
        velocimetry.get_ffpiv(lazy, y, x, np.ones(len(a) - 1), **kw)
    assert "lazy" in str(e.value) and lazy.calls == {}
    # the other refusals and the argument errors come first, as for a materialised stack, and still load nothing
    with pytest.raises(NotImplementedError, match="pair_step together with peak_ratio"):
        velocimetry.get_ffpiv(lazy, y, x, np.ones(len(a) - 1), peak_ratio=True, **kw)
    with pytest.raises(ValueError, match="pair_step_max"):
        velocimetry.get_ffpiv(lazy, y, x, np.ones(len(a) - 1), pair_step_max=0, **kw)
    assert lazy.calls == {} and loads == []


def test_shard_refuses_a_lag():
    from pyorc_amd import shard

    for call in (lambda ps: shard.sharded_piv(lambda a, b: None, 6, (32, 32), (16, 16), None, pair_step=ps),
                 lambda ps: shard.sharded_piv_dev(None, 6, (32, 32), (16, 16), None, pair_step=ps)):
        for ps in (2, "adaptive", np.ones((2, 2), int)):
            with pytest.raises(NotImplementedError, match=r"pair_step with pyorc_amd\.shard"):
                call(ps)


def test_get_ffpiv_argument_errors_come_before_any_gpu_work():
    a = ref.pass_stack(32)
    y, x = (np.arange(q) for q in ref.grid_shape(32))
    kw = dict(overlap=(16, 16), res_y=0.01, res_x=0.01)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        velocimetry.get_ffpiv(a, np.arange(7), np.arange(9), np.ones(6), window_size=(24, 24), search_area_size=(24, 24), pair_step=2, **{**kw, "overlap": (12, 12)})
    for bad in dict(pair_step=17), dict(pair_step="adaptive", pair_step_max=0), dict(pair_step="adaptive", pair_step_target=17.0), \
            dict(pair_step=np.ones((2, 2), int)):
        with pytest.raises(ValueError, match="pair_step"):
            velocimetry.get_ffpiv(a, y, x, np.ones(6), window_size=(32, 32), search_area_size=(32, 32), **kw, **bad)


# ---- 3. the planner's halos ----------------------------------------------------------------------------------------------------------------
def test_lagged_slices_carry_a_halo_of_the_largest_lag():
    # pairs [a, b) of a chunk, frames [a, min(b + halo, n_frames)): the halo shrinks at the end of the stack, never below frame b
    for n_frames, chunk_pairs, halo in ((12, 3, 4), (12, 5, 1), (7, 1, 3), (7, 2, 16), (30, 7, 8)):
        base = [(p, min(p + chunk_pairs, n_frames - 1) + 1) for p in range(0, n_frames - 1, chunk_pairs)]
        got = velocimetry.lagged_slices(base, n_frames, halo)
        assert [(a, p) for a, p, _ in got] == [(a, b - 1 - a) for a, b in base]                       # the same pairs
        for (a, p, end) in got:
            assert end == min(a + p + halo, n_frames) and end >= a + p + 1
        assert sum(p for _, p, _ in got) == n_frames - 1
    assert velocimetry.lagged_slices([(0, 4), (3, 7)], 7, 1) == [(0, 3, 4), (3, 3, 7)]                  # a lag of 1: today's slices
    # the default of aligned_slices is untouched
    assert velocimetry.aligned_slices(10, 4, 1) == [(0, 4), (3, 7), (6, 10)]


def test_the_halo_counts_in_the_memory_of_a_launch():
    dim, ws, ov = (1080, 1920), (32, 32), (16, 16)
    plain = window.required_memory(n_frames=11, dim_size=dim, window_size=ws, overlap=ov, dtype=np.uint8)
    spec = window.lag_spec("adaptive", ws, None, 8)
    lagged = window.lag_required_memory(10, 8, dim, ws, ov, np.uint8, spec)
    n_win = int(np.prod(window.get_array_shape(dim, ws, ov)))
    # 10 pairs + 8 halo frames, one lag byte and two int16 per window and pair, and -- adaptive -- nothing more: pass 0 writes the result block
    assert lagged >= window.required_memory(n_frames=18, dim_size=dim, window_size=ws, overlap=ov, dtype=np.uint8) + 10 * n_win * 5
    assert lagged > plain


# ---- 4. the parity inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.LAG_WINDOWS)
def test_parity_inputs(n):
    m, ov, dim = ref.PASS_CASES[n]
    for form in FORMS:
        for signal in (False, True):
            r = ref.parity_ref(n, form, np.uint8, signal)
            assert r["tie"].mean() <= 0.01, (form, signal)
            assert np.isfinite(r["u"]).mean() >= 0.5, (form, signal)
    assert set(np.unique(ref.window_lags(n))) == {1, 2, 3, 4}
    r = ref.parity_ref(n, "int")
    assert r["lag"][:, 0, 0].tolist() == [3, 3, 3, 3, 2, 1]
    # the signal stack: the threshold takes windows out, and not the same ones at every lag
    s1, s3 = ref.parity_ref(n, "array", np.uint8, True), ref.parity_ref(n, "int", np.uint8, True)
    assert 0.05 <= np.isnan(s3["u"]).mean() <= 0.6 and (np.isnan(s1["corr"]) != np.isnan(s3["corr"])).any()
    # the adaptive input: at least three distinct lags, at least one offset the frame clamp changes
    r = ref.parity_ref(n, "adaptive")
    assert len(np.unique(r["lag"])) >= 3
    lag, raw = ref.predict_lag(r["pass0"]["u"], r["pass0"]["v"], dim, m, ov, ref.PASS_T, *ref.ADAPTIVE[n], clamp=False)
    assert np.array_equal(lag, r["lag"]) and (raw != r["shift"]).any() and np.array_equal(mp.clamp_shift(raw, dim, m, ov), r["shift"])


def off_the_boundaries(r, dim, m, ov, n_frames, k_max, target):
    """The GPU's pass 0 is within 1e-4 (of max(|x|, 0.05)) of the reference's: moved by twice that in every direction, the lag-1 field of an
    adaptive input must still give the same lags and offsets, or the comparison of integers on the GPU would rest on luck."""
    u, v = r["pass0"]["u"], r["pass0"]["v"]
    base = ref.predict_lag(u, v, dim, m, ov, n_frames, k_max, target)
    assert np.array_equal(base[0], r["lag"]) and np.array_equal(base[1], r["shift"])
    du, dv = 2e-4 * np.maximum(np.abs(u), 0.05), 2e-4 * np.maximum(np.abs(v), 0.05)
    for su in (-1, 1):
        for sv in (-1, 1):
            got = ref.predict_lag(u + su * du, v + sv * dv, dim, m, ov, n_frames, k_max, target)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (su, sv)


@pytest.mark.parametrize("n", ref.LAG_WINDOWS)
@pytest.mark.parametrize("case", ["u8", "f32", "f64", "signal"])
def test_adaptive_parity_inputs_sit_off_the_predictor_s_rounding_boundaries(n, case):
    m, ov, dim = ref.PASS_CASES[n]
    dtype = {"u8": np.uint8, "f32": np.float32, "f64": np.float64, "signal": np.uint8}[case]
    off_the_boundaries(ref.parity_ref(n, "adaptive", dtype, case == "signal"), dim, m, ov, ref.PASS_T, *ref.ADAPTIVE[n])


@pytest.mark.parametrize("n", ref.LAG_WINDOWS)
def test_table_inputs(n):
    m, ov, dim = ref.PASS_CASES[n]
    lag, sh = ref.table_case(n)
    r = ref.table_ref(n)
    assert r["tie"].mean() <= 0.01 and np.isfinite(r["u"]).mean() >= 0.5
    assert r["lag"][0, 0, 0] == 1 and r["lag"][1, -1, -1] == ref.PASS_T - 1 - 1        # 0 -> 1, 200 -> the frames left
    assert (r["lag"] != lag).sum() == 2 and (r["shift"] != sh).any() and r["lag"].shape[0] == ref.TABLE_PAIRS < ref.PASS_T - 1


@pytest.mark.parametrize("name", sorted(ref.SMALL_GRIDS))
def test_small_grid_inputs(name):
    n, ov, dim = ref.SMALL_GRIDS[name]
    for form in ("array", "adaptive"):
        r = ref.small_ref(name, form)
        assert r["tie"].mean() <= 0.01 and np.isfinite(r["u"]).mean() >= 0.5, form
    off_the_boundaries(ref.small_ref(name, "adaptive"), dim, n, ov, ref.SMALL_T, ref.SMALL_K, None)
    if name == "odd job count":
        assert r["u"].size % 8 != 0 and r["u"].size == 100


# ---- 5. the benefit on the gentle river profile ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ov", ref.PROFILE_CASES)
def test_adaptive_lags_cut_the_error_of_slow_windows(n, ov):
    lag1, adaptive = ref.profile_ref(n, ov, False), ref.profile_ref(n, ov, True)
    e1, ea = ref.slow_median_error(lag1["u"], lag1["v"], n, ov), ref.slow_median_error(adaptive["u"], adaptive["v"], n, ov)
    print(f"{n} @ {ov}: slow-window median error {e1:.5f} px/frame at lag 1, {ea:.5f} adaptive (K = {ref.PROFILE_K}): {ea / e1:.3f} x")
    want1, wanta = ref.PROFILE_MEDIANS[(n, ov)]
    assert abs(e1 - want1) <= 0.01 * want1 and abs(ea - wanta) <= 0.01 * wanta       # the constants the documents quote
    assert ea <= 0.5 * e1
    _, slow = ref.profile_truth(n, ov)
    P = ref.PROFILE_T - 1 - ref.PROFILE_TAIL
    k = adaptive["lag"][:P]
    assert slow.any() and not slow.all() and k[:, slow].min() >= 3 and k[:, slow].mean() > k[:, ~slow].mean() + 1       # the slow windows got the long lags
