"""Sliding ensemble, host side (CPU): argument validation, the block / output / label arithmetic, the planner on multiples of the
stride, the block store in ``required_memory``, and the CPU checks of the inputs tests/test_gpu_sliding.py relies on (tie shares of
the reference, and that the count-filter case really has outputs with differing NaN masks)."""
import numpy as np
import pytest

from pyorc_amd import piv, shard, velocimetry, window
from oracle import piv_oracle as po
from tests import recipe_doubles as rd
from tests import sliding_ref as ref


def ffpiv(a, **kw):
    n = len(a)
    return velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(n - 1), (32, 32), (16, 16), (32, 32), 1.0, 1.0, **kw)


@pytest.mark.parametrize("M,s", [(4, 3), (4, 0), (2, 4), (0, None), (4, -2)])
def test_window_and_stride_must_divide(M, s):
    a = np.zeros((9, 64, 64), np.uint8)
    with pytest.raises(ValueError, match="need 1 <= ensemble_stride <= ensemble_window and ensemble_window % ensemble_stride == 0"):
        ffpiv(a, ensemble_corr=True, ensemble_window=M, ensemble_stride=s)
    with pytest.raises(ValueError, match="ensemble_window % ensemble_stride == 0"):
        piv.Ensemble((64, 64), (32, 32), (16, 16), sliding=(M, s))


def test_keywords_need_ensemble_mode_and_whole_numbers():
    a = np.zeros((9, 64, 64), np.uint8)
    with pytest.raises(ValueError, match="need ensemble_corr=True"):
        ffpiv(a, ensemble_window=4)
    with pytest.raises(ValueError, match="ensemble_stride needs ensemble_window"):
        ffpiv(a, ensemble_corr=True, ensemble_stride=2)
    with pytest.raises(ValueError, match="ensemble_window must be a whole number of frame pairs"):
        ffpiv(a, ensemble_corr=True, ensemble_window=4.5)
    assert window.sliding_spec(True, 6, None) == (6, 6) and window.sliding_spec(True, np.int64(6), 2) == (6, 2)
    assert window.sliding_spec(False, None, None) is None


def test_too_few_pairs_for_one_window():
    with pytest.raises(ValueError, match="ensemble_window 10 needs at least 10 pairs, got 8"):
        ffpiv(np.zeros((9, 64, 64), np.uint8), ensemble_corr=True, ensemble_window=10, ensemble_stride=5)
    with pytest.raises(ValueError, match="ensemble_window 4 needs at least 4 pairs, got 3"):
        window.sliding_outputs(3, 4, 1)


class Lazy:
    """A stack that materialises on ``load()`` (no ``.data``)."""

    def __init__(self, a):
        self._a, self.dtype, self.shape = a, a.dtype, a.shape

    def __len__(self):
        return len(self._a)

    def __getitem__(self, k):
        return self._a[k] if isinstance(k, (int, np.integer)) else Lazy(self._a[k])

    def load(self):
        return self._a


def test_what_is_not_in_this_mode_raises_not_implemented():
    a = np.zeros((9, 64, 64), np.uint8)
    with pytest.raises(NotImplementedError, match=r"ensemble_window with devices=\[0, 1\] is not implemented"):
        ffpiv(a, ensemble_corr=True, ensemble_window=4, ensemble_stride=2, devices=[0, 1])
    with pytest.raises(NotImplementedError, match="ensemble_window with a lazy stack is not implemented"):
        ffpiv(Lazy(a), ensemble_corr=True, ensemble_window=4, ensemble_stride=2)
    with pytest.raises(NotImplementedError, match="ensemble_corr=True with search_area_size != window_size"):
        velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(8), (12, 12), (16, 16), (32, 32), 1.0, 1.0, ensemble_corr=True,
                              ensemble_window=4)

    class Sliding:
        sliding = (4, 2)

    class Comm:
        rank, world = 0, 1

    with pytest.raises(NotImplementedError, match="not implemented for pyorc_amd.shard"):
        shard.sharded_ensemble(lambda f0, f1: a[f0:f1], 8, Sliding, 0.1, 1.5, 0.2, Comm())


def test_other_engines_do_not_know_the_keywords(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((9, 64, 64), np.uint8))
        with pytest.raises(TypeError, match="ensemble_window / ensemble_stride is a keyword of engine='hip' only"):
            acc.get_piv(32, engine="numba", ensemble_corr=True, ensemble_window=4, ensemble_stride=2)
        with pytest.raises(TypeError, match="ensemble_window is a keyword of engine='hip' only"):
            acc.get_piv(32, engine="numba", ensemble_corr=True, ensemble_window=4)
    finally:
        plugin.uninstall()


def test_blocks_outputs_labels_and_trailing_pairs():
    assert window.sliding_outputs(12, 4, 2) == (6, 5)
    assert window.sliding_outputs(13, 4, 2) == (6, 5)        # a trailing pair fills no block
    assert window.sliding_outputs(12, 6, 1) == (12, 7) and window.sliding_outputs(12, 6, 6) == (2, 2)
    assert window.sliding_outputs(14, 6, 6) == (2, 2) and window.sliding_outputs(12, 12, 12) == (1, 1)
    t = np.cumsum(np.r_[0.0, np.linspace(0.03, 0.05, 13)])   # uneven frame times: 14 frames, 13 pairs
    dt = np.diff(t)
    labels, dts = velocimetry.sliding_labels(t, dt, 4, 2, 5)
    for j in range(5):
        assert labels[j] == pytest.approx(t[1:][2 * j:2 * j + 4].mean(), rel=1e-15)
        assert dts[j] == pytest.approx(dt[2 * j:2 * j + 4].mean(), rel=1e-15)
    r = ref.sliding_piv(np.zeros((14, 40, 40), np.uint8), dt, (32, 32), (16, 16), 4, 2, time=t)
    assert np.array_equal(r["time"], labels) and np.array_equal(r["dt"], dts) and r["v_x"].shape == (5, 1, 1)


def test_planner_cuts_chunks_on_multiples_of_the_stride(monkeypatch):
    dim = (70, 90)
    monkeypatch.setattr(window, "available_memory", lambda: 1 << 40)
    args = (dim, (32, 32), (16, 16), np.uint8)
    for n_frames, cs, s in ((25, 7, 2), (25, 10, 3), (26, None, 4), (13, 5, 6), (40, 4, 5)):
        slices = velocimetry.plan_sliding_slices(n_frames, *args, cs, 4, "hip", 12, s)
        assert slices[0][0] == 0 and slices[-1][1] == n_frames
        assert all(a % s == 0 for a, _ in slices) and all(p[1] - 1 == q[0] for p, q in zip(slices, slices[1:]))
        if cs is not None and cs - 1 >= s:
            assert max(b - a for a, b in slices) <= cs
    assert velocimetry.plan_sliding_slices(26, *args, None, 4, "hip", 12, 4) == [(0, 26)]
    assert window.chunk_alignment((32, 32), dim, (16, 16)) == 25                    # the other modes keep theirs


def test_a_block_that_does_not_fit_one_call_is_refused_by_the_planner(monkeypatch):
    dim, args = (70, 90), ((70, 90), (32, 32), (16, 16), np.uint8)
    store = window.sliding_store_bytes(6, dim, (32, 32), (16, 16))                  # 24 pairs in blocks of 4
    room = window.required_memory(4, *args[:3], sliding_blocks=6)                   # 3 pairs next to the store fit, a block of 4 does not
    assert room > store
    monkeypatch.setattr(window, "available_memory", lambda: room)
    with pytest.raises(ValueError, match=r"ensemble_stride 4: a block of 4 pairs \(5 frames, \d+ bytes with the block store of 6 blocks\) does not fit one call"):
        velocimetry.plan_sliding_slices(25, *args, 4, 1, "hip", 12, 4)                # (the plan: 3 pairs per call)
    monkeypatch.setattr(velocimetry, "MAX_WINDOWS_PER_LAUNCH", 40)                  # 12 windows per pair: 3 pairs per launch
    monkeypatch.setattr(window, "available_memory", lambda: 1 << 40)
    with pytest.raises(ValueError, match="one launch takes 40 windows, this grid has 12 per pair; use a smaller ensemble_stride"):
        velocimetry.plan_sliding_slices(25, *args, None, 1, "hip", 12, 4)
    assert velocimetry.plan_sliding_slices(25, *args, None, 1, "hip", 12, 3) == [(0, 4), (3, 7), (6, 10), (9, 13), (12, 16), (15, 19), (18, 22), (21, 25)]


def test_required_memory_counts_the_block_store():
    dim = (1080, 1920)
    plain = window.required_memory(101, dim, (32, 32), (16, 16))
    n_win = np.prod(window.get_array_shape(dim, (32, 32), (16, 16)))
    assert window.sliding_store_bytes(1, dim, (32, 32), (16, 16)) == n_win * (32 * 32 + 1) * 4 == 7854 * 1025 * 4   # 32.2 MB: "32 MB per block"
    assert window.required_memory(101, dim, (32, 32), (16, 16), sliding_blocks=10) == plain + 10 * n_win * 1025 * 4
    assert window.sliding_store_bytes(3, (70, 90), (12, 20), (6, 10)) == 3 * 10 * 8 * 241 * 4


# ---- the inputs of tests/test_gpu_sliding.py -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,M,s", ref.PARITY, ids=[f"{c}-{M}-{s}" for c, M, s in ref.PARITY])
def test_reference_ties_are_rare(case, M, s):
    for dtype in ref.DTYPES:
        r = ref.case_ref(case, dtype, M, s)
        assert r["tie"].mean() <= 0.01, (case, dtype, float(r["tie"].mean()))
        assert np.isfinite(r["v_x"]).mean() > 0.5, case           # the case measures something


def test_count_filter_case_has_outputs_with_differing_nan_masks():
    r = ref.blanked_ref()
    masks = np.isnan(r["v_x"]) & (r["count"] < 0.5 * 4)
    assert r["tie"].mean() <= 0.01
    assert masks[0].sum() == 0 or not np.array_equal(masks[0], masks[2])
    assert len({m.tobytes() for m in masks}) >= 2 and masks.any() and not masks.all(axis=(1, 2)).any()
    assert np.array_equal(r["count"] < 2, np.isnan(r["planes"]).all(axis=(-2, -1)).reshape(r["count"].shape))


def test_rescue_case_reference_ties_are_rare():
    r = ref.speckle_ref()
    assert r["v_x"].shape == (3, 11, 15) and r["tie"].mean() <= 0.01 and np.isfinite(r["v_x"]).mean() > 0.5
    (f0, f1), (g0, g1) = ref.RESCUE_CHUNKS                   # the second call starts inside output 1 and off pair 0, on a block
    _, _, M, s = ref.RESCUE
    assert f1 - 1 == g0 and g0 % s == 0 and s < g0 < s + M and g1 == len(ref.speckle_stack())


@pytest.mark.parametrize("mode", [0, 1])
def test_signal_case_drops_what_it_should_in_both_modes(mode):
    a, thr = ref.signal_stack(), ref.SIGNAL_THR
    r = ref.signal_ref(mode)
    assert r["tie"].mean() <= 0.01 and np.isfinite(r["v_x"]).mean() > 0.5
    assert np.isnan(r["v_x"][:, 0, 0]).all() and (r["count"][:, 0, 0] == 0).all()         # the empty corner, in every output
    stack = po.sliding_window_stack(a, (32, 32), (16, 16))
    if mode == 0:
        kept = np.array([po.signal_mask(stack[t], stack[t + 1], thr).sum() for t in range(12)])
        assert kept.max() == 11 and (kept[[5, 6]] == 4).all() and (np.delete(kept, [5, 6]) == 11).all()    # frame 6: two of four columns, and the window next to the corner
        assert not np.array_equal(r["count"], ref.signal_ref(1)["count"])                   # the modes differ on this stack
    else:
        with po.semantics(signal_mode=1):
            whole = po.signal_mask_stack(stack, thr)
            assert whole.sum() == 11 and not whole[0]
            for j in range(5):                           # an output's frames alone keep the same positions as the whole stack
                assert np.array_equal(po.signal_mask_stack(stack[2 * j:2 * j + 5], thr), whole), j


# ---- the inputs of tests/test_gpu_batch_loops.py ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.LOOP_CASES))
def test_loop_case_reference_ties_are_rare_and_its_calls_cut_where_they_should(case):
    """Measured: "long" and "stepped" tie share 0.0, 11 of 990 vectors NaN; "many" tie share 0.11 %, at most 0.61 % (one window) in one
    output.  On "stepped" the windows of the speckle part (columns 0 .. 6, the ones the float32 fit is ill-conditioned on) have another
    u from output to output: 77, 61, 77, 22 and 66 of the 77 move by more than 1e-4 px; on "long" none of them moves at all."""
    T, M, s, calls, stepped = ref.LOOP_CASES[case]
    r = ref.loop_ref(case)
    n_blk, n_out = window.sliding_outputs(T - 1, M, s)
    print(case, "ties:", float(r["tie"].mean()), "worst output:", float(r["tie"].mean(axis=(1, 2)).max()), "NaN:", int(np.isnan(r["v_x"]).sum()))
    assert r["v_x"].shape == (n_out, 11, 15) and r["tie"].mean() <= 0.01 and r["tie"].mean(axis=(1, 2)).max() <= 0.01
    assert np.isfinite(r["v_x"]).mean() > 0.9
    (f0, f1), (g0, g1) = calls
    assert f0 == 0 and f1 - 1 == g0 and g0 % s == 0 and g1 == T
    speckles = r["v_x"][:, :, :7]
    moved = (np.abs(np.diff(speckles, axis=0)) > 1e-4).sum(axis=(1, 2))
    print(case, "speckle windows that move from one output to the next:", moved.tolist())
    if case == "stepped":
        assert (moved >= 20).all()
    elif case == "long":
        assert not moved.any()                                # every pair moves 1 px: the fit cannot tell which pairs were summed
    else:
        assert moved.max() <= 3                               # "many": a few windows next to the particle part
    if M == 20:
        # the rescue's pair-blocks of 16: outputs 0 .. 3 straddle pair 16, output 4 pair 32; each call holds a full and a ragged block
        assert (n_blk, n_out) == (10, 6)
        assert all(j * s < 16 < j * s + M for j in range(4)) and 4 * s < 32 < 4 * s + M
        assert f1 - 1 > 16 and (f1 - 1) % 16 != 0 and g1 - 1 - g0 > 16 and (g1 - 1 - g0) % 16 != 0
    else:
        assert n_out == 16
