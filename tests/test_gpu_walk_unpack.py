"""The un-packing phase of the walking kernels (piv_fft_impl.h, walk_iteration) runs its ky = 0 .. N/2 steps in batches: the exchanges
with the mirrored lane of a whole batch are requested before the batch's first step.  The batch cuts the N/2 + 1 steps differently
per window size, so the shapes here are the smallest on which a cut can go wrong: windows of 6, 16, 24, 32, 62 and 64 = 4, 9, 13, 17,
32 and 33 steps -- fewer steps than a batch, an exact multiple, a ragged last batch --, frames of 3 x 3 windows at 50 % overlap (25
window positions), uint8 at every size and float32 / float64 at 32.

Per shape: the per-timestep results and planes, and the ensemble results, against the float64 oracle through the gates of
tests/test_gpu_parity.py (same functions, same tolerances); and bit-equality -- uint32 views, NaN payloads included -- between one
launch over all pairs and the same pairs launched in two pieces cut on an anchor, the library's documented invariant.  7 pairs
placed 3 before and 4 behind an anchor: the one launch walks a 3-pair and a 4-pair segment (two iterations of two frames, then
two and one of a single frame), the two pieces the same two segments.  Once 80 pairs at 32, across the anchors at 25, 50 and 75.
A zero-variance window and a NaN sample put the dead / skip flags that ride on the carry across the batch boundaries.
"""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import piv_oracle as po
from pyorc_amd.synth import particle_stack
from tests.test_gpu_parity import TOL, check_against_oracle, rel_err

pytestmark = pytest.mark.gpu

PAIRS = 7
SHAPES = [(6, np.uint8), (16, np.uint8), (24, np.uint8), (32, np.uint8), (32, np.float32), (32, np.float64), (62, np.uint8), (64, np.uint8)]
IDS = [f"{n}-{np.dtype(d).name}" for n, d in SHAPES]
_stacks = {}


def stack(n, dtype, pairs=PAIRS):
    """(pairs + 1, 3 n, 3 n) frames, made once per shape and never written to."""
    key = (n, np.dtype(dtype).name, pairs)
    if key not in _stacks:
        fr = particle_stack(pairs + 1, 3 * n, 3 * n, seed=400 + n, density=0.08)
        if dtype != np.uint8:
            fr = (fr.astype(dtype) - 31.25) * 0.5   # signed, non-integer
        fr.setflags(write=False)
        _stacks[key] = fr
    return _stacks[key]


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def assert_same_bits(whole, parts, what):
    for k, w in enumerate(whole):
        joined = np.concatenate([p[k] for p in parts], axis=0)
        assert w.shape == joined.shape, (what, k)
        assert np.array_equal(bits(w), bits(joined)), (what, ("u", "v", "corr", "s2n", "planes")[k])


def one_against_two_launches(fr, n, cut_behind, planes=True, thr=None):
    """fr's pairs with the anchor `cut_behind` pairs after the first one: one launch against two cut there."""
    import pyorc_amd
    from pyorc_amd import window

    ws, ov = (n, n), (n // 2, n // 2)
    A = window.chunk_alignment(ws, fr.shape[1:], ov)
    assert A >= cut_behind
    off = A - cut_behind
    whole = pyorc_amd.piv_pairs(fr, ws, ov, thr, return_planes=planes, pair_offset=off)
    parts = [pyorc_amd.piv_pairs(fr[:cut_behind + 1], ws, ov, thr, return_planes=planes, pair_offset=off),
             pyorc_amd.piv_pairs(fr[cut_behind:], ws, ov, thr, return_planes=planes, pair_offset=A)]
    assert_same_bits(whole, parts, (n, fr.dtype.name, planes, thr))
    return whole


# the kernels are instantiated per (planes written or not, signal score or not), and each instantiation has a batch of its own
THR = 0.05
VARIANTS = [(True, None), (False, None), (True, THR), (False, THR)]


def gate_without_planes(fr, n, thr):
    """check_against_oracle's comparisons for a launch that writes no planes (another kernel instantiation)."""
    import pyorc_amd

    ws, ov = (n, n), (n // 2, n // 2)
    u, v, cm, sn = pyorc_amd.piv_pairs(fr, ws, ov, thr)
    uo, vo, cmo, sno, cond = c_oracle.piv_pairs(fr, ws, ov, thr, return_cond=True)
    ok = ~c_oracle.exact_tie(cond, cmo)
    assert ok.mean() >= 0.9
    for name, g, r in (("u", u, uo), ("v", v, vo)):
        assert np.array_equal(np.isnan(g)[ok], np.isnan(r)[ok]), name
        assert rel_err(g[ok], r[ok].astype(np.float64)) <= TOL, name
    for name, g, r in (("corr", cm, cmo), ("s2n", sn, sno)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), name
        assert rel_err(g, r.astype(np.float64)) <= TOL, name


@pytest.mark.parametrize("n,dtype", SHAPES, ids=IDS)
def test_per_timestep_vs_oracle(gpu, n, dtype):
    fr = stack(n, dtype)
    for thr in (None, THR):
        check_against_oracle(fr, (n, n), (n // 2, n // 2), thr=thr)
        gate_without_planes(fr, n, thr)


@pytest.mark.parametrize("n,dtype", SHAPES, ids=IDS)
def test_one_launch_equals_two_cut_on_the_anchor(gpu, n, dtype):
    for planes, thr in VARIANTS:
        one_against_two_launches(stack(n, dtype), n, 3, planes, thr)


@pytest.mark.parametrize("n,dtype", SHAPES, ids=IDS)
def test_ensemble_vs_oracle(gpu, n, dtype):
    from pyorc_amd import frames as F

    fr = stack(n, dtype)
    for thr in (None, THR):
        kw = dict(ensemble_corr=True, corr_min=0.1, s2n_min=1.5, signal_threshold=thr)
        got = F.get_piv(fr, n, **kw)
        ref = po.get_ffpiv(fr, np.ones(PAIRS), (n, n), (n // 2, n // 2), 1.0, 1.0, **kw)
        for k in ("v_x", "v_y", "corr", "s2n"):
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (k, thr)
            assert rel_err(got[k], np.asarray(ref[k], dtype=np.float64)) <= TOL, (k, thr)


def ensemble_state(fr, n, bounds):
    import pyorc_amd.piv as P

    ens = P.Ensemble(fr.shape[1:], (n, n), (n // 2, n // 2))
    try:
        cms = [np.concatenate(ens.accumulate(fr[a:b + 1], 0.1, 1.5), axis=1) for a, b in zip(bounds, bounds[1:])]
        return (np.concatenate(cms), *ens.export_state())
    finally:
        ens.close()


def test_80_pairs_across_the_anchors(gpu):
    """32 x 32, 80 pairs: a job walks past pairs 25, 50 and 75; per time step and as an ensemble, one launch against two cut at 75."""
    import pyorc_amd
    from pyorc_amd import window

    n, P = 32, 80
    fr = stack(n, np.uint8, P)
    ws, ov = (n, n), (n // 2, n // 2)
    assert 75 % window.chunk_alignment(ws, fr.shape[1:], ov) == 0
    check_against_oracle(fr, ws, ov)
    whole = pyorc_amd.piv_pairs(fr, ws, ov, return_planes=True)
    parts = [pyorc_amd.piv_pairs(fr[:76], ws, ov, return_planes=True), pyorc_amd.piv_pairs(fr[75:], ws, ov, return_planes=True, pair_offset=75)]
    assert_same_bits(whole, parts, "80 pairs")
    one, two = ensemble_state(fr, n, [0, P]), ensemble_state(fr, n, [0, 75, P])
    for a, b in zip(one, two):
        assert np.array_equal(bits(a), bits(b))


def test_ensemble_64_one_launch_equals_two(gpu):
    """The 64 x 64 ensemble kernel (its partial sum travels through the transpose tile): 28 pairs, cut on the grid's anchor."""
    from pyorc_amd import window

    n, P = 64, 28
    fr = stack(n, np.uint8, P)
    A = window.chunk_alignment((n, n), fr.shape[1:], (n // 2, n // 2))
    assert 0 < A < P
    one, two = ensemble_state(fr, n, [0, P]), ensemble_state(fr, n, [0, A, P])
    for a, b in zip(one, two):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n", [32, 64])
def test_zero_variance_window_rides_the_carry(gpu, n):
    """A constant window in the frames around the cut: dead flags of both pairs of an iteration and of the carried frame."""
    fr = stack(n, np.uint8).copy()
    fr[2:5, :n, :n] = 9           # window (0, 0) of frames 2, 3, 4: pairs 1 .. 4 have a zero-variance side
    u, v, cm, sn = check_against_oracle(fr, (n, n), (n // 2, n // 2))
    assert (cm[1:5, 0, 0] == 0.0).all() and np.isnan(u[1:5, 0, 0]).all() and np.isnan(sn[1:5, 0, 0]).all()
    assert (cm[0, 0, 0] > 0.0) and (cm[5, 0, 0] > 0.0)
    whole = one_against_two_launches(fr, n, 3)
    assert (whole[2][1:5, 0, 0] == 0.0).all() and np.isnan(whole[0][1:5, 0, 0]).all()


def test_nan_sample_float32(gpu):
    """One NaN sample in frame 3 of a float32 stack, inside window (0, 0) only: pairs 2 and 3 of that window are skipped (NaN in all
    four results), and the skip flag of frame 3 is carried from the 3-pair segment's last iteration into the next segment's first.
    Every other window is a job of its own and keeps the bits of the clean stack; the other pairs of window (0, 0) share an inverse
    transform with a skipped plane, which rounds into theirs: finite, and the clean stack's corr / s2n to 1e-5 (the bound
    tests/test_gpu_parity.py, assert_same_to_rounding, sets for two runs that share transforms differently)."""
    import pyorc_amd
    from pyorc_amd import window

    n = 32
    clean = stack(n, np.float32)
    fr = clean.copy()
    fr[3, 5, 7] = np.nan          # row and column < 16
    ws, ov = (n, n), (n // 2, n // 2)
    ref = pyorc_amd.piv_pairs(clean, ws, ov, pair_offset=window.chunk_alignment(ws, fr.shape[1:], ov) - 3)
    got = one_against_two_launches(fr, n, 3)
    hit = np.zeros(ref[0].shape, bool)
    hit[2:4, 0, 0] = True
    same_job = np.zeros_like(hit)
    same_job[:, 0, 0] = True
    for k, name in enumerate(("u", "v", "corr", "s2n")):
        assert np.isnan(got[k][hit]).all(), name
        assert np.array_equal(bits(got[k])[~same_job], bits(ref[k])[~same_job]), name
        assert np.isfinite(got[k][same_job & ~hit]).all(), name
    for k in (2, 3):
        assert rel_err(got[k][same_job & ~hit], ref[k][same_job & ~hit].astype(np.float64)) <= 1e-5
