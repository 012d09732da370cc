"""CPU checks of the geometry sweep of the mode PIV kernels (tests/mode_geometry_inputs.py): that every grid is the intended one, that the
job counts reach the blocks they are meant to reach, and -- from the float64 references alone -- that the inputs suit the gates
tests/test_gpu_mode_geometry.py borrows.

Those gates cap the share of windows they set aside (exact ties: 1 %; fragile SPOF windows: 1 %; fragile second peaks: 5 %; the masked
gate sets nothing aside), which says nothing about a grid of two windows: one tie there is half the case.  So a geometry with fewer than
100 windows (pairs x rows x cols, what the gates count) holds NO tie and NO fragile window in any reference -- every mode, every sample
type, the signal-threshold stack included -- and a larger one stays within the caps; the masked references hold none anywhere.  The
seeds are 1000 + n + H + W, replaced where that formula's stack broke this rule (``mode_geometry_inputs.SEEDS`` lists what it broke).

Both classes of a mask (windows below ``k_min`` and finite ones) and of a signal threshold (skipped and kept windows) are asked of the
geometries with more than 10 windows in the grid: the windows of a smaller grid here are one window (1 x 1), near copies of one window
(stride 1: their origins lie within 7 px) or at most 3 x 3, and whether one of them falls on the other side is then an accident of the
seed, not a property of the geometry."""
import numpy as np
import pytest

from oracle import piv_oracle as po
from tests import deform_ref, masked_ref, peak2_ref, spof_ref
from tests import mode_geometry_inputs as mg
from tests import multipass_ref as mp

# rows x cols per window size: (dim - n) // (n - overlap) + 1 per axis, worked out by hand from the table of the sweep
GRIDS = {"one-window": {16: (1, 1), 32: (1, 1), 64: (1, 1)},
         "row-stride-1": {16: (1, 8), 32: (1, 8), 64: (1, 8)},
         "col-stride-1": {16: (6, 1), 32: (6, 1), 64: (6, 1)},
         "odd-stride": {16: (5, 8), 32: (3, 6), 64: (3, 5)},            # strides 5, 13, 29
         "ragged-0": {16: (2, 3), 32: (2, 3), 64: (2, 3)},
         "blocks": {16: (4, 11), 32: (2, 11), 64: (1, 11)},
         "asym": {16: (5, 3), 32: (3, 3), 64: (3, 3)},                  # strides (5, 15), (13, 31), (29, 63)
         "asym-T": {16: (3, 8), 32: (3, 13), 64: (3, 24)}}              # strides (n, 3)
CAPS = {"shifted": 0.01, "deformed": 0.01, "shifted-ensemble": 0.01, "spof": 0.01, "spof-ensemble": 0.01, "masked": 0.0, "peak2-1": 0.05,
        "peak2-q": 0.05}
SMALL = 100


def keys_of(n):
    return [k for k in mg.KEYS if k[1] == n]


# ---- grids and jobs ---------------------------------------------------------------------------------------------------------------------
def test_every_grid_is_the_intended_one():
    assert set(GRIDS) == set(mg.NAMES) and len(mg.KEYS) == 24
    for key in mg.KEYS:
        name, n = key
        g = mg.GEOMETRIES[key]
        assert mg.grid(key) == GRIDS[name][n], key
        assert max(g.dim) <= 385 and g.dim[0] * g.dim[1] <= 161 * 385, key     # small frames: the tallest is 195 x 133 (asym-T at 64 px)
        assert all(0 <= o < n for o in g.overlap)
        y0, x0 = mp.grid_origins(g.dim, n, g.overlap)
        assert np.array_equal(y0, np.arange(len(y0)) * (n - g.overlap[0])) and np.array_equal(x0, np.arange(len(x0)) * (n - g.overlap[1]))
        assert y0[-1] + n <= g.dim[0] and x0[-1] + n <= g.dim[1]
    for n in mg.SIZES:
        assert mg.GEOMETRIES[("asym", n)].overlap[0] != mg.GEOMETRIES[("asym", n)].overlap[1]
        assert mg.GEOMETRIES[("asym-T", n)].overlap[0] != mg.GEOMETRIES[("asym-T", n)].overlap[1]
        assert mg.GEOMETRIES[("asym", n)].dim == mg.GEOMETRIES[("asym-T", n)].dim[::-1]
        h, w = mg.GEOMETRIES[("ragged-0", n)].dim                      # an unread margin on both axes
        assert h % n and w % n
        assert (mg.GEOMETRIES[("odd-stride", n)].dim[1] % 2) and (n - mg.GEOMETRIES[("odd-stride", n)].overlap[0]) % 2


def test_blocks_reaches_nine_blocks_with_a_partial_last_one():
    for n, jobs in ((16, 132), (32, 66), (64, 33)):
        got, nb, last = mg.blocks(("blocks", n))
        per = mg.jobs_per_block(n)
        assert per == {16: 16, 32: 8, 64: 4}[n]
        assert got == jobs and nb == 9 and nb % 8 and 0 < last < per, (n, got, nb, last)
    for n in mg.SIZES:                                                  # one-window: every block mostly tail
        jobs, nb, last = mg.blocks(("one-window", n))
        assert (jobs, nb) == (2, 1) and last < mg.jobs_per_block(n)


def test_origins_reach_every_alignment():
    for n in mg.SIZES:
        _, x0 = mp.grid_origins(mg.GEOMETRIES[("row-stride-1", n)].dim, n, n - 1)
        assert set(x0 % 4) == {0, 1, 2, 3} and set(x0 % 8) == set(range(8))
        y0, _ = mp.grid_origins(mg.GEOMETRIES[("col-stride-1", n)].dim, n, n - 1)
        assert set(y0 % 4) == {0, 1, 2, 3}
        g = mg.GEOMETRIES[("odd-stride", n)]
        y0, x0 = mp.grid_origins(g.dim, n, g.overlap)
        assert set(x0 % 4) == {0, 1, 2, 3}
        assert set((y0[:, None] * g.dim[1] + x0[None, :]).reshape(-1) % 4) == {0, 1, 2, 3}      # the first sample of a window, in elements


# ---- ties and fragile windows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mg.SIZES)
def test_no_small_geometry_needs_a_window_set_aside(n):
    worst = {}
    for key in keys_of(n):
        g = mg.GEOMETRIES[key]
        rows, cols = mg.grid(key)
        windows = (g.T - 1) * rows * cols
        refs = [(mode, np.dtype(dtype).name, mg.ref(mode, key, dtype)) for dtype in mg.DTYPES for mode in mg.modes_of(key)]
        refs += [(mode, "signal", mg.signal_ref(mode, key)) for mode in mg.modes_of(key)]
        for mode, what, r in refs:
            bad, total = mg.set_aside(mode, r)
            per_pair = 1 if mode in mg.ENSEMBLES else g.T - 1
            assert r["corr"].size == per_pair * rows * cols
            if windows < SMALL or CAPS[mode] == 0.0:
                assert bad == 0, (key, mode, what, bad, total)
            else:
                assert bad <= CAPS[mode] * total, (key, mode, what, bad, total)
                if bad:
                    worst[(key[0], mode, what)] = f"{bad} / {total}"
    print(n, "set aside on the larger geometries:", worst)


# ---- both classes -----------------------------------------------------------------------------------------------------------------------
def test_masks_and_signal_stacks_hold_both_classes():
    for key in mg.KEYS:
        rows, cols = mg.grid(key)
        m = mg.mask(key)
        assert m.shape == mg.GEOMETRIES[key].dim and m.any() and not m.all()
        if rows * cols <= 10:
            continue
        r = mg.ref("masked", key)
        full, partial, below = masked_ref.classes(r["k"], key[1])
        assert below and (full + partial) and np.isnan(r["corr"]).any() and np.isfinite(r["corr"]).any(), key
        for mode in mg.modes_of(key):
            c = mg.signal_ref(mode, key)["corr"]
            assert np.isnan(c).any() and np.isfinite(c).any(), (key, mode)
            if mode != "masked":          # (without a threshold nothing is skipped: what is skipped above is the threshold's doing)
                assert np.isfinite(mg.ref(mode, key)["corr"]).all(), (key, mode)


def test_the_ensemble_thresholds_keep_every_pair():
    """From the references: with corr_min = 0 and s2n_min = 0.5 every pair of every window passes (s2n >= 1 by construction), so no pair
    value sits on a threshold and every count is the number of pairs."""
    for key in mg.KEYS:
        for mode in mg.ENSEMBLES:
            r = mg.ref(mode, key)
            assert (r["count"] == mg.GEOMETRIES[key].T - 1).all() and (r["pair_s2n"] >= 1.0).all() and (r["pair_corr"] > 1e-6).all(), (key, mode)


# ---- offsets, nodes, the NaN sample ---------------------------------------------------------------------------------------------------
def test_offsets_and_nodes():
    for key in mg.KEYS:
        g = mg.GEOMETRIES[key]
        rows, cols = mg.grid(key)
        sh = mg.offsets(key)
        assert sh.dtype == np.int16 and sh.shape == (g.T - 1, rows, cols, 2)
        assert tuple(sh[0, 0, 0]) == mg.WILD[0] and tuple(sh[-1, -1, -1]) == mg.WILD[1]
        clamped = mp.clamp_shift(sh, g.dim, g.n, g.overlap)
        assert not np.array_equal(clamped[0, 0, 0], sh[0, 0, 0]) and not np.array_equal(clamped[-1, -1, -1], sh[-1, -1, -1])
        inner = np.ones(sh.shape[:3], bool)
        inner[0, 0, 0] = inner[-1, -1, -1] = False
        assert (np.abs(sh[inner].astype(int) - np.array([mg.SHIFT[1], mg.SHIFT[0]])) <= 3).all()
        assert np.array_equal(mg.ref("shifted", key)["shift"], clamped)
        nd = mg.nodes(key)
        assert nd.dtype == np.int32 and nd.shape == (g.T - 1, rows, cols, 2)
        assert (np.abs(nd[inner] - 128 * np.array([mg.SHIFT[1], mg.SHIFT[0]])) <= 192).all()
        assert (np.abs(nd[0, 0, 0]) >= 20 * 128).all() and (np.abs(nd[-1, -1, -1]) >= 20 * 128).all()
    for key in mg.SYM_KEYS:                # the wild nodes do push samples across the frame edge
        g = mg.GEOMETRIES[key]
        dv, du = deform_ref.dense64(mg.nodes(key)[0], g.dim, g.n, g.overlap[0])
        assert (64 * np.arange(g.dim[0])[:, None] + dv < 0).any() or (64 * np.arange(g.dim[1])[None, :] + du < 0).any(), key
    assert len(mg.SYM_KEYS) == 18
    for key in set(mg.KEYS) - set(mg.SYM_KEYS):
        with pytest.raises(ValueError, match="one overlap for both axes"):
            mg.compute("deformed", key, mg.stack(key))


def test_the_nan_sample_is_read_by_several_windows_but_not_by_all():
    for n in mg.SIZES:
        for name in mg.NAN_NAMES:
            key = (name, n)
            y, x = mg.nan_sample(key)
            hit = mg.windows_holding(key, y, x)
            assert mg.mask(key)[y, x] and 2 <= hit.sum() < hit.size, key
            stack = po.sliding_window_stack(np.arange(np.prod(mg.GEOMETRIES[key].dim)).reshape((1,) + mg.GEOMETRIES[key].dim), (n, n),
                                            mg.GEOMETRIES[key].overlap)[0]
            lin = y * mg.GEOMETRIES[key].dim[1] + x
            assert np.array_equal((stack == lin).any(axis=(-2, -1)).reshape(hit.shape), hit)


# ---- the references take an int or a pair -------------------------------------------------------------------------------------------------
def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("n", mg.SIZES)
def test_an_int_overlap_is_the_pair_of_it(n):
    key = ("odd-stride", n)
    g = mg.GEOMETRIES[key]
    a, ov = mg.stack(key)[:3], g.overlap[0]
    sh, nd, m = mg.offsets(key)[:2], mg.nodes(key)[:2], mg.mask(key)
    same(mp.shifted_piv(a, n, ov, sh), mp.shifted_piv(a, n, (ov, ov), sh))
    same(deform_ref.deformed_piv(a, n, ov, nd), deform_ref.deformed_piv(a, n, (ov, ov), nd))
    same(spof_ref.piv(a, n, ov), spof_ref.piv(a, n, (ov, ov)))
    same(spof_ref.ensemble(a, n, ov, **mg.SPOF_ENS_KW), spof_ref.ensemble(a, n, (ov, ov), **mg.SPOF_ENS_KW))
    same(masked_ref.piv(a, n, ov, m), masked_ref.piv(a, n, (ov, ov), m))
    same(peak2_ref.piv(a, n, ov, 1), peak2_ref.piv(a, n, (ov, ov), 1))
    for q, p in zip(mp.grid_origins(g.dim, n, ov), mp.grid_origins(g.dim, n, (ov, ov))):
        assert np.array_equal(q, p)
    assert np.array_equal(mp.clamp_shift(sh, g.dim, n, ov), mp.clamp_shift(sh, g.dim, n, (ov, ov)))
    # ... and a pair is read as (oy, ox): the transposed stack at the swapped pair gives the transposed windows
    t = mg.GEOMETRIES[("asym", n)]
    b = mg.stack(("asym", n))
    r, rt = spof_ref.piv(b, n, t.overlap), spof_ref.piv(np.ascontiguousarray(b.transpose(0, 2, 1)), n, t.overlap[::-1])
    assert r["corr"].shape[1:] == mg.grid(("asym", n)) == rt["corr"].shape[:0:-1]
    assert np.allclose(r["corr"], rt["corr"].transpose(0, 2, 1), rtol=0, atol=1e-12)
