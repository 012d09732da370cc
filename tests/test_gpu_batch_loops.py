"""Host loops past their first iteration: a deformation pass in several batches of pairs (``deform_pass``, api_piv.hip), a sliding
finish in several tiles of outputs and as partial reads (``lspiv_ensemble_sliding_finish``, api_ensemble.hip), and the ensemble's
float64 rescue across pair-blocks of 16 and across kept chunks of more than one block, on sliding and shifted handles.  Two test hooks
make the batches and tiles small: LSPIV_DEFORM_WS_BYTES and LSPIV_SLIDING_TILE_BYTES (the switch list).  A result is per
pair, per output: every cut must leave every bit where it was, and the uncut run is gated against the float64 reference in the same
test.  The inputs are checked on the CPU: tests/test_deform_host.py, tests/test_sliding_host.py, tests/test_ensemble_multipass_host.py."""
import contextlib

import numpy as np
import pytest

from pyorc_amd import _lib, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import deform_ref as dr
from tests import ensemble_multipass_ref as emp
from tests import multipass_ref as mp
from tests import sliding_ref as sr
from tests import test_gpu_ensemble_multipass as tem
from tests import test_gpu_sliding as tsl
from tests.test_gpu_deform import gate as deform_gate
from tests.test_gpu_multipass import KEYS, same_bits
from tests.test_gpu_rescue_modes import refitted
from tests.test_multipass_host import long_stack

pytestmark = pytest.mark.gpu
TOL = 1e-4
DTYPES = (np.uint8, np.float32, np.float64)
DTYPE_IDS = ("u8", "f32", "f64")


@contextlib.contextmanager
def rescue_off():
    old = _lib.get_option("rescue")
    _lib.set_option("rescue", 0)
    try:
        yield
    finally:
        _lib.set_option("rescue", old)


def differing(x, y):
    """Windows whose (u, v) differ between two runs."""
    return ~(((x[0] == y[0]) | (np.isnan(x[0]) & np.isnan(y[0]))) & ((x[1] == y[1]) | (np.isnan(x[1]) & np.isnan(y[1]))))


# ---- B1. a deformation pass in batches of pairs ---------------------------------------------------------------------------------------------
def deform_workspace(monkeypatch, n_frames, dim, T, n, ov):
    """A workspace of exactly ``n_frames`` warped frames (None: the default), checked against what the library reports for it."""
    H, W = dim
    if n_frames is None:
        monkeypatch.delenv("LSPIV_DEFORM_WS_BYTES", raising=False)
        return
    monkeypatch.setenv("LSPIV_DEFORM_WS_BYTES", str(n_frames * H * W * 4))
    n_win = int(np.prod(window.get_array_shape(dim, (n, n), (ov, ov))))
    assert _lib.load().lspiv_deform_required_bytes(T, H, W, n, n, ov, ov) == min(n_frames, T - 1) * H * W * 4 + (T - 1) * n_win * 8


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", list(dr.PASS_CASES))
def test_deformation_batches_do_not_change_a_bit(gpu, monkeypatch, case, dtype):
    """3 pairs in batches of 1 + 1 + 1 and 2 + 1 (a ragged last batch): frame pointer, nodes, the four result arrays and the planes move
    along with the batch.  With the signal threshold, with and without planes, host and HBM-resident stacks."""
    n, ov, dim = dr.PASS_CASES[case]
    nodes, r = dr.hand_nodes(case), dr.signal_ref(case)
    a = dr.signal_stack(case).astype(dtype)       # (the float stacks hold the same sample values: an affine map would move the zeros)
    for x in (a, DeviceFrames.from_host(a)):
        run = lambda planes: list(piv.piv_pairs_deformed(x, (n, n), (ov, ov), nodes, dr.SIGNAL_THR, return_planes=planes))
        deform_workspace(monkeypatch, None, dim, dr.PASS_T, n, ov)
        base, fit, seen = refitted(lambda: run(True))
        deform_gate(base[:4], r, base[4])
        bare = run(False)
        same_bits(bare, base[:4], "without planes")
        for k in (1, 2):
            deform_workspace(monkeypatch, k, dim, dr.PASS_T, n, ov)
            got, fit_k, seen_k = refitted(lambda: run(True))
            same_bits(got, base, f"batches of {k}")
            assert (fit_k, seen_k) == (fit, seen), k
            same_bits(run(False), bare, f"batches of {k}, without planes")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("field", dr.RESCUE_FIELDS)
def test_rescue_in_a_batch_after_the_first(gpu, monkeypatch, field, dtype):
    """The speckle stack at 32 @ 16, 4 pairs in batches of 1 and of 2: the rescue pass reads window B from the workspace before the next
    batch overwrites it, and windows of later batches ARE re-fitted (the windows whose u, v differ with the pass off, by pair).
    Measured on an MI355X: 140 (uniform) and 124 (mixed) of 308 windows re-fitted, for every sample type; windows that differ without
    the pass in each of the pairs 0, 1, 2 and 3."""
    n, ov = 32, 16
    a, r, nodes = mp.rescue_stack(dtype), dr.rescue_ref(n, ov, field, dtype), dr.rescue_nodes(n, ov, field)
    run = lambda: list(piv.piv_pairs_deformed(a, (n, n), (ov, ov), nodes, return_planes=True))
    base, fit, seen = refitted(run)
    deform_gate(base[:4], r, base[4])
    with rescue_off():
        off = run()
    pairs = np.unique(np.nonzero(differing(off, base))[0])
    print("re-fitted:", fit, "of", seen, "| pairs with windows that differ without the pass:", pairs.tolist())
    assert fit > 0 and pairs.max() >= 2            # a re-fitted window in a batch after the first, for batches of 1 and of 2 pairs
    for k in (1, 2):
        deform_workspace(monkeypatch, k, mp.RESCUE_DIM, mp.RESCUE_T, n, ov)
        got, fit_k, seen_k = refitted(run)
        same_bits(got, base, f"batches of {k}")
        assert (fit_k, seen_k) == (fit, seen), k


def test_chain_with_two_deformation_passes_in_batches(gpu, monkeypatch):
    """64 -> 32 and two deformation passes: the second pass's nodes come from the first one's batched results."""
    a = dr.accuracy_stack(5)
    chain = [(64, 32), (32, 16)]
    run = lambda x: piv.piv_multipass(x, chain, return_planes=True, return_shift=True, deform_passes=2)
    base = run(a)
    r = dr.deformed_piv(a, 32, 16, dr.predict_nodes(*piv.piv_multipass(a, chain, deform_passes=1)[:2]))    # on the GPU's own previous pass
    deform_gate(base[:4], r, base[4])
    for k in (1, 2):
        deform_workspace(monkeypatch, k, a.shape[1:], len(a), 32, 16)
        same_bits(run(a), base, f"batches of {k}")
        same_bits(run(DeviceFrames.from_host(a)), base, f"batches of {k}, device entry")


def test_get_ffpiv_chunks_of_a_batched_chain(gpu, monkeypatch):
    """51 pairs in chunks on the anchors, each chunk's deformation pass one pair per batch."""
    a = long_stack()
    P = len(a) - 1
    x, y = window.get_rect_coordinates(a.shape[1:], (16, 16), (8, 8))
    run = lambda **kw: velocimetry.get_ffpiv(a, y, x, np.full(P, 0.5), (16, 16), (8, 8), (16, 16), 0.02, 0.02, coarse_passes=[(64, 32)],
                                             deform_passes=1, **kw)
    whole = run()
    deform_workspace(monkeypatch, 1, a.shape[1:], len(a), 16, 8)
    for kw in (dict(chunksize=3), dict()):
        got = run(**kw)
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (kw, k)


# ---- B2. a sliding finish in tiles of outputs, partial reads, pair-blocks and kept chunks ---------------------------------------------------
WS, OV = sr.LOOP_WINDOW
# one output's mean planes on the 200 x 264 speckle stack: ``out_bytes`` = n_win * wy * wx * sizeof(float) of lspiv_ensemble_sliding_finish
# (api_ensemble.hip), which divides LSPIV_SLIDING_TILE_BYTES by it -- here a block of the store (window.sliding_store_bytes) less its counts
N_WIN = int(np.prod(window.get_array_shape((200, 264), WS, OV)))
OUT_BYTES = window.sliding_store_bytes(1, (200, 264), WS, OV) - N_WIN * 4
assert OUT_BYTES == N_WIN * WS[0] * WS[1] * 4


@contextlib.contextmanager
def sliding_handle(a, M, s, chunks=None):
    e = piv.Ensemble(a.shape[1:], WS, OV, sliding=(M, s))
    try:
        for f0, f1 in chunks or [(0, len(a))]:
            e.accumulate(a[f0:f1], sr.KW["corr_min"], sr.KW["s2n_min"])
        yield e
    finally:
        e.close()


def finish(e, **kw):
    """(u, v, count, planes), (flagged, rescued, float32_kept)."""
    got = e.finish_sliding(sr.KW["count_min"], return_planes=True, **kw)
    st = e.stats()
    return got, (st["flagged"], st["rescued"], st["float32_kept"])


def tile_of(monkeypatch, n_outputs):
    if n_outputs is None:
        monkeypatch.delenv("LSPIV_SLIDING_TILE_BYTES", raising=False)
    else:
        monkeypatch.setenv("LSPIV_SLIDING_TILE_BYTES", str(n_outputs * OUT_BYTES))


def uv_err(got, r):
    ok = ~r["tie"]
    return max(tsl.rel_err(got[0][ok], r["v_x"][ok]), tsl.rel_err(got[1][ok], r["v_y"][ok]))


@pytest.mark.parametrize("case", ["long", "stepped"])
def test_sliding_tiles_partial_reads_and_pair_blocks(gpu, monkeypatch, case):
    """40 pairs, (M, s) = (20, 4): 6 outputs of 20 pairs each; outputs 0 .. 3 straddle pair 16, output 4 pair 32 (the rescue's pair-blocks).
    Tiles of 1 and of 4 + 2 outputs thread the tile's first output into the mean kernel, the rescue and the host copies; every
    (first, n) read is the rows of the whole read; two accumulate calls make two kept chunks of two pair-blocks each.
    Measured on an MI355X: 451 of 990 (output, window) flagged, all 451 re-fitted, in one call and in two; without the pass 77, 77, 76,
    77, 77 and 66 windows of the outputs 0 .. 5 differ and the u, v error is 8.1e-4 (5.8e-6 with it).
    "stepped" is the same run on the stack whose speckles jump (tests/sliding_ref.py): on "long" every pair moves 1 px and a flagged
    window's fit is the same whichever pairs the rescue sums; on "stepped" it is not (tests/test_sliding_host.py), so the u, v gate there
    is what checks ``out0``, ``pair0`` and ``blk0`` of ``ensemble_partials``.  Measured: 451 flagged and re-fitted again; 77, 77, 77, 77,
    77 and 66 windows differ without the pass, u, v error 3.5e-4 without and 9.3e-6 with it.  A build that hands the rescue the first
    tile's ``out0`` for every tile, or ``pair0 = 0`` for every kept chunk, fails "stepped" and passes "long"."""
    T, M, s, calls, stepped = sr.LOOP_CASES[case]
    a, r = sr.speckle_stack(T=T, stepped=stepped), sr.loop_ref(case)
    n_out = r["v_x"].shape[0]
    assert (n_out, a.shape, r["planes"].nbytes // 2) == (6, (41, 200, 264), n_out * OUT_BYTES)
    public = tsl.run_public(a, WS, OV, M, s, sr.KW)
    with sliding_handle(a, M, s) as e:
        whole, st = finish(e)
        print("flagged, rescued, float32 kept:", st)
        assert np.array_equal(np.asarray(public["v_x"]), whole[0], equal_nan=True) and np.array_equal(np.asarray(public["v_y"]), whole[1], equal_nan=True)
        tsl.check_parity(public, whole[3], whole[2], r)                                   # flagged windows included
        assert e.stats()["retain_complete"] and st[0] > 0 and st[1] == st[0] - st[2] > 0
        for tile in (1, 4):
            tile_of(monkeypatch, tile)
            got, st_t = finish(e)
            same_bits(got, whole, f"tiles of {tile}")
            assert st_t == st, tile
            for k in KEYS:
                assert np.array_equal(np.asarray(tsl.run_public(a, WS, OV, M, s, sr.KW)[k]), np.asarray(public[k]), equal_nan=True), (tile, k)
        for tile in (None, 1):
            tile_of(monkeypatch, tile)
            for k in range(n_out):
                for m in range(1, n_out - k + 1):
                    got, _ = finish(e, first=k, n=m)
                    same_bits(got, [x[k:k + m] for x in whole], f"outputs [{k}, {k + m}), tile {tile}")
    tile_of(monkeypatch, None)
    # the rescue re-fits windows of outputs after the first
    with rescue_off(), sliding_handle(a, M, s) as e:
        off, st_off = finish(e)
    differ = differing(off, whole)
    print("windows that differ without the pass, per output:", differ.sum(axis=(1, 2)).tolist(), "| u, v error with", uv_err(whole, r), "without", uv_err(off, r))
    assert st_off[0] == 0 and np.array_equal(off[2], whole[2]) and np.array_equal(off[3], whole[3], equal_nan=True)
    assert 1 <= differ.sum() <= st[1] and differ[1:].any()
    # two accumulate calls of 20 pairs: two kept chunks, blk0 = 2 and pair0 = 20 in the second, ragged blocks 16 + 4
    for tile in (None, 1):
        tile_of(monkeypatch, tile)
        with sliding_handle(a, M, s, calls) as e:
            two, st2 = finish(e)
            assert e.stats()["retain_complete"] and e.stats()["chunks_kept"] == 2
        assert np.array_equal(two[3], whole[3], equal_nan=True) and np.array_equal(two[2], whole[2])
        assert np.array_equal(np.isnan(two[0]), np.isnan(whole[0])) and np.array_equal(np.isnan(two[1]), np.isnan(whole[1]))
        print("two calls: u, v", uv_err(two, r), st2)
        assert uv_err(two, r) <= TOL and st2[:2] == st[:2]


def test_sliding_tiles_over_many_outputs(gpu, monkeypatch):
    """35 pairs, (M, s) = (4, 2): 16 outputs in tiles of 5 + 5 + 5 + 1.  Measured on an MI355X: 1182 of 2640 (output, window) flagged, all
    re-fitted."""
    T, M, s, calls, _ = sr.LOOP_CASES["many"]
    a, r = sr.speckle_stack(T=T), sr.loop_ref("many")
    public = tsl.run_public(a, WS, OV, M, s, sr.KW)
    with sliding_handle(a, M, s) as e:
        whole, st = finish(e)
        print("flagged, rescued, float32 kept:", st)
        assert whole[0].shape[0] == 16 and st[1] > 0
        assert np.array_equal(np.asarray(public["v_x"]), whole[0], equal_nan=True)
        tsl.check_parity(public, whole[3], whole[2], r)
        for tile in (5, 1):
            tile_of(monkeypatch, tile)
            got, st_t = finish(e)
            same_bits(got, whole, f"tiles of {tile}")
            assert st_t == st, tile
        tile_of(monkeypatch, 5)
        got, _ = finish(e, first=3, n=11)                                                 # 5 + 5 + 1 from output 3
        same_bits(got, [x[3:14] for x in whole], "outputs [3, 14) in tiles of 5")
    with sliding_handle(a, M, s, calls) as e:                                             # still in tiles of 5
        two, st2 = finish(e)
    assert np.array_equal(two[3], whole[3], equal_nan=True) and np.array_equal(two[2], whole[2]) and st2[:2] == st[:2]
    assert np.array_equal(np.isnan(two[0]), np.isnan(whole[0])) and uv_err(two, r) <= TOL


# ---- B3. the shifted ensemble over more than one pair-block ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stepped", [False, True], ids=["steady", "stepped"])
@pytest.mark.parametrize("dtype", emp.LONG_DTYPES, ids=["f32", "f64"])
def test_shifted_ensemble_rescue_across_pair_blocks_and_chunks(gpu, dtype, stepped):
    """35 pairs on a shifted handle: one accumulate call makes the pair-blocks 16 + 16 + 3, two calls (17 + 18 pairs) two kept chunks of
    two blocks each.  float64 also as a DeviceFrames stack (on the host entry it is narrowed while staged).
    Measured on an MI355X: 77 of 165 windows flagged and re-fitted, in one call and in two, on every stack; without the pass 44 windows
    differ and the u, v error is 1.1e-3 (float32) and 6.4e-4 (float64) against 5.6e-6 with it.
    "stepped": the stack whose speckles jump, where the fit of a flagged window depends on which pairs are summed
    (tests/test_ensemble_multipass_host.py: a call's pairs alone move every such window by 8e-3 px or more) -- the u, v gate of the
    two-call run there checks ``blk0`` of ``ensemble_partials``; on "steady" it cannot.  Measured: 77 flagged and re-fitted, all 77 differ
    without the pass, u, v error 6.1e-4 (float32) and 5.5e-4 (float64) without against 5.6e-6 with it.  A build with ``blk0 = 0`` for
    every kept chunk fails "stepped" and passes "steady"."""
    n, ov = emp.RESCUE
    a, r, sh = emp.long_speckle_stack(dtype, stepped), emp.long_speckle_ref(dtype, stepped), emp.speckle_shift()
    ok = ~r["tie"]
    err = lambda g: max(tem.rel_err(g["u"][ok], r["u"][ok]), tem.rel_err(g["v"][ok], r["v"][ok]))
    for x in (a,) if dtype == np.float32 else (a, DeviceFrames.from_host(a)):
        one = tem.run_pass(x, n, ov, sh, emp.KW)
        two = tem.run_pass(x, n, ov, sh, emp.KW, emp.LONG_CHUNKS)
        for got, kept in ((one, 1), (two, 2)):
            st = got["stats"]
            print(st)
            assert st["retain_complete"] and st["chunks_kept"] == kept and st["flagged"] > 0
            assert st["flagged"] == st["rescued"] + st["float32_kept"] and st["rescued"] > 0
            tem.check_parity(got, r)                                                      # flagged windows included
        tem.same_bits(two, one, keys=("count", "planes", "corr", "s2n"))
        assert (two["stats"]["flagged"], two["stats"]["rescued"]) == (one["stats"]["flagged"], one["stats"]["rescued"])
        with rescue_off():
            off = tem.run_pass(x, n, ov, sh, emp.KW)
        tem.same_bits(off, one, keys=("count", "planes", "corr", "s2n"))
        differ = differing((off["u"], off["v"]), (one["u"], one["v"]))
        print("windows that differ without the pass:", int(differ.sum()), "| u, v error with", err(one), "two calls", err(two), "without", err(off))
        assert off["stats"]["flagged"] == 0 and 1 <= differ.sum() <= one["stats"]["rescued"]
        assert err(one) <= TOL and err(two) <= TOL < err(off)
