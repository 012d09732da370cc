"""Sliding ensemble on the GPU against tests/sliding_ref.py: parity of every output on every window
family, the count filter, chunk independence in bits, the degenerate windows against today's ensemble, the float64 rescue per
output (on a stack that has flagged windows), signal thresholds in both modes on host and HBM-resident stacks, and the public surface.  The inputs and their CPU checks (tie shares, differing NaN masks): tests/test_sliding_host.py."""
import numpy as np
import pytest

from pyorc_amd import DeviceFrames, _lib, frames, piv, velocimetry, window
from tests import sliding_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4     # the project's gate, as tests/test_gpu_fullsize.py has it: relative, floor 0.05 (px, or plane units)


def rel_err(got, want, floor=0.05):
    with np.errstate(all="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), floor)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


def run_public(a, ws, ov, M, s, kw, **more):
    nr, nc = window.get_array_shape(a.shape[1:], ws, ov)
    return velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), np.ones(len(a) - 1), ws, ov, ws, 1.0, 1.0, ensemble_corr=True,
                                 ensemble_window=M, ensemble_stride=s, **kw, **more)


def run_handle(a, ws, ov, M, s, kw, chunks=None):
    """(u, v, count, planes, stats) of one sliding handle fed with the frame slices ``chunks`` (default: the whole stack)."""
    e = piv.Ensemble(a.shape[1:], ws, ov, sliding=(M, s))
    try:
        for f0, f1 in chunks or [(0, len(a))]:
            e.accumulate(a[f0:f1], kw["corr_min"], kw["s2n_min"], kw.get("signal_threshold"))
        return e.finish_sliding(kw["count_min"], return_planes=True) + (e.stats(),)
    finally:
        e.close()


def check_parity(got, planes, cnt, r, where=None):
    ok = ~r["tie"] if where is None else where
    for k in ("v_x", "v_y", "corr", "s2n"):
        g = np.asarray(got[k])
        assert g.dtype == np.float32 and g.shape == r[k].shape, k
        assert np.array_equal(np.isnan(g)[ok], np.isnan(r[k])[ok]), k
        print(k, rel_err(g[ok], r[k][ok]))
        assert rel_err(g[ok], r[k][ok]) <= TOL, k
    assert np.array_equal(cnt, r["count"])
    flat = ok.reshape(ok.shape[0], -1)
    assert np.array_equal(np.isnan(planes)[flat], np.isnan(r["planes"])[flat])
    print("planes", rel_err(planes[flat], r["planes"][flat]))
    assert rel_err(planes[flat], r["planes"][flat]) <= TOL


@pytest.mark.parametrize("dtype", ref.DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("case,M,s", ref.PARITY, ids=[f"{c}-{M}-{s}" for c, M, s in ref.PARITY])
def test_every_output_matches_the_reference(gpu, case, M, s, dtype):
    ws, ov, _, _ = ref.CASES[case]
    a, r = ref.case_stack(case, dtype), ref.case_ref(case, dtype, M, s)
    got = run_public(a, ws, ov, M, s, ref.KW)
    u, v, cnt, planes, st = run_handle(a, ws, ov, M, s, ref.KW)
    assert np.array_equal(np.asarray(got["v_x"]), u, equal_nan=True) and np.array_equal(np.asarray(got["v_y"]), v, equal_nan=True)   # res = dt = 1
    assert np.array_equal(np.asarray(got.coords["time"]), r["time"])
    check_parity(got, planes, cnt, r)
    # the rescue per output: with the frames retained (host accumulate) every flagged fit is re-evaluated or accounted for
    assert st["retain_complete"] and st["flagged"] == st["rescued"] + st["float32_kept"]


def test_count_filter_gives_each_output_its_own_nan_mask(gpu):
    a, r = ref.blanked_stack(), ref.blanked_ref()
    got = run_public(a, (32, 32), (16, 16), 4, 2, ref.COUNT_KW)
    u, v, cnt, planes, _ = run_handle(a, (32, 32), (16, 16), 4, 2, ref.COUNT_KW)
    assert np.array_equal(cnt, r["count"])
    for k in ("v_x", "v_y", "corr"):
        assert np.array_equal(np.isnan(np.asarray(got[k])), np.isnan(r[k])), k
    assert np.array_equal(np.isnan(planes), np.isnan(r["planes"]))
    assert len({np.isnan(np.asarray(got["v_x"])[j]).tobytes() for j in range(len(u))}) >= 2
    check_parity(got, planes, cnt, r)


@pytest.mark.parametrize("case", ["32-16", "64-48"])
def test_chunking_does_not_change_a_bit(gpu, case):
    ws, ov, _, T = ref.CASES[case]
    a, s = ref.case_stack(case), 2
    whole = run_public(a, ws, ov, 4, s, ref.KW)
    for cs in (2 * s + 1, 3 * s + 1):          # chunks of 2 s and 3 s pairs (+ the halo frame)
        got = run_public(a, ws, ov, 4, s, ref.KW, chunksize=cs)
        for k in ("v_x", "v_y", "corr", "s2n"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (cs, k)
    pl = [run_handle(a, ws, ov, 4, s, ref.KW, chunks)[3] for chunks in (None, [(0, 5), (4, 11), (10, 13)])]
    assert np.array_equal(pl[0], pl[1], equal_nan=True)
    # one launch per block (LSPIV_WALK = 0) against the walking kernel: the gate, not the bits
    old = _lib.get_option("walk")
    _lib.set_option("walk", 0)
    try:
        per_block = run_public(a, ws, ov, 4, s, ref.KW)
    finally:
        _lib.set_option("walk", old)
    for k in ("v_x", "v_y", "corr", "s2n"):
        g, w = np.asarray(per_block[k]), np.asarray(whole[k], dtype=np.float64)
        ok = ~ref.case_ref(case, np.uint8, 4, s)["tie"]
        assert np.array_equal(np.isnan(g)[ok], np.isnan(w)[ok]) and rel_err(g[ok], w[ok]) <= TOL, k


def test_degenerate_windows_are_todays_ensemble(gpu):
    ws, ov, _, T = ref.CASES["32-16"]
    a, P = ref.case_stack("32-16"), T - 1
    kw = ref.KW

    def plain(stack):
        e = piv.Ensemble(stack.shape[1:], ws, ov)
        try:
            e.accumulate(stack, kw["corr_min"], kw["s2n_min"])
            return e.finish(kw["count_min"], len(stack) - 1, return_mean=True)     # count_min * pairs, as the sliding mode counts
        finally:
            e.close()

    u, v, cnt, planes, _ = run_handle(a, ws, ov, P, P, kw)       # s = M = P: one output
    pu, pv, pc, pm = plain(a)
    assert u.shape[0] == 1 and np.array_equal(cnt.ravel(), pc)
    assert np.array_equal(np.isnan(planes), np.isnan(pm)) and rel_err(planes, pm.astype(np.float64)) <= TOL
    assert np.array_equal(np.isnan(u), np.isnan(pu)) and rel_err(u, pu.astype(np.float64)) <= TOL and rel_err(v, pv.astype(np.float64)) <= TOL
    u, v, cnt, planes, _ = run_handle(a, ws, ov, 4, 4, kw)       # s = M: one fresh ensemble per block
    assert u.shape[0] == 3
    for b in range(3):
        pu, pv, pc, pm = plain(a[4 * b:4 * b + 5])
        assert np.array_equal(cnt[b].ravel(), pc)
        assert np.array_equal(np.isnan(planes[b]), np.isnan(pm[0])) and rel_err(planes[b], pm[0].astype(np.float64)) <= TOL
        assert np.array_equal(np.isnan(u[b]), np.isnan(pu[0])) and rel_err(u[b], pu[0].astype(np.float64)) <= TOL
        assert rel_err(v[b], pv[0].astype(np.float64)) <= TOL


def test_rescue_per_output_and_switched_off(gpu):
    """The float64 rescue per output on a stack that HAS ill-conditioned fits (tests/sliding_ref.py ``speckle_stack``): windows are
    flagged and re-evaluated over their own output's pairs, every non-tie window then passes the gate -- in one accumulate call and
    in two (the second starts at pair 4, output 1 straddles them) --, and without the pass the same run misses the gate."""
    ws, ov, M, s = ref.RESCUE
    a, r = ref.speckle_stack(), ref.speckle_ref()
    ok = ~r["tie"]

    def err(u, v):
        e = max(rel_err(u[ok], r["v_x"][ok]), rel_err(v[ok], r["v_y"][ok]))
        print("u, v", e)
        return e

    u, v, cnt, planes, st = run_handle(a, ws, ov, M, s, ref.KW)
    print(st)
    assert st["retain_complete"] and st["chunks_kept"] == 1 and st["flagged"] > 0
    assert st["rescued"] == st["flagged"] - st["float32_kept"] > 0
    assert np.array_equal(cnt, r["count"]) and np.array_equal(np.isnan(u)[ok], np.isnan(r["v_x"])[ok])
    assert err(u, v) <= TOL                                  # flagged windows included
    u2, v2, cnt2, planes2, st2 = run_handle(a, ws, ov, M, s, ref.KW, ref.RESCUE_CHUNKS)
    print(st2)
    assert st2["retain_complete"] and st2["chunks_kept"] == 2 and (st2["flagged"], st2["rescued"]) == (st["flagged"], st["rescued"])
    assert np.array_equal(planes2, planes, equal_nan=True) and np.array_equal(cnt2, cnt)
    assert np.array_equal(np.isnan(u2), np.isnan(u)) and err(u2, v2) <= TOL
    old = _lib.get_option("rescue")
    _lib.set_option("rescue", 0)
    try:
        u0, v0, cnt0, planes0, st0 = run_handle(a, ws, ov, M, s, ref.KW)
    finally:
        _lib.set_option("rescue", old)
    assert st0["flagged"] == 0 and np.array_equal(cnt0, cnt) and np.array_equal(planes0, planes, equal_nan=True)
    same = ((u0 == u) | (np.isnan(u0) & np.isnan(u))) & ((v0 == v) | (np.isnan(v0) & np.isnan(v)))
    print("windows that differ without the pass", int((~same).sum()))
    assert 1 <= (~same).sum() <= st["rescued"]              # only re-evaluated windows differ: the others keep their bits
    assert err(u0, v0) > TOL                                 # what the pass is for


@pytest.mark.parametrize("mode", [0, 1], ids=["per-pair", "per-position"])
def test_signal_thresholds_on_host_and_device_stacks(gpu, mode):
    """``signal_threshold`` in both signal modes against the reference, and the same stack resident in HBM: through ``get_ffpiv``
    (a ``DeviceFrames`` stack) and through ``accumulate_dev`` on a borrowed pointer -- the bits of the host stack, rescue included."""
    ws, ov, M, s = (32, 32), (16, 16), 4, 2
    a, r = ref.signal_stack(), ref.signal_ref(mode)
    kw = dict(ref.KW, signal_threshold=ref.SIGNAL_THR)
    old = _lib.get_option("signal_mode")
    _lib.set_option("signal_mode", mode)
    try:
        got = run_public(a, ws, ov, M, s, kw)
        u, v, cnt, planes, st = run_handle(a, ws, ov, M, s, kw)
        d = DeviceFrames.from_host(a)
        dev = run_public(d, ws, ov, M, s, kw)
        e = piv.Ensemble(a.shape[1:], ws, ov, sliding=(M, s))
        try:
            e.set_retain(e.RETAIN_BORROW)
            d_cs = DeviceFrames.empty((2, len(a) - 1, e.n_rows * e.n_cols), np.float32)
            e.accumulate_dev(d.ptr, d.dtype, len(a), kw["corr_min"], kw["s2n_min"], d_cs.ptr, kw["signal_threshold"])
            ud, vd, cntd, planesd = e.finish_sliding(kw["count_min"], return_planes=True)
            std = e.stats()
        finally:
            e.close()
    finally:
        _lib.set_option("signal_mode", old)
    check_parity(got, planes, cnt, r)
    assert np.isnan(u[:, 0, 0]).all() and (cnt[:, 0, 0] == 0).all()                 # the empty corner: dropped in every output
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(np.asarray(dev[k]), np.asarray(got[k]), equal_nan=True), k
    for x, y in ((ud, u), (vd, v), (cntd, cnt), (planesd, planes)):
        assert np.array_equal(x, y, equal_nan=True)
    assert std["retain_complete"] and std["chunks_kept"] == 1 and (std["flagged"], std["rescued"]) == (st["flagged"], st["rescued"])


def test_the_store_keeps_the_layout_of_its_first_call(gpu):
    """64 x 64: the walking kernel leaves lane-major slots, the per-block path row-major ones.  A handle refuses a call that would
    write the other layout, and the finish decodes what was written whatever the 'walk' option says by then."""
    ws, ov, _, _ = ref.CASES["64-48"]
    a = ref.case_stack("64-48")
    want = run_handle(a, ws, ov, 4, 2, ref.KW)
    old = _lib.get_option("walk")
    e = piv.Ensemble(a.shape[1:], ws, ov, sliding=(4, 2))
    try:
        e.reserve_sliding(len(a) - 1)
        e.accumulate(a[:5], ref.KW["corr_min"], ref.KW["s2n_min"])
        _lib.set_option("walk", 0)
        with pytest.raises(ValueError, match="'walk' setting .* changed between accumulate calls"):
            e.accumulate(a[4:], ref.KW["corr_min"], ref.KW["s2n_min"])
        assert e.finish_sliding(ref.KW["count_min"])[0].shape[0] == 1          # the refused call left the handle as it was
        _lib.set_option("walk", old)
        e.accumulate(a[4:], ref.KW["corr_min"], ref.KW["s2n_min"])
        _lib.set_option("walk", 0)
        got = e.finish_sliding(ref.KW["count_min"], return_planes=True)
    finally:
        _lib.set_option("walk", old)
        e.close()
    for x, y in zip(got, want[:4]):
        assert np.array_equal(x, y, equal_nan=True)


def test_calls_a_sliding_handle_refuses(gpu):
    e = piv.Ensemble((70, 90), (32, 32), (16, 16), sliding=(4, 2))
    try:
        a = ref.case_stack("32-16")
        with pytest.raises(ValueError, match="accumulated give 0"):
            e.finish_sliding(0.2)
        e.accumulate(a[:6], 0.1, 1.5)                          # 5 pairs: ends inside a block, so it was the last call
        with pytest.raises(ValueError, match="multiple of 2 pairs"):
            e.accumulate(a[5:8], 0.1, 1.5)
        for call in (lambda: e.finish(0.2, 1), e.export_state, lambda: e.import_state(np.zeros((12, 32, 32)), np.zeros(12)),
                     lambda: piv.ensemble_allreduce([e])):
            with pytest.raises(ValueError, match="sliding ensemble handle"):
                call()
        assert e.finish_sliding(0.2)[0].shape == (1, 3, 4)
        with pytest.raises(ValueError, match=r"outputs \[1, 2\) asked for"):
            e.finish_sliding(0.2, first=1, n=1)
    finally:
        e.close()
    plain = piv.Ensemble((70, 90), (32, 32), (16, 16))
    try:
        with pytest.raises(ValueError, match="sliding="):
            plain.finish_sliding(0.2)
    finally:
        plain.close()


def test_public_surface_labels_and_scaling(gpu, monkeypatch):
    a = ref.case_stack("32-16")
    t = np.cumsum(np.r_[0.0, np.linspace(0.03, 0.05, len(a) - 1)])
    kw = dict(ensemble_corr=True, ensemble_window=4, ensemble_stride=2, time=t, resolution=0.01)
    ds = frames.get_piv(a, 32, **kw)
    r = ref.sliding_piv(a, np.diff(t), (32, 32), (16, 16), 4, 2, res=0.01, time=t)
    assert np.asarray(ds["v_x"]).shape == (5, 3, 4) and np.array_equal(np.asarray(ds.coords["time"]), r["time"])
    ok = ~r["tie"]
    for k in ("v_x", "v_y", "corr", "s2n"):
        g = np.asarray(ds[k])
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g)[ok], np.isnan(r[k])[ok]), k
        floor = 0.05 * 0.01 / r["dt"].max() if k in ("v_x", "v_y") else 0.05        # the 0.05 px floor in metres per second
        assert rel_err(g[ok], r[k][ok], floor=floor) <= TOL, k
    # the same call through the wrapped accessor of an installed pyorc (the test double)
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(32, engine="hip", **kw)
    finally:
        plugin.uninstall()
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(np.asarray(via[k]), np.asarray(ds[k]), equal_nan=True), k
