"""Multi-pass ensemble on the GPU against tests/ensemble_multipass_ref.py: the shifted ensemble pass at every
size and sample type through host stacks and DeviceFrames, the clamp, zero offsets, window and chunk independence in bits, the masks, the
float64 rescue at the offsets, and the chain through the public surface.  The inputs and their CPU checks (tie shares, values next to a
threshold or a half-integer): tests/test_ensemble_multipass_host.py.  The gate is tests/test_gpu_sliding.py's ``check_parity``."""
import numpy as np
import pytest

from pyorc_amd import DeviceFrames, _lib, frames, piv, velocimetry, window
from tests import ensemble_multipass_ref as ref
from tests import multipass_ref as mp

pytestmark = pytest.mark.gpu
TOL = 1e-4     # the project's gate: relative, floor 0.05 (px, or plane units)


def rel_err(got, want, floor=0.05):
    with np.errstate(all="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), floor)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


def run_pass(a, n, ov, shift, kw, chunks=None, signal_threshold=None, device_shift=False):
    """dict(u, v, count, planes, corr, s2n, shift, stats) of one Ensemble handle with the offsets ``shift`` fed with the frame slices
    ``chunks`` (default: the whole stack); corr / s2n as get_ffpiv forms them."""
    if device_shift and shift is not None:
        d = DeviceFrames.empty((1, 1, shift.nbytes), np.uint8)
        _lib.check(_lib.load().lspiv_memcpy_h2d(d.c_ptr, _lib.ptr(np.ascontiguousarray(shift)), shift.nbytes))
        shift = d
    e = piv.Ensemble(a.shape[1:], (n, n), (ov, ov), shift=shift)
    try:
        chunks = chunks or [(0, len(a))]
        cm, sn = (np.empty((len(a) - 1, e.n_rows * e.n_cols), np.float32) for _ in range(2))
        for f0, f1 in chunks:
            e.accumulate(a[f0:f1], kw["corr_min"], kw["s2n_min"], signal_threshold, out=(cm[f0:f1 - 1], sn[f0:f1 - 1]))
        u, v, cnt, planes = e.finish(kw["count_min"], 1, return_mean=True)
        corr, s2n = piv.ensemble_means(cm, sn, cnt, kw["count_min"], 1)
        shape = (1, e.n_rows, e.n_cols)
        return dict(u=u, v=v, count=cnt, planes=planes, corr=corr.reshape(shape), s2n=s2n.reshape(shape), shift=e.shift, stats=e.stats())
    finally:
        e.close()


def check_parity(got, r, where=None):
    """NaN masks identical, counts equal as integers, u, v, corr, s2n and the mean planes within the gate -- on the windows that are no ties."""
    ok = ~r["tie"] if where is None else where
    assert (~ok).mean() <= 0.01
    for k in ("u", "v", "corr", "s2n"):
        g = np.asarray(got[k])
        assert g.dtype == np.float32 and g.shape == r[k].shape, k
        assert np.array_equal(np.isnan(g)[ok], np.isnan(r[k])[ok]), k
        print(k, rel_err(g[ok], r[k][ok]))
        assert rel_err(g[ok], r[k][ok]) <= TOL, k
    assert np.array_equal(np.asarray(got["count"]).reshape(-1), r["count"])
    flat = ok.reshape(ok.shape[0], -1)
    planes = np.asarray(got["planes"])
    assert np.array_equal(np.isnan(planes)[flat], np.isnan(r["planes"])[flat])
    print("planes", rel_err(planes[flat], r["planes"][flat]))
    assert rel_err(planes[flat], r["planes"][flat]) <= TOL


def same_bits(x, y, keys=("u", "v", "count", "planes", "corr", "s2n")):
    for k in keys:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


# ---- 1. the shifted ensemble pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=["u8", "f32", "f64"])
@pytest.mark.parametrize("T", ref.PASS_FRAMES, ids=["5pairs", "6pairs"])
@pytest.mark.parametrize("n", list(ref.PASS_CASES))
def test_shifted_pass_matches_the_reference(gpu, n, T, dtype):
    m, ov, _ = ref.PASS_CASES[n]
    a, r, sh = ref.pass_stack(n, T, dtype), ref.pass_ref(n, T, dtype), ref.hand_shift(n)
    got = run_pass(a, m, ov, sh, ref.KW)
    assert np.array_equal(got["shift"], r["shift"])
    check_parity(got, r)
    assert got["stats"]["retain_complete"] and got["stats"]["flagged"] == got["stats"]["rescued"] + got["stats"]["float32_kept"]
    if dtype != np.float64:      # (float64 is narrowed while a host stack is staged; a DeviceFrames stack of float64 is read as it is)
        dev = run_pass(DeviceFrames.from_host(a), m, ov, sh, ref.KW, device_shift=True)
        same_bits(dev, got)
        assert np.array_equal(dev["shift"], got["shift"])
    else:
        check_parity(run_pass(DeviceFrames.from_host(a), m, ov, sh, ref.KW, device_shift=True), r)


# ---- 2. offsets outside the frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(ref.PASS_CASES))
def test_offsets_outside_the_frame_are_clamped(gpu, n):
    m, ov, dim = ref.PASS_CASES[n]
    a, far = ref.pass_stack(n), ref.far_shift(n)
    clamped = mp.clamp_shift(far, dim, m, ov).astype(np.int16)
    got = run_pass(a, m, ov, far, ref.OPEN_KW)            # (windows against unrelated content: masks that keep every plane)
    assert np.array_equal(got["shift"], clamped)
    same_bits(run_pass(a, m, ov, clamped, ref.OPEN_KW), got)
    check_parity(got, ref.pass_ref(n, shift="far", kw="OPEN"))


# ---- 3. zero or absent offsets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(ref.PASS_CASES))
def test_zero_offsets_are_the_plain_ensemble_within_the_gate(gpu, n):
    """An all-zero field runs the shifted kernel and gives the same bits however the field reaches the handle (host array, device array);
    the handle without a field is today's ensemble (two planes per inverse transform): the gate, not the bits."""
    m, ov, _ = ref.PASS_CASES[n]
    a, r = ref.pass_stack(n), ref.pass_ref(n, shift=None)
    zero = np.zeros(ref.grid_shape(n) + (2,), np.int16)
    got = run_pass(a, m, ov, zero, ref.KW)
    same_bits(run_pass(a, m, ov, zero, ref.KW, device_shift=True), got)
    assert not got["shift"].any()
    check_parity(got, r)
    plain = run_pass(a, m, ov, None, ref.KW)
    assert plain["shift"] is None
    check_parity(plain, r)
    assert np.array_equal(plain["count"], got["count"]) and np.array_equal(np.isnan(plain["u"]), np.isnan(got["u"]))
    for k in ("u", "v", "corr", "s2n", "planes"):
        assert rel_err(got[k], np.asarray(plain[k], dtype=np.float64)) <= TOL, k


# ---- 4. window independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(ref.PASS_CASES))
def test_one_windows_offset_changes_that_window_alone(gpu, n):
    m, ov, _ = ref.PASS_CASES[n]
    a, sh = ref.pass_stack(n), ref.hand_shift(n)
    rows, cols = ref.grid_shape(n)
    moved = sh.copy()
    moved[rows // 2, cols // 2] += np.array([2, -3], np.int16)
    w = (rows // 2) * cols + cols // 2
    base, got = run_pass(a, m, ov, sh, ref.KW), run_pass(a, m, ov, moved, ref.KW)
    others = np.arange(rows * cols) != w
    for k in ("u", "v", "corr", "s2n"):
        x, y = got[k].reshape(-1), base[k].reshape(-1)
        assert np.array_equal(x[others], y[others], equal_nan=True), k
    assert np.array_equal(got["planes"][0][others], base["planes"][0][others], equal_nan=True)
    assert np.array_equal(got["count"][others], base["count"][others])
    assert not np.array_equal(got["planes"][0][w], base["planes"][0][w]) and got["u"].reshape(-1)[w] != base["u"].reshape(-1)[w]


# ---- 5. chunk independence in bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(ref.PASS_CASES))
def test_chunking_does_not_change_a_bit(gpu, n):
    m, ov, dim = ref.PASS_CASES[n]
    a, sh = ref.pass_stack(n), ref.hand_shift(n)
    kw = dict(ref.KW, count_min=0.0)           # quirk Q3 (count_min * number of chunks) cannot bind
    whole = run_pass(a, m, ov, sh, kw)
    align = window.chunk_alignment((m, m), dim, (ov, ov))
    aligned = [(p, min(p + align, 6) + 1) for p in range(0, 6, align)] if align < 6 else [(0, 3), (2, 7)]
    for chunks in (aligned, [(0, 2), (1, 4), (3, 7)], [(0, 4), (3, 7)]):        # the last two start on the odd pairs 1 and 3
        same_bits(run_pass(a, m, ov, sh, kw, chunks), whole)
        same_bits(run_pass(DeviceFrames.from_host(a), m, ov, sh, kw, chunks), whole)


# ---- 6. masks -----------------------------------------------------------------------------------------------------------------------------
def test_signal_threshold_scores_the_shifted_window(gpu):
    m, ov, _ = ref.PASS_CASES[32]
    a, r = ref.signal_stack(), ref.signal_ref()
    got = run_pass(a, m, ov, ref.hand_shift(32), ref.KW, signal_threshold=ref.SIGNAL_THR)
    check_parity(got, r)
    assert np.isnan(got["u"]).any()
    same_bits(run_pass(DeviceFrames.from_host(a), m, ov, ref.hand_shift(32), ref.KW, signal_threshold=ref.SIGNAL_THR), got)


def run_public(a, chain, kw, **more):
    n, ov = chain[-1]
    nr, nc = window.get_array_shape(a.shape[1:], (n, n), (ov, ov))
    return velocimetry.get_ffpiv(a, np.arange(nr), np.arange(nc), np.ones(len(a) - 1), (n, n), (ov, ov), (n, n), 1.0, 1.0, ensemble_corr=True,
                                 coarse_passes=chain[:-1], **kw, **more)


def check_chain(a, chain, want, kw, **more):
    """``piv.ensemble_multipass`` pass by pass (offsets as integers, every pass within the gate) and ``get_ffpiv``: the same bits."""
    *res, per = piv.ensemble_multipass(a, chain, kw["corr_min"], kw["s2n_min"], kw["count_min"], return_passes=True, **more)
    for k, (r, (u, v, cnt, sh, planes)) in enumerate(zip(want, per)):
        if k:
            assert np.array_equal(sh, r["shift"]), k
        else:
            assert sh is None
        ok = ~r["tie"]
        assert np.array_equal(np.isnan(u)[ok], np.isnan(r["u"])[ok]) and np.array_equal(cnt, r["count"]), k
        assert rel_err(u[ok], r["u"][ok]) <= TOL and rel_err(v[ok], r["v"][ok]) <= TOL, k
    u, v, cnt, corr, s2n = res
    check_parity(dict(u=u, v=v, count=cnt, corr=corr, s2n=s2n, planes=per[-1][4]), want[-1])
    return dict(v_x=u, v_y=v, corr=corr, s2n=s2n)


def test_count_filter_and_the_predictor_skip_blanked_windows(gpu):
    a, want = ref.blanked_stack(), ref.blanked_chain()
    got = check_chain(a, ref.CHAINS["64"], want, ref.COUNT_KW)
    assert np.isnan(got["v_x"]).mean() > 0.1 and np.isfinite(got["v_x"]).any()
    ds = run_public(a, ref.CHAINS["64"], ref.COUNT_KW)
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(np.asarray(ds[k]), got[k], equal_nan=True), k


# ---- 7. rescue ----------------------------------------------------------------------------------------------------------------------------
def test_rescue_reads_the_window_at_its_offset(gpu):
    """On a stack that HAS ill-conditioned fits: windows are flagged, re-evaluated in float64 at their clamped offsets, and the offset
    is added after that -- every non-tie window passes the gate, in one accumulate call and in two, on host stacks and borrowed
    DeviceFrames."""
    n, ov = ref.RESCUE
    a, r, sh = ref.speckle_stack(), ref.speckle_ref(), ref.speckle_shift()
    got = run_pass(a, n, ov, sh, ref.KW)
    st = got["stats"]
    print(st)
    assert st["retain_complete"] and st["chunks_kept"] == 1 and st["flagged"] > 0
    assert st["flagged"] == st["rescued"] + st["float32_kept"] and st["rescued"] > 0
    check_parity(got, r)
    two = run_pass(a, n, ov, sh, ref.KW, [(0, 5), (4, 9)])
    assert two["stats"]["chunks_kept"] == 2 and (two["stats"]["flagged"], two["stats"]["rescued"]) == (st["flagged"], st["rescued"])
    same_bits(two, got, keys=("count", "planes", "corr", "s2n"))
    check_parity(two, r)
    dev = run_pass(DeviceFrames.from_host(a), n, ov, sh, ref.KW)
    assert dev["stats"]["retain_complete"] and (dev["stats"]["flagged"], dev["stats"]["rescued"]) == (st["flagged"], st["rescued"])
    same_bits(dev, got)


# ---- 8. the chain through the public surface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CHAINS))
def test_chain_through_the_public_surface(gpu, name, monkeypatch):
    a, chain, want = ref.river_stack(), ref.CHAINS[name], ref.river_chain(name)
    got = check_chain(a, chain, want, ref.DEFAULT_KW)
    assert ref.within_half_px(dict(u=got["v_x"], v=got["v_y"])) >= 0.90
    ds = run_public(a, chain, ref.DEFAULT_KW)
    runs = {"DeviceFrames": run_public(DeviceFrames.from_host(a), chain, ref.DEFAULT_KW),
            "two workers": run_public(a, chain, ref.DEFAULT_KW, devices=[0, 0]),
            "chunksize 4": run_public(a, chain, dict(ref.DEFAULT_KW, count_min=0.0), chunksize=4),
            "frames.get_piv": frames.get_piv(a, 16, ensemble_corr=True, coarse_passes=chain[:-1], resolution=1.0, time=np.arange(len(a)))}
    zero = run_public(a, chain, dict(ref.DEFAULT_KW, count_min=0.0))
    for label, other in runs.items():
        base = zero if label == "chunksize 4" else ds
        for k in ("v_x", "v_y", "corr", "s2n"):
            assert np.array_equal(np.asarray(other[k]), np.asarray(base[k]), equal_nan=True), (label, k)
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(np.asarray(ds[k]), got[k], equal_nan=True), k
    assert np.array_equal(np.asarray(ds.coords["time"]), [1])
    # two chunkings of every pass, the second chunk starting on the odd pair 3 (count_min = 0: the number of chunks cannot bind)
    args = (ref.DEFAULT_KW["corr_min"], ref.DEFAULT_KW["s2n_min"], 0.0)
    one, two = piv.ensemble_multipass(a, chain, *args), piv.ensemble_multipass(a, chain, *args, chunks=[(0, 4), (3, 7)])
    for x, y, z in zip(one, two, (zero["v_x"], zero["v_y"], None, zero["corr"], zero["s2n"])):
        assert np.array_equal(x, y, equal_nan=True)
        assert z is None or np.array_equal(x, np.asarray(z), equal_nan=True)
    # the same call through the wrapped accessor of an installed pyorc (the test double)
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(16, engine="hip", ensemble_corr=True, coarse_passes=[c[0] for c in chain[:-1]])
    finally:
        plugin.uninstall()
    assert np.array_equal(np.isnan(np.asarray(via["v_x"])), np.isnan(got["v_x"]))


# ---- 9. no coarse passes: today's ensemble ------------------------------------------------------------------------------------------------
def test_an_empty_chain_is_todays_ensemble(gpu):
    a = ref.river_stack()
    nr, nc = window.get_array_shape(a.shape[1:], (32, 32), (16, 16))
    args = (a, np.arange(nr), np.arange(nc), np.ones(len(a) - 1), (32, 32), (16, 16), (32, 32), 1.0, 1.0)
    today = velocimetry.get_ffpiv(*args, ensemble_corr=True, **ref.DEFAULT_KW)
    for cp in ([], None):
        got = velocimetry.get_ffpiv(*args, ensemble_corr=True, coarse_passes=cp, **ref.DEFAULT_KW)
        for k in ("v_x", "v_y", "corr", "s2n"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(today[k]), equal_nan=True), k


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------------
def test_calls_a_shifted_handle_refuses(gpu):
    a = ref.pass_stack(32)
    m, ov, dim = ref.PASS_CASES[32]
    sh = ref.hand_shift(32)
    with pytest.raises(ValueError, match="must be square and one of"):
        piv.Ensemble((70, 90), (24, 24), (12, 12), shift=np.zeros((4, 6, 2), np.int16))
    with pytest.raises(ValueError, match="shift must have shape"):
        piv.Ensemble(dim, (m, m), (ov, ov), shift=sh[:-1])
    with pytest.raises(NotImplementedError, match="sliding= and shift= exclude each other"):
        piv.Ensemble(dim, (m, m), (ov, ov), sliding=(4, 2), shift=sh)
    lib = _lib.load()
    e, plain, other = piv.Ensemble(dim, (m, m), (ov, ov), shift=sh), piv.Ensemble(dim, (m, m), (ov, ov)), piv.Ensemble(dim, (m, m), (ov, ov), shift=sh + 1)
    try:
        with pytest.raises(ValueError, match="shifted handle"):
            _lib.check(lib.lspiv_ensemble_set_sliding(e._h, 4, 2))
        for pair in ([e, plain], [e, other]):
            with pytest.raises(ValueError, match="other window offsets"):
                piv.ensemble_allreduce(pair)
        e.accumulate(a, 0.1, 1.5)
        with pytest.raises(ValueError, match="before the first accumulate"):
            _lib.check(lib.lspiv_ensemble_set_shift(e._h, _lib.ptr(sh)))
        _lib.check(lib.lspiv_ensemble_set_shift(plain._h, None))           # NULL on a plain handle: nothing to clear
        with pytest.raises(ValueError, match="not a shifted handle"):
            _lib.check(lib.lspiv_ensemble_get_shift(plain._h, _lib.ptr(np.empty_like(sh))))
        # export / import carry a shifted handle's sums as before: a second handle with the same offsets finishes to the same bits
        twin = piv.Ensemble(dim, (m, m), (ov, ov), shift=sh)
        try:
            twin.import_state(*e.export_state())
            old = _lib.get_option("rescue")
            _lib.set_option("rescue", 0)
            try:
                for x, y in zip(twin.finish(0.2, 1), e.finish(0.2, 1)):
                    assert np.array_equal(x, y, equal_nan=True)
            finally:
                _lib.set_option("rescue", old)
        finally:
            twin.close()
    finally:
        for h in (e, plain, other):
            h.close()
    for opt, val, msg in (("signal_mode", 1, "signal_mode = 1"), ("norm_clip", 0, "norm_clip = 0")):
        old = _lib.get_option(opt)
        try:
            if opt == "signal_mode":
                e = piv.Ensemble(dim, (m, m), (ov, ov), shift=sh)           # set_shift does not look at signal_mode ...
                _lib.set_option(opt, val)
                try:
                    with pytest.raises(ValueError, match=msg):              # ... the first accumulate does, as multi-pass PIV
                        e.accumulate(a, 0.1, 1.5, 0.2)
                finally:
                    e.close()
            else:
                _lib.set_option(opt, val)
                with pytest.raises(ValueError, match=msg):
                    piv.Ensemble(dim, (m, m), (ov, ov), shift=sh)
        finally:
            _lib.set_option(opt, old)
