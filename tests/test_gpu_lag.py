"""The per-window frame lag on the GPU against tests/lag_ref.py, the float64 reference.  Gate, the multi-pass
tests' own: NaN masks identical, u, v, corr, s2n within 1e-4 (of max(|ref|, 0.05)), planes within 2e-6; only windows whose reference plane
has an exact float64 tie for its maximum are set aside, at most 1 % of a case; lags and clamped offsets are compared as integers.  The
inputs are checked on the CPU (tests/test_lag_host.py)."""
import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import lag_ref as ref
from tests import multipass_ref as mp
from tests.test_gpu_search_area import TOL, gate, rel_err

pytestmark = pytest.mark.gpu
SIZES = ref.LAG_WINDOWS
FORMS = ("int", "array", "adaptive")


def same_bits(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w, equal_nan=True), (what, k)


def lagged(a, n, form, **kw):
    """``piv_pairs_lagged`` of a parity input: [u, v, corr, s2n], lag, planes, shift."""
    m, ov, _ = ref.PASS_CASES[n]
    *res, lag, planes, shift = piv.piv_pairs_lagged(a, (m, m), (ov, ov), **ref.parity_kw(n, form), return_planes=True, return_shift=True, **kw)
    return res, lag, planes, shift


def check(got, r):
    res, lag, planes, shift = got
    assert lag.dtype == np.uint8 and shift.dtype == np.int16
    assert np.array_equal(lag, r["lag"]) and np.array_equal(shift, r["shift"])       # the reference's integers
    gate(res, r, planes)


# ---- 1. parity against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=("u8", "f32", "f64"))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_parity_host_and_device_entry(gpu, n, form, dtype):
    a = ref.pass_stack(n, dtype)
    r = ref.parity_ref(n, form, dtype)
    host = lagged(a, n, form)
    check(host, r)
    dev = lagged(DeviceFrames.from_host(a), n, form)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(dev[0] + [dev[1], dev[2], dev[3]], host[0] + [host[1], host[2], host[3]], "host and device entry points differ")
    else:
        check(dev, r)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_signal_threshold_scores_the_lagged_window(gpu, n, form):
    a = ref.signal_stack(n)
    r = ref.parity_ref(n, form, np.uint8, True)
    check(lagged(a, n, form, signal_threshold=ref.SIGNAL_THR), r)
    check(lagged(DeviceFrames.from_host(a.astype(np.float32)), n, form, signal_threshold=ref.SIGNAL_THR), r)


@pytest.mark.parametrize("name", sorted(ref.SMALL_GRIDS))
def test_small_and_odd_grids(gpu, name):
    """A grid whose job count is no multiple of the jobs per block and grids of one row / one window (tests/lag_ref.py, SMALL_GRIDS): jobs
    past the end store nothing, the predictor's neighbourhood is clipped on every side.  (The adaptive inputs sit off the predictor's
    rounding boundaries: tests/test_lag_host.py.)"""
    n, ov, dim = ref.SMALL_GRIDS[name]
    a = ref.small_stack(name)
    for form, kw in (("array", dict(pair_step=ref.small_lags(name))), ("adaptive", dict(pair_step="adaptive", pair_step_max=ref.SMALL_K))):
        r = ref.small_ref(name, form)
        *res, lag, planes, shift = piv.piv_pairs_lagged(DeviceFrames.from_host(a), (n, n), (ov, ov), **kw, return_planes=True, return_shift=True)
        assert np.array_equal(lag, r["lag"]) and np.array_equal(shift, r["shift"]), name
        gate(res, r, planes)


@pytest.mark.parametrize("n", SIZES)
def test_a_caller_s_table_and_offsets_through_the_c_abi(gpu, n):
    """LSPIV_LAG_TABLE with explicit int16 offsets, which the Python layer never passes: both entry points, 4 pairs of a 7-frame stack (the
    rest is the call's halo), a table whose 0 and 200 are clamped to 1 and to the frames left, offsets the frame clamp changes."""
    import ctypes as C

    lib = gpu
    m, ov, (H, W) = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    T, P = len(a), ref.TABLE_PAIRS
    rows, cols = ref.grid_shape(n)
    lag, sh = (np.ascontiguousarray(q) for q in ref.table_case(n))
    r = ref.table_ref(n)
    # the host-fed entry point
    res = [np.empty((P, rows, cols), np.float32) for _ in range(4)]
    planes = np.empty((P, rows * cols, m, m), np.float32)
    lag_out, sh_out = np.empty((P, rows, cols), np.uint8), np.empty((P, rows, cols, 2), np.int16)
    _lib.check(lib.lspiv_piv_lag_pairs_at(_lib.ptr(a), 0, T, P, H, W, m, m, ov, ov, -1.0, 0, window.LAG_TABLE, 0, 0, _lib.ptr(lag), _lib.ptr(sh),
                                          *(_lib.ptr(q) for q in res), _lib.ptr(planes), _lib.ptr(lag_out), _lib.ptr(sh_out)))
    check((res, lag_out, planes, sh_out), r)
    # the device entry point; the clamped offsets written over the caller's own
    d = DeviceFrames.from_host(a)
    d_res, d_planes = DeviceFrames.empty((4, P, rows * cols), np.float32), DeviceFrames.empty((P * rows * cols, m, m), np.float32)
    d_lag, d_lag_out, d_sh = DeviceFrames.from_host(lag), DeviceFrames.empty((P, rows, cols), np.uint8), DeviceFrames.from_host(sh.view(np.uint8).reshape(P, rows, cols * 4))
    _lib.check(lib.lspiv_piv_lag_pairs_dev_at(d.c_ptr, 0, T, P, H, W, m, m, ov, ov, -1.0, 0, window.LAG_TABLE, 0, 0, d_lag.c_ptr, d_sh.c_ptr, d_res.c_ptr,
                                              d_planes.c_ptr, d_lag_out.c_ptr, d_sh.c_ptr, None))
    dev = d_res.to_host().reshape(4, P, rows, cols)
    same_bits(list(dev) + [d_lag_out.to_host(), d_planes.to_host().reshape(planes.shape), d_sh.to_host().view(np.int16).reshape(sh.shape)],
              res + [lag_out, planes, sh_out], "host and device entry points differ")
    # what the header rules out
    for form, k, t128, lag_ptr, sh_ptr, what in ((window.LAG_ADAPTIVE, 4, 1024, d_lag.c_ptr, None, "d_lag"), (window.LAG_ADAPTIVE, 4, 1024, None, d_sh.c_ptr, "d_shift"),
                                               (window.LAG_TABLE, 0, 0, None, None, "lag array"), (window.LAG_UNIFORM, 17, 0, None, None, "lag 17"), (4, 1, 0, None, None, "lag_form")):
        rc = lib.lspiv_piv_lag_pairs_dev_at(d.c_ptr, 0, T, P, H, W, m, m, ov, ov, -1.0, 0, form, k, t128, lag_ptr, sh_ptr, d_res.c_ptr, None, d_lag_out.c_ptr, None, None)
        assert rc == _lib.LSPIV_EINVAL and what in lib.lspiv_last_error().decode(), what
    assert lib.lspiv_piv_lag_pairs_dev_at(d.c_ptr, 0, T, T, H, W, m, m, ov, ov, -1.0, 0, 0, 2, 0, None, None, d_res.c_ptr, None, d_lag_out.c_ptr, None, None) == _lib.LSPIV_ESHAPE


# ---- 2. bit-equality with what exists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_a_uniform_array_is_the_shifted_kernel_on_every_residue_class(gpu, n, k):
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    d = DeviceFrames.from_host(a)
    *res, lag, planes = piv.piv_pairs_lagged(d, (m, m), (ov, ov), np.full(ref.grid_shape(n), k), return_planes=True)
    seen = 0
    for r in range(k):
        sub = np.ascontiguousarray(a[r::k])
        if len(sub) < 2:
            continue
        us, vs, cs, ss, ps = piv.piv_pairs_shifted(DeviceFrames.from_host(sub), (m, m), (ov, ov), None, return_planes=True)
        for j in range(len(sub) - 1):
            t = r + j * k
            assert (lag[t] == k).all()
            same_bits([res[2][t], res[3][t], planes[t]], [cs[j], ss[j], ps[j]], f"corr, s2n, plane of pair {t}")
            same_bits([res[0][t], res[1][t]], [us[j] / np.float32(k), vs[j] / np.float32(k)], f"u, v of pair {t}")
            seen += 1
    assert seen == len(a) - k                                       # every pair whose lag the stack does not clip


@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=("u8", "f32", "f64"))
@pytest.mark.parametrize("n", SIZES)
def test_an_all_ones_array_is_the_shifted_kernel_at_zero_offsets(gpu, n, dtype):
    m, ov, _ = ref.PASS_CASES[n]
    d = DeviceFrames.from_host(ref.pass_stack(n, dtype))
    *res, lag, planes = piv.piv_pairs_lagged(d, (m, m), (ov, ov), np.ones(ref.grid_shape(n), dtype=np.int32), 4, None, 0.1, return_planes=True)
    assert (lag == 1).all()
    same_bits(res + [planes], piv.piv_pairs_shifted(d, (m, m), (ov, ov), None, 0.1, return_planes=True), "all-ones array")


@pytest.mark.parametrize("n", SIZES)
def test_pair_step_one_is_the_call_without_the_keyword(gpu, n):
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    for x in (a, DeviceFrames.from_host(a)):
        *res, lag, planes = piv.piv_pairs_lagged(x, (m, m), (ov, ov), 1, return_planes=True)
        same_bits(res + [planes], piv.piv_pairs(x, (m, m), (ov, ov), return_planes=True), "pair_step = 1")
        assert lag.dtype == np.uint8 and (lag == 1).all()
    y, x = (np.arange(q) for q in ref.grid_shape(n))
    kw = dict(window_size=(m, m), overlap=(ov, ov), search_area_size=(m, m), res_y=0.02, res_x=0.03)
    plain = velocimetry.get_ffpiv(a, y, x, np.full(len(a) - 1, 0.04), **kw)
    one = velocimetry.get_ffpiv(a, y, x, np.full(len(a) - 1, 0.04), pair_step=1, **kw)
    same_bits([np.asarray(one[key]) for key in ("s2n", "corr", "v_x", "v_y")], [np.asarray(plain[key]) for key in ("s2n", "corr", "v_x", "v_y")])
    assert "pair_step" not in plain and np.asarray(one["pair_step"]).dtype == np.uint8 and (np.asarray(one["pair_step"]) == 1).all()


def test_end_of_stack(gpu):
    a = ref.pass_stack(32)[:5]
    *_, lag = piv.piv_pairs_lagged(a, (32, 32), (16, 16), 3)
    assert lag.shape == (4, *ref.grid_shape(32)) and [np.unique(lag[t]).tolist() for t in range(4)] == [[3], [3], [2], [1]]
    *_, lag = piv.piv_pairs_lagged(DeviceFrames.from_host(a), (32, 32), (16, 16), "adaptive", 16, 16.0)
    assert (lag <= np.array([4, 3, 2, 1])[:, None, None]).all() and lag[0].max() == 4


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["array", "adaptive"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "DeviceFrames"])
def test_chunks_with_their_halo_give_the_bits_of_one_launch(gpu, form, on_device):
    """Chunks of 1, 2 and 3 pairs, odd starts included, each with min(largest lag, frames to the end) halo frames.  (The adaptive form's
    lag-1 pass runs the walking kernel, whose last bit may depend on where a chunk starts; the lags and offsets it is turned into are
    integers, and the lagged pass is pair-local -- the inputs sit off the predictor's rounding boundaries, tests/test_lag_host.py.)"""
    n = 32
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    T = len(a)
    kw = ref.parity_kw(n, form)
    halo = 4 if form == "array" else ref.ADAPTIVE[n][0]
    stack = DeviceFrames.from_host(a) if on_device else a
    whole = piv.piv_pairs_lagged(stack, (m, m), (ov, ov), **kw, return_planes=True, return_shift=True)
    for cuts in ([0, 1, 2, 3, 4, 5, 6], [0, 1, 3, 6], [0, 3, 6], [0, 2, 5, 6]):
        parts = []
        for p0, p1 in zip(cuts, cuts[1:]):
            end = min(p1 + halo, T)
            parts.append(piv.piv_pairs_lagged(stack[p0:end], (m, m), (ov, ov), **kw, return_planes=True, return_shift=True, pairs=p1 - p0,
                                              pair_offset=p0))
        same_bits([np.concatenate(q) for q in zip(*parts)], whole, f"cuts {cuts}")


@pytest.mark.parametrize("form", FORMS)
def test_get_ffpiv_chunked_and_the_dataset(gpu, form):
    n = 32
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    y, x = (np.arange(q) for q in ref.grid_shape(n))
    dt = np.linspace(0.03, 0.05, len(a) - 1)
    kw = dict(window_size=(m, m), overlap=(ov, ov), search_area_size=(m, m), res_y=0.02, res_x=0.03, **ref.parity_kw(n, form))
    one = velocimetry.get_ffpiv(a, y, x, dt, **kw)
    u, v, cm, sn, lag = piv.piv_pairs_lagged(a, (m, m), (ov, ov), **ref.parity_kw(n, form))
    assert set(one) == {"s2n", "corr", "v_x", "v_y", "pair_step"} and np.array_equal(np.asarray(one["pair_step"]), lag)
    same_bits([np.asarray(one[k]) for k in ("s2n", "corr")], [sn, cm])
    same_bits([np.asarray(one["v_x"]), np.asarray(one["v_y"])],
              [(u * 0.03 / dt[:, None, None]).astype(np.float32), (v * 0.02 / dt[:, None, None]).astype(np.float32)], "px -> m/s")
    assert np.array_equal(np.asarray(one.coords["time"]), np.arange(1, len(a)))
    if form != "adaptive":       # (the adaptive form cuts on the anchors of its lag-1 pass: this stack is shorter than one)
        small = velocimetry.get_ffpiv(a, y, x, dt, chunksize=3, **kw)
        same_bits([np.asarray(small[k]) for k in sorted(one)], [np.asarray(one[k]) for k in sorted(one)], "chunksize = 3")
    dev = velocimetry.get_ffpiv(DeviceFrames.from_host(a), y, x, dt, **kw)
    same_bits([np.asarray(dev[k]) for k in sorted(one)], [np.asarray(one[k]) for k in sorted(one)], "DeviceFrames")
    ds = frames.get_piv(a, m, overlap=(ov, ov), **ref.parity_kw(n, form))
    assert np.array_equal(np.asarray(ds["pair_step"]), lag)


# ---- 4. the predictor entry point alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_max,target", [(4, None), (8, 4.0), (16, 8.0), (1, 0.3)])
def test_predictor_entry_point_value_for_value(gpu, k_max, target):
    u, v = ref.hand_fields()
    want = ref.predict_lag(u, v, ref.HAND_DIM, ref.HAND_N, ref.HAND_OV, ref.HAND_T, k_max, target)
    got = piv.predict_lag(u, v, ref.HAND_DIM, (ref.HAND_N, ref.HAND_N), (ref.HAND_OV, ref.HAND_OV), ref.HAND_T, k_max, target)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int16
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a longer stack behind the same pairs lifts the clip
    want = ref.predict_lag(u, v, ref.HAND_DIM, ref.HAND_N, ref.HAND_OV, 40, k_max, target)
    got = piv.predict_lag(u, v, ref.HAND_DIM, (ref.HAND_N, ref.HAND_N), (ref.HAND_OV, ref.HAND_OV), 40, k_max, target)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 5. the float64 rescue pass under a lag --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=("u8", "f32"))
@pytest.mark.parametrize("n,ov", mp.RESCUE_GEOMETRIES, ids=[f"{n}@{ov}" for n, ov in mp.RESCUE_GEOMETRIES])
def test_rescue_reads_the_lagged_frame(gpu, n, ov, dtype):
    """Single-pixel speckles drifting 1 px per frame (the ambiguity input of the multi-pass rescue tests, one frame longer): at a lag of 2
    every peak still sits on exactly-zero neighbours, so windows are flagged and re-fitted in float64 -- from frame t + 2."""
    from tests import sliding_ref

    a = sliding_ref.as_samples(sliding_ref.speckle_stack(T=mp.RESCUE_T + 1, H=mp.RESCUE_DIM[0], W=mp.RESCUE_DIM[1], seed=11), dtype)
    rows, cols = (len(q) for q in mp.grid_origins(mp.RESCUE_DIM, n, ov))
    r = ref.lagged_piv(a.astype(np.float64), n, ov, ref.table(2, len(a), len(a) - 1, (rows, cols)))

    def run(x):
        *res, lag, planes = piv.piv_pairs_lagged(x, (n, n), (ov, ov), 2, return_planes=True)
        assert np.array_equal(lag, r["lag"])
        return res, planes

    def uv_err(res):
        ok = ~r["tie"]
        return max(rel_err(res[0][ok], r["u"][ok]), rel_err(res[1][ok], r["v"][ok]))

    on, planes = run(a)
    gate(on, r, planes)
    dev, dplanes = run(DeviceFrames.from_host(a))
    same_bits(dev + [dplanes], on + [planes], "host and device entry points differ")
    old = _lib.get_option("rescue")
    _lib.set_option("rescue", 0)
    try:
        off, _ = run(a)
    finally:
        _lib.set_option("rescue", old)
    print("u, v error with the pass", uv_err(on), "without", uv_err(off))
    assert uv_err(on) <= TOL < uv_err(off)                          # at least one window misses the gate without the pass


# ---- 6. options ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,val", [("border_peak", 1), ("border_peak", 2), ("std_ddof", 1), ("v_sign", 1)])
def test_options_follow_the_reference(gpu, opt, val):
    n = 16                                                         # (a lag of 3 puts a fifth of this input's peaks on the plane border)
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    _lib.set_option(opt, val)
    try:
        with po.semantics(**{opt: val}):
            want = {form: (ref.adaptive(a.astype(np.float64), m, ov, *ref.ADAPTIVE[n]) if form == "adaptive" else
                           ref.lagged_piv(a.astype(np.float64), m, ov, ref.table(ref.INT_LAG, len(a), len(a) - 1, ref.grid_shape(n))))
                    for form in ("int", "adaptive")}
        got = {form: lagged(a, n, form) for form in want}
        for form in want:
            check(got[form], want[form])
        if opt == "v_sign":
            _lib.set_option(opt, 0)
            off = lagged(a, n, "adaptive")
            same_bits([got["adaptive"][0][0], -got["adaptive"][0][1], got["adaptive"][1], got["adaptive"][3]], [off[0][0], off[0][1], off[1], off[3]],
                      "v_sign is applied last: the same lags and offsets")
        if opt == "border_peak":
            assert np.isfinite(got["int"][0][0]).all() and np.isnan(ref.parity_ref(n, "int")["u"]).any()
    finally:
        _lib.set_option(opt, 0)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    a = ref.pass_stack(32)
    for opt, val, back in (("norm_clip", 0, 1), ("signal_mode", 1, 0)):
        _lib.set_option(opt, val)
        try:
            for call in (lambda: piv.piv_pairs_lagged(a, (32, 32), (16, 16), 2), lambda: piv.piv_pairs_lagged(DeviceFrames.from_host(a), (32, 32), (16, 16), "adaptive")):
                with pytest.raises(ValueError, match=opt) as e:
                    call()
                assert e.value.code == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, back)
    lib = _lib.load()
    assert [lib.lspiv_lag_supported(w, w) for w in (8, 16, 24, 32, 64, 128)] == [0, 1, 0, 1, 1, 0] and not lib.lspiv_lag_supported(32, 16)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        piv.piv_pairs_lagged(a, (24, 24), (12, 12), 2)
    with pytest.raises(ValueError, match="grid's shape"):
        piv.piv_pairs_lagged(a, (32, 32), (16, 16), np.ones((2, 2), int))
    with pytest.raises(ValueError, match="pairs must lie"):
        piv.piv_pairs_lagged(a, (32, 32), (16, 16), 2, pairs=len(a))
    y, x = (np.arange(q) for q in ref.grid_shape(32))
    kw = dict(window_size=(32, 32), overlap=(16, 16), search_area_size=(32, 32), res_y=0.01, res_x=0.01)
    for other in (dict(ensemble_corr=True), dict(coarse_passes=[64]), dict(peak_ratio=True), dict(validate=True), dict(devices="all")):
        with pytest.raises(NotImplementedError, match="pair_step") as e:
            velocimetry.get_ffpiv(DeviceFrames.from_host(a), y, x, np.ones(len(a) - 1), pair_step=2, **kw, **other)
        assert next(iter(other)) in str(e.value)


def test_the_wrapped_accessor_takes_the_keywords(gpu, monkeypatch):
    """``Frames.get_piv(engine="hip", pair_step=...)`` through the accessor double: the dataset gains ``pair_step``; a refused combination
    is refused there too, and the keywords belong to this engine alone."""
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    n = 32
    m, ov, _ = ref.PASS_CASES[n]
    a = ref.pass_stack(n)
    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(m, engine="hip", pair_step=3)
        want = frames.get_piv(a, m, pair_step=3)
        assert np.array_equal(np.asarray(via["pair_step"]), ref.parity_ref(n, "int")["lag"])
        same_bits([np.asarray(via[k]) for k in ("s2n", "corr", "v_x", "v_y")], [np.asarray(want[k]) for k in ("s2n", "corr", "v_x", "v_y")], "wrapped accessor")
        via = rd.Frames(a).get_piv(m, engine="hip", pair_step="adaptive", pair_step_max=ref.ADAPTIVE[n][0], pair_step_target=ref.ADAPTIVE[n][1])
        assert np.array_equal(np.asarray(via["pair_step"]), ref.parity_ref(n, "adaptive")["lag"])
        assert "pair_step" in rd.Frames(a).get_piv(m, engine="hip", pair_step=1) and "pair_step" not in frames.get_piv(a, m)
        with pytest.raises(NotImplementedError, match="pair_step together with peak_ratio"):
            rd.Frames(a).get_piv(m, engine="hip", pair_step=3, peak_ratio=True)
        with pytest.raises(ValueError, match="pair_step_max"):
            rd.Frames(a).get_piv(m, engine="hip", pair_step="adaptive", pair_step_max=17)
        from tests import lazy_doubles

        lazy = lazy_doubles.from_frames(a, block=3).map_time(lambda blk: blk, "touch")      # what a real pyorc hands over: dask-backed
        with pytest.raises(NotImplementedError, match="pair_step with a lazy stack"):
            rd.Frames(lazy).get_piv(m, engine="hip", pair_step=3)
        assert lazy.calls == {}
    finally:
        plugin.uninstall()


# ---- 8. the benefit on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ov", ref.PROFILE_CASES)
def test_adaptive_lags_cut_the_error_of_slow_windows_on_the_device(gpu, n, ov):
    d = DeviceFrames.from_host(ref.profile_stack())
    u1, v1, *_ = piv.piv_pairs(d, (n, n), (ov, ov))
    ua, va, _, _, lag = piv.piv_pairs_lagged(d, (n, n), (ov, ov), "adaptive", ref.PROFILE_K)
    e1, ea = ref.slow_median_error(u1, v1, n, ov), ref.slow_median_error(ua, va, n, ov)
    print(f"{n} @ {ov}: slow-window median error {e1:.5f} px/frame at lag 1, {ea:.5f} adaptive: {ea / e1:.3f} x; lags", np.unique(lag).tolist())
    assert ea <= 0.5 * e1
