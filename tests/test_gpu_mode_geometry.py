"""The mode PIV kernels (shifted pass, window deformation, SPOF, image mask, second peak, the shifted and SPOF ensemble passes) over the
geometry sweep of tests/mode_geometry_inputs.py: one window, one row and one column at stride 1, odd strides, oy != ox, an unread margin
and nine blocks at every window size -- origins at every alignment and job counts the parity inputs of those modes never produce.

Nothing is judged by a number of this file's own: every comparison with a float64 reference goes through the gate of the mode's own test
module (1e-4 on the results, 2e-6 on the planes; tests/test_gpu_search_area.py for the shifted and the deformed pass), imported as it
is.  tests/test_mode_geometry_host.py shows from the references alone that the geometries with fewer than 100 windows leave those gates
nothing to set aside, and that the larger ones stay within the gates' caps.

The deformation pass takes one overlap for both axes: it runs the six symmetric geometries, and is refused on the other two."""
import numpy as np
import pytest

from pyorc_amd import piv
from pyorc_amd.device import DeviceFrames
from tests import mode_geometry_inputs as mg
from tests.test_gpu_ensemble_multipass import check_parity
from tests.test_gpu_masked import gate as masked_gate
from tests.test_gpu_peak2 import gate as peak2_gate
from tests.test_gpu_search_area import gate as tie_gate
from tests.test_gpu_spof import ens_gate as spof_ens_gate
from tests.test_gpu_spof import gate as spof_gate

pytestmark = pytest.mark.gpu
BY_KEY = pytest.mark.parametrize("key", mg.KEYS, ids=mg.IDS)
BY_SYM_KEY = pytest.mark.parametrize("key", mg.SYM_KEYS, ids=mg.SYM_IDS)
BY_DTYPE = pytest.mark.parametrize("dtype", mg.DTYPES, ids=mg.DTYPE_IDS)
NAN_KEYS = [(name, n) for n in mg.SIZES for name in mg.NAN_NAMES]


def same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True), (what, k)


def call(mode, key, a, signal_threshold=None):
    """``mode`` at the geometry ``key`` on ``a`` (a host stack or DeviceFrames), with planes: (u, v, corr, s2n, planes), the second peak's
    (u, v, corr, s2n, peak2, planes)."""
    g = mg.GEOMETRIES[key]
    ws, ov = (g.n, g.n), g.overlap
    if mode == "shifted":
        return piv.piv_pairs_shifted(a, ws, ov, mg.offsets(key), signal_threshold, return_planes=True)
    if mode == "deformed":
        return piv.piv_pairs_deformed(a, ws, ov, mg.nodes(key), signal_threshold, return_planes=True)
    if mode == "spof":
        return piv.piv_pairs_filtered(a, ws, ov, "spof", signal_threshold, return_planes=True)
    if mode == "masked":
        return piv.piv_pairs_masked(a, ws, ov, mg.mask(key), signal_threshold=signal_threshold, return_planes=True)
    return piv.piv_pairs_peak2(a, ws, ov, mg.radii(g.n)[mode == "peak2-q"], signal_threshold, return_planes=True)


def check(mode, got, r, what):
    """The mode's own gate on a :func:`call` result."""
    print("----", what)
    if mode in ("shifted", "deformed"):
        tie_gate(got[:4], r, got[4])
    elif mode == "spof":
        spof_gate(got[:4], r, got[4])
    elif mode == "masked":
        masked_gate(got[:4], r, got[4], what=what)
    else:
        peak2_gate(got[4], got[5], r, what)
    print("windows set aside: %d of %d" % mg.set_aside(mode, r))


def parity(mode, key, dtype):
    """Device entry point against the reference; the host-fed one gives its bits for uint8 and float32 (a float64 host stack is narrowed
    to float32 while it is staged, in HBM it stays float64: there the gate)."""
    a, r = mg.stack(key, dtype), mg.ref(mode, key, dtype)
    what = f"{mode} {key[1]}-{key[0]} {np.dtype(dtype).name}"
    dev = call(mode, key, DeviceFrames.from_host(a))
    check(mode, dev, r, what + " device")
    host = call(mode, key, a)
    if dtype != np.float64:
        same_bits(host, dev, "host-fed and device entry points differ")
    else:
        check(mode, host, r, what + " host-fed")
    return dev


# ---- 1. per-pair parity with planes -----------------------------------------------------------------------------------------------------
@BY_DTYPE
@BY_KEY
def test_shifted_pass(gpu, key, dtype):
    parity("shifted", key, dtype)


@BY_DTYPE
@BY_SYM_KEY
def test_deformed_pass(gpu, key, dtype):
    parity("deformed", key, dtype)


@BY_DTYPE
@BY_KEY
def test_spof(gpu, key, dtype):
    dev = parity("spof", key, dtype)
    assert np.nanmax(dev[4]) <= 1.0 and np.nanmin(dev[4]) >= 0.0


@BY_DTYPE
@BY_KEY
def test_masked(gpu, key, dtype):
    parity("masked", key, dtype)


@BY_DTYPE
@BY_KEY
def test_second_peak_at_radius_1_and_a_quarter_window(gpu, key, dtype):
    for mode in ("peak2-1", "peak2-q"):
        dev = parity(mode, key, dtype)
        tie_gate(dev[:4], mg.ref("unshifted", key, dtype), dev[5])          # the primary: the shifted pass without offsets


def test_deformed_pass_refuses_two_overlaps(gpu):
    for key in sorted(set(mg.KEYS) - set(mg.SYM_KEYS)):
        for a in (mg.stack(key), DeviceFrames.from_host(mg.stack(key))):
            with pytest.raises(ValueError, match="one overlap for both axes"):
                call("deformed", key, a)


# ---- 2. the signal-threshold variant ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", mg.MODES)
@BY_KEY
def test_signal_threshold(gpu, key, mode):
    if mode == "deformed" and key not in mg.SYM_KEYS:
        with pytest.raises(ValueError, match="one overlap for both axes"):
            call(mode, key, mg.signal_stack(key), mg.SIGNAL_THR)
        return
    a, r = mg.signal_stack(key), mg.signal_ref(mode, key)
    dev = call(mode, key, DeviceFrames.from_host(a), mg.SIGNAL_THR)
    check(mode, dev, r, f"{mode} {key[1]}-{key[0]} signal")
    same_bits(call(mode, key, a, mg.SIGNAL_THR), dev, "host-fed and device entry points differ")


# ---- 3. identities that need no reference -----------------------------------------------------------------------------------------------
@BY_DTYPE
@BY_KEY
def test_identities_between_the_modes(gpu, key, dtype):
    g = mg.GEOMETRIES[key]
    ws, ov = (g.n, g.n), g.overlap
    rows, cols = mg.grid(key)
    d = DeviceFrames.from_host(mg.stack(key, dtype))
    none = piv.piv_pairs_shifted(d, ws, ov, None, return_planes=True)
    same_bits(piv.piv_pairs_shifted(d, ws, ov, np.zeros((g.T - 1, rows, cols, 2), np.int16), return_planes=True), none, "all-zero offsets")
    for r in mg.radii(g.n):
        *res, p2, planes = piv.piv_pairs_peak2(d, ws, ov, r, return_planes=True)
        same_bits(res + [planes], none, "the shifted kernel without offsets")
        same_bits([piv.second_peak(planes, r).reshape(p2.shape)], [p2], "second_peak on the kernel's own planes")
    if key in mg.SYM_KEYS:
        zero = piv.piv_pairs_deformed(d, ws, ov, None, return_planes=True)
        same_bits(piv.piv_pairs_deformed(d, ws, ov, np.zeros((g.T - 1, rows, cols, 2), np.int32), return_planes=True), zero, "all-zero nodes")
        if dtype == np.float32:     # (tests/test_gpu_deform.py: on float32 stacks the mixed-type kernel keeps the shifted kernel's arithmetic order)
            same_bits(zero, none, "zero nodes against the shifted kernel at zero offsets")


# ---- 4. one NaN sample --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("spof", "masked", "peak2-q", "deformed"))
@pytest.mark.parametrize("key", NAN_KEYS, ids=[f"{n}-{name}" for name, n in NAN_KEYS])
def test_a_nan_sample_takes_out_the_windows_that_hold_it_and_no_others(gpu, key, mode):
    """Frame 0 is the window of frame t of pair 0 alone (and is never warped): exactly the windows of pair 0 whose rectangle holds the
    sample -- a valid one of the mask -- are NaN, every other window keeps the clean run's bits."""
    a = mg.stack(key, np.float32)
    y, x = mg.nan_sample(key)
    clean = call(mode, key, DeviceFrames.from_host(a))
    b = a.copy()
    b[0, y, x] = np.nan
    got = call(mode, key, DeviceFrames.from_host(b))
    hit = np.zeros(clean[0].shape, bool)
    hit[0] = mg.windows_holding(key, y, x)
    assert 2 <= hit.sum() < hit[0].size
    for g, c in zip(got[:4], clean[:4]):
        assert np.isnan(g[hit]).all() and np.array_equal(g[~hit], c[~hit], equal_nan=True)
    flat = hit.reshape(hit.shape[0], -1)
    assert np.isnan(got[-1][flat]).all() and np.array_equal(got[-1][~flat], clean[-1][~flat], equal_nan=True)
    if mode == "peak2-q":
        assert np.isnan(got[4][hit]).all() and np.array_equal(got[4][~hit], clean[4][~hit], equal_nan=True)
    if mode != "masked":            # (under the mask a window below k_min is NaN with or without the sample)
        assert np.isfinite(clean[2][hit]).all()


# ---- 5. the ensemble passes ---------------------------------------------------------------------------------------------------------------
def run_ensemble(a, key, kw, **handle):
    """dict(u, v, count, planes, corr, s2n, shift, stats) of one Ensemble handle (``shift=`` or ``spectral_filter=``) fed with the whole
    stack; corr / s2n as get_ffpiv forms them."""
    g = mg.GEOMETRIES[key]
    e = piv.Ensemble(g.dim, (g.n, g.n), g.overlap, **handle)
    try:
        cm, sn = e.accumulate(a, kw["corr_min"], kw["s2n_min"])
        u, v, cnt, planes = e.finish(kw["count_min"], 1, return_mean=True)
        corr, s2n = piv.ensemble_means(cm, sn, cnt, kw["count_min"], 1)
        shape = (1, e.n_rows, e.n_cols)
        return dict(u=u, v=v, count=cnt, planes=planes, corr=corr.reshape(shape), s2n=s2n.reshape(shape), shift=e.shift, stats=e.stats())
    finally:
        e.close()


ENS_KEYS = ("u", "v", "count", "planes", "corr", "s2n")


@pytest.mark.parametrize("dtype", mg.DTYPES[:2], ids=mg.DTYPE_IDS[:2])
@BY_KEY
def test_shifted_ensemble_pass(gpu, key, dtype):
    a, r = mg.stack(key, dtype), mg.ref("shifted-ensemble", key, dtype)
    got = run_ensemble(a, key, mg.emp.OPEN_KW, shift=mg.offsets(key)[0])
    assert np.array_equal(got["shift"], r["shift"])
    print("---- shifted-ensemble", f"{key[1]}-{key[0]}", np.dtype(dtype).name)
    check_parity(got, r)
    print("windows set aside: %d of %d" % mg.set_aside("shifted-ensemble", r))
    dev = run_ensemble(DeviceFrames.from_host(a), key, mg.emp.OPEN_KW, shift=mg.offsets(key)[0])
    same_bits([dev[k] for k in ENS_KEYS + ("shift",)], [got[k] for k in ENS_KEYS + ("shift",)], "host and device stacks differ")


@pytest.mark.parametrize("dtype", mg.DTYPES[:2], ids=mg.DTYPE_IDS[:2])
@BY_KEY
def test_spof_ensemble(gpu, key, dtype):
    a, r = mg.stack(key, dtype), mg.ref("spof-ensemble", key, dtype)
    got = run_ensemble(a, key, mg.SPOF_ENS_KW, spectral_filter="spof")
    print("---- spof-ensemble", f"{key[1]}-{key[0]}", np.dtype(dtype).name)
    spof_ens_gate(got, r)
    print("windows set aside: %d of %d" % mg.set_aside("spof-ensemble", r))
    dev = run_ensemble(DeviceFrames.from_host(a), key, mg.SPOF_ENS_KW, spectral_filter="spof")
    same_bits([dev[k] for k in ENS_KEYS], [got[k] for k in ENS_KEYS], "host and device stacks differ")
