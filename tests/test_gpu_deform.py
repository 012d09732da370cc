"""Window deformation passes on the GPU against tests/deform_ref.py, the float64 reference.  Gate: NaN
masks identical, u, v, corr, s2n and the planes within 1e-4 (of max(|ref|, 0.05)) on the windows whose reference plane has no exact
float64 tie for its maximum (at most 1 % of a case).  Both sides always get the SAME nodes -- a chain is compared pass by pass, the
reference fed with the GPU's own previous pass: a previous-pass u within 1e-4 of a half-unit may land on the other side of the rint on
the two sides.  The predictor is compared as integers.  Inputs, tie shares and signal fractions are checked on the CPU
(tests/test_deform_host.py)."""
import numpy as np
import pytest

from pyorc_amd import _lib, executor, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import deform_ref as ref
from tests import multipass_ref as mp
from tests.test_gpu_multipass import KEYS, _Lazy, same_bits
from tests.test_gpu_search_area import rel_err
from tests.test_multipass_host import long_stack

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = list(ref.PASS_CASES)


def gate(got, r, planes=None, where=None):
    u, v, cm, sn = got
    ok = ~r["tie"] if where is None else where & ~r["tie"]
    assert r["tie"].mean() <= 0.01
    assert u.dtype == v.dtype == cm.dtype == sn.dtype == np.float32 and u.shape == r["u"].shape
    for name, g, x in (("u", u, r["u"]), ("v", v, r["v"]), ("corr", cm, r["corr"]), ("s2n", sn, r["s2n"])):
        assert np.array_equal(np.isnan(g)[ok], np.isnan(x)[ok]), f"{name}: NaN mask differs"
        print(name, rel_err(g[ok], x[ok]))
        assert rel_err(g[ok], x[ok]) <= TOL, name
    if planes is not None:
        flat = ok.reshape(ok.shape[0], -1)
        assert np.array_equal(np.isnan(planes)[flat], np.isnan(r["planes"])[flat])
        print("planes", rel_err(planes[flat], r["planes"][flat]))
        assert rel_err(planes[flat], r["planes"][flat]) <= TOL


def geometry(case):
    n, ov, dim = ref.PASS_CASES[case] if case in ref.PASS_CASES else ref.GRID_CASES[case]
    return n, ov, dim


# ---- 1. the predictor -------------------------------------------------------------------------------------------------------------------
def hand_field(rng, P, rows, cols, scale):
    u = (rng.standard_normal((P, rows, cols)) * scale).astype(np.float32)
    v = (rng.standard_normal((P, rows, cols)) * scale).astype(np.float32)
    half = rng.random((P, rows, cols)) < 0.25                      # exact half-units k / 64 + 1 / 128: a float32 tie of the rint
    u[half] = (np.rint(u[half] * 64) / 64 + 1 / 128).astype(np.float32)
    other = ~half & (rng.random((P, rows, cols)) < 0.25)
    v[other] = (np.rint(v[other] * 64) / 64 - 1 / 128).astype(np.float32)
    for _ in range(3):                                             # NaN patches, in one component or both
        p, r, c = rng.integers(P), rng.integers(rows), rng.integers(cols)
        (u if rng.random() < 0.5 else v)[p, r:r + 3, c:c + 2] = np.nan
    u[rng.random((P, rows, cols)) < 0.05] = np.inf
    big = rng.random((P, rows, cols)) < 0.1                        # finite values far beyond any frame, up to the largest float32
    v[big] = rng.choice(np.array([3.3e38, -3.3e38, 1e10, -1e10, 2.0 ** 31, -2.0 ** 31, 40000.0, -32767.5, 32767.0, 32766.99], np.float32), size=int(big.sum()))
    return u, v


@pytest.mark.parametrize("rows,cols", [(5, 7), (1, 9), (6, 1), (1, 1), (19, 24)])
def test_predictor_kernel_equals_the_reference(gpu, rows, cols):
    rng = np.random.default_rng(rows * 100 + cols)
    for scale in (0.3, 3.0, 40.0):
        u, v = hand_field(rng, 4, rows, cols, scale)
        want = ref.predict_nodes(u, v)
        got = piv.predict_deform(u, v)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    nanf = np.full((2, rows, cols), np.nan, np.float32)
    assert not piv.predict_deform(nanf, nanf).any()
    for x in (1 / 128, 3 / 128, -1 / 128, -3 / 128, 5 / 128, 0.5, 1e-9, -0.0):       # half-units alone: to even
        f = np.full((1, rows, cols), x, np.float32)
        assert np.array_equal(piv.predict_deform(f, -f), ref.predict_nodes(f, -f)), x


# ---- 2. one pass against the reference, on the same nodes ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=["u8", "f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_pass_matches_the_reference_host_and_device_entry(gpu, case, dtype):
    n, ov, _ = geometry(case)
    a, nodes, r = ref.pass_stack(case, dtype), ref.hand_nodes(case), ref.pass_ref(case, dtype)
    *host, planes = piv.piv_pairs_deformed(a, (n, n), (ov, ov), nodes, return_planes=True)
    gate(host, r, planes)
    *dev, dplanes = piv.piv_pairs_deformed(DeviceFrames.from_host(a), (n, n), (ov, ov), nodes, return_planes=True)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(dev + [dplanes], host + [planes], "host and device entry points differ")
    else:
        gate(dev, r, dplanes)
    same_bits(piv.piv_pairs_deformed(a, (n, n), (ov, ov), nodes), host, "without planes")


@pytest.mark.parametrize("case", CASES)
def test_signal_threshold_scores_the_warped_window(gpu, case):
    n, ov, _ = geometry(case)
    r = ref.signal_ref(case)
    for dtype in ref.PASS_DTYPES:       # (the float stacks hold the same sample values: an affine map would move the zeros)
        got = piv.piv_pairs_deformed(DeviceFrames.from_host(ref.signal_stack(case).astype(dtype)), (n, n), (ov, ov), ref.hand_nodes(case),
                                     ref.SIGNAL_THR, return_planes=True)
        gate(got[:4], r, got[4])


# ---- 3. grids: one row of nodes, and 75 % overlap (a window spans more than one node interval) -----------------------------------------
@pytest.mark.parametrize("case", list(ref.GRID_CASES))
def test_grid_cases(gpu, case):
    n, ov, _ = geometry(case)
    got = piv.piv_pairs_deformed(ref.pass_stack(case), (n, n), (ov, ov), ref.hand_nodes(case), return_planes=True)
    gate(got[:4], ref.pass_ref(case), got[4])


# ---- 4. zero nodes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.PASS_DTYPES, ids=["u8", "f32", "f64"])
@pytest.mark.parametrize("case", CASES)
def test_zero_nodes_are_the_plain_pass(gpu, case, dtype):
    """The warped frame IS frame t+1 (for uint8 exactly so by construction, for floats because one weight is 4096 and three are 0).  On
    float32 stacks the mixed-type kernel keeps the shifted kernel's arithmetic order: the bits of piv_pairs_shifted at zero offsets.
    On uint8 stacks window B takes the float statistics instead of the shifted kernel's exact integer ones, on float64 stacks in HBM B
    is the narrowed sample: there the gate is asserted, against the reference and against the shifted kernel."""
    n, ov, dim = geometry(case)
    a = ref.pass_stack(case, dtype)
    d = DeviceFrames.from_host(a)
    rows, cols = window.get_array_shape(dim, (n, n), (ov, ov))
    none = piv.piv_pairs_deformed(d, (n, n), (ov, ov), None, return_planes=True)
    same_bits(piv.piv_pairs_deformed(d, (n, n), (ov, ov), np.zeros((ref.PASS_T - 1, rows, cols, 2), np.int32), return_planes=True), none)
    r = ref.pass_ref(case, dtype, nodes=None)
    gate(none[:4], r, none[4])
    shifted = piv.piv_pairs_shifted(d, (n, n), (ov, ov), None, return_planes=True)
    if dtype == np.float32:
        same_bits(none, shifted, "zero nodes against the shifted kernel at zero offsets")
    else:
        gate(none[:4], dict(r, **dict(zip(("u", "v", "corr", "s2n"), (x.astype(np.float64) for x in shifted[:4])), planes=shifted[4].astype(np.float64))), none[4])


# ---- 5. a node reaches the windows whose pixels interpolate from it, and no others -----------------------------------------------------
@pytest.mark.parametrize("case", CASES + ["75%"])
def test_a_node_reaches_its_neighbourhood_alone(gpu, case):
    n, ov, dim = geometry(case)
    s = n - ov
    d = DeviceFrames.from_host(ref.pass_stack(case))
    nodes = ref.hand_nodes(case)
    base = piv.piv_pairs_deformed(d, (n, n), (ov, ov), nodes, 0.02, return_planes=True)
    P, rows, cols = nodes.shape[:3]
    y0, x0 = mp.grid_origins(dim, n, ov)
    for (p, r, c) in ((0, 0, 0), (1, rows // 2, cols // 2), (2, rows - 1, cols - 1)):
        nd = nodes.copy()
        nd[p, r, c] += (3 * 128 + 5, -2 * 128 - 9)
        got = piv.piv_pairs_deformed(d, (n, n), (ov, ov), nd, 0.02, return_planes=True)
        # node (r, c) sits at pixel y0[r] + n / 2 - 0.5 and enters the field strictly less than one node interval around it; a window
        # covers its origin .. origin + n - 1.  Farther than one interval plus half a window: untouched, bit for bit
        cy, cx = y0[r] + n / 2 - 0.5, x0[c] + n / 2 - 0.5
        far = np.ones(base[0].shape, bool)
        far[p] = (np.abs(y0 + n / 2 - 0.5 - cy)[:, None] >= s + n / 2) | (np.abs(x0 + n / 2 - 0.5 - cx)[None, :] >= s + n / 2)
        assert not far[p, r, c]
        for g, b in zip(got[:4], base[:4]):
            assert np.array_equal(g[far], b[far], equal_nan=True), (p, r, c)
        assert np.array_equal(got[4].reshape(-1, n, n)[far.reshape(-1)], base[4].reshape(-1, n, n)[far.reshape(-1)], equal_nan=True)
        assert not np.array_equal(got[4][p, r * cols + c], base[4][p, r * cols + c])
    # the pairs in two calls
    first = piv.piv_pairs_deformed(d[0:2], (n, n), (ov, ov), nodes[:1], 0.02, return_planes=True, pair_offset=0)
    rest = piv.piv_pairs_deformed(d[1:ref.PASS_T], (n, n), (ov, ov), nodes[1:], 0.02, return_planes=True, pair_offset=1)
    same_bits([np.concatenate([f, q]) for f, q in zip(first, rest)], base, "two calls")


# ---- 6. the chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,D", [([(64, 32), (32, 16)], 1), ([(64, 32), (32, 16)], 2), ([(32, 16)], 1), ([(64, 32), (32, 16), (16, 8)], 1)],
                         ids=["64-32+1", "64-32+2", "32+1", "64-32-16+1"])
def test_chain_is_its_passes(gpu, chain, D):
    a = ref.accuracy_stack(5)
    n, ov = chain[-1]
    u, v, cm, sn, planes, shift, per = piv.piv_multipass(a, chain, return_planes=True, return_shift=True, return_passes=True, deform_passes=D)
    assert len(per) == len(chain) + D
    for k in range(len(chain), len(chain) + D):
        want = ref.predict_nodes(per[k - 1][0], per[k - 1][1])                 # on the GPU's own previous pass: exact
        assert np.array_equal(per[k][4], want), k
        r = ref.deformed_piv(a, n, ov, per[k][4])
        gate(per[k][:4], r, planes if k == len(per) - 1 else None)
    # the one call is the composition; the host entry and the DeviceFrames entry give the same bits; the offsets are the chain's
    same_bits((u, v, cm, sn), per[-1][:4], "one call against the passes")
    if len(chain) > 1:
        assert np.array_equal(shift, per[len(chain) - 1][4])
    else:
        assert not shift.any()
    same_bits(piv.piv_multipass(DeviceFrames.from_host(a), chain, return_planes=True, return_shift=True, deform_passes=D), (u, v, cm, sn, planes, shift))
    same_bits(piv.piv_multipass(a, chain, return_planes=True, return_shift=True, deform_passes=D), (u, v, cm, sn, planes, shift), "host entry")
    same_bits(piv.piv_multipass(a, window.multipass_spec((n, n), (ov, ov), chain[:-1], D)), (u, v, cm, sn), "a MultiPassWindow carries the count")
    # none and zero are today's call
    today = piv.piv_multipass(a, chain, return_planes=True, return_shift=True)
    for d0 in (None, 0):
        same_bits(piv.piv_multipass(a, chain, return_planes=True, return_shift=True, deform_passes=d0), today, "deform_passes = 0")


# ---- 7. get_ffpiv: chunks, devices, device and lazy stacks ------------------------------------------------------------------------------
def test_get_ffpiv_chunks_devices_device_stack_and_lazy_stack(gpu):
    """51 pairs on a 70 x 101 frame: pass 0's anchors (64 px: 25 pairs) fall at pairs 25 and 50, so chunksize and devices= really cut."""
    a = long_stack()
    P = len(a) - 1
    x, y = window.get_rect_coordinates(a.shape[1:], (16, 16), (8, 8))
    run = lambda f, **kw: velocimetry.get_ffpiv(f, y, x, np.full(P, 0.5), (16, 16), (8, 8), (16, 16), 0.02, 0.02, **kw)
    d = DeviceFrames.from_host(a)
    direct = piv.piv_multipass(d, [(64, 32), (16, 8)], deform_passes=1)
    whole = run(a, coarse_passes=[(64, 32)], deform_passes=1)
    assert np.array_equal(np.asarray(whole["corr"]), direct[2], equal_nan=True)
    for f, kw, chunks, workers in ((a, dict(chunksize=2), 3, 1), (a, dict(devices=[0, 0]), 2, 2), (a, dict(chunksize=3, devices=[0, 0]), 3, 2),
                                   (d, dict(chunksize=4), 3, 1), (_Lazy(a), dict(chunksize=3), 3, 1), (_Lazy(a), dict(), 1, 1)):
        got = run(f, coarse_passes=[(64, 32)], deform_passes=1, **kw)
        st = dict(executor.LAST_STATS)
        assert st["chunks"] >= chunks and len(st["per_device"]) == workers, (type(f).__name__, kw, st)
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (type(f).__name__, kw, k)
    # the chain itself in three calls on the anchors
    parts = [piv.piv_multipass(d[p0:p1 + 1], [(64, 32), (16, 8)], deform_passes=1, pair_offset=p0) for p0, p1 in ((0, 25), (25, 50), (50, P))]
    same_bits([np.concatenate(q) for q in zip(*parts)], direct, "three calls")
    # without coarse passes, through frames.get_piv; 0 and None are today's results
    alone = piv.piv_multipass(a[:9], [(16, 8)], deform_passes=2)
    ds = frames.get_piv(a[:9], 16, deform_passes=2)
    same_bits([np.asarray(ds[k]) for k in KEYS], alone, "frames.get_piv")
    same_bits([np.asarray(frames.get_piv(a[:9], 16, deform_passes=2, chunksize=3)[k]) for k in KEYS], alone, "chunked")
    plain = frames.get_piv(a[:9], 16)
    same_bits([np.asarray(frames.get_piv(a[:9], 16, deform_passes=dp)[k]) for dp in (None, 0) for k in KEYS], [np.asarray(plain[k]) for k in KEYS] * 2)
    chained = frames.get_piv(a[:9], 16, coarse_passes=[(64, 32)])
    same_bits([np.asarray(frames.get_piv(a[:9], 16, coarse_passes=[(64, 32)], deform_passes=0)[k]) for k in KEYS], [np.asarray(chained[k]) for k in KEYS])


def test_wrapped_accessor_takes_the_keyword(gpu, monkeypatch):
    """``Frames.get_piv(engine="hip", coarse_passes=[64], deform_passes=1)`` -- what a recipe's ``get_piv:`` section calls."""
    from pyorc_amd import plugin
    from tests import recipe_doubles as rd

    a = long_stack()[:9]
    direct = piv.piv_multipass(a, [(64, 32), (16, 8)], deform_passes=1)
    alone = piv.piv_multipass(a, [(16, 8)], deform_passes=1)
    plain = frames.get_piv(a, 16)
    rd.install(monkeypatch.setitem)
    try:
        via = rd.Frames(a).get_piv(16, engine="hip", coarse_passes=[64], deform_passes=1)
        same_bits([np.asarray(via[k]) for k in KEYS], direct, "wrapped accessor, chain")
        via = rd.Frames(a).get_piv(16, engine="hip", deform_passes=1)
        same_bits([np.asarray(via[k]) for k in KEYS], alone, "wrapped accessor, no coarse passes")
        with pytest.raises(ValueError, match="deform_passes must be a whole number"):
            rd.Frames(a).get_piv(16, engine="hip", deform_passes=7)
    finally:
        plugin.uninstall()
    assert not np.array_equal(alone[0], np.asarray(plain["v_x"]), equal_nan=True)


def test_v_sign_is_applied_once_at_the_end(gpu):
    a = ref.accuracy_stack(5)
    off = piv.piv_multipass(a, ref.ACCURACY_CHAIN, deform_passes=2)
    _lib.set_option("v_sign", 1)
    try:
        on = piv.piv_multipass(a, ref.ACCURACY_CHAIN, deform_passes=2, return_passes=True)
        one = piv.piv_pairs_deformed(a, (32, 32), (16, 16), on[4][-1][4])
    finally:
        _lib.set_option("v_sign", 0)
    same_bits((on[0], -on[1], on[2], on[3]), off, "v_sign")
    same_bits((one[0], -one[1]), (on[4][-1][0], on[4][-1][1]), "the pass entry point negates v")


# ---- 8. the value of the feature, on the device -------------------------------------------------------------------------------------------
def test_one_deformation_pass_halves_the_error_on_the_device(gpu):
    a = ref.accuracy_stack(5)
    u0, v0, _, _ = piv.piv_multipass(a, ref.ACCURACY_CHAIN)
    u1, v1, _, _ = piv.piv_multipass(a, ref.ACCURACY_CHAIN, deform_passes=1)
    m0, s0 = ref.accuracy_figures(u0, v0)
    m1, s1 = ref.accuracy_figures(u1, v1)
    print(f"integer chain median {m0:.4f} px, share {s0:.3f}; + one deformation pass {m1:.4f} px, share {s1:.3f}; ratio {m1 / m0:.3f}")
    assert m1 <= 0.65 * m0


# ---- 9. the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    a = ref.pass_stack(16)
    n, ov, (H, W) = ref.PASS_CASES[16]
    for opt, val, back in (("norm_clip", 0, 1), ("signal_mode", 1, 0)):
        _lib.set_option(opt, val)
        try:
            for call in (lambda: piv.piv_pairs_deformed(a, (16, 16), (8, 8)), lambda: piv.piv_multipass(a, [(16, 8)], 0.05, deform_passes=1),
                         lambda: piv.piv_multipass(DeviceFrames.from_host(a), [(32, 16), (16, 8)], 0.05, deform_passes=1),
                         lambda: frames.get_piv(a, 16, deform_passes=1, signal_threshold=0.05)):
                with pytest.raises(ValueError, match=opt) as e:
                    call()
                assert e.value.code == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, back)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        piv.piv_pairs_deformed(a, (24, 24), (12, 12))
    with pytest.raises(ValueError, match="nodes must have shape"):
        piv.piv_pairs_deformed(a, (16, 16), (8, 8), np.zeros((3, 2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="one shape"):
        piv.predict_deform(np.zeros((2, 3, 3)), np.zeros((2, 3, 4)))
    lib = _lib.load()
    d = DeviceFrames.from_host(a)
    rows, cols = window.get_array_shape((H, W), (n, n), (ov, ov))
    out = DeviceFrames.empty((4, 3, rows * cols), np.float32)
    nodes = DeviceFrames.empty((1, 1, 3 * rows * cols * 8), np.uint8)
    E = _lib
    assert lib.lspiv_piv_deform_pairs_dev_at(None, 0, 4, H, W, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, W, 16, 16, 8, 8, -1.0, 0, None, out.c_ptr, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, W, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, None, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, W, 16, 16, 8, 8, -1.0, -1, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 1, H, W, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_ESHAPE
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, 12, W, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_ESHAPE
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, W, 24, 24, 12, 12, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EUNSUPPORTED
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, W, 16, 16, 8, 4, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EUNSUPPORTED
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, 4, H, 40000, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 3, 4, H, W, 16, 16, 8, 8, -1.0, 0, nodes.c_ptr, out.c_ptr, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_predict_deform_dev(None, out.c_ptr, 1, 2, 2, nodes.c_ptr, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_predict_deform_dev(out.c_ptr, out.c_ptr, 1, 2, 2, None, None) == E.LSPIV_EINVAL
    assert lib.lspiv_piv_predict_deform_dev(out.c_ptr, out.c_ptr, 1, 0, 2, nodes.c_ptr, None) == E.LSPIV_ESHAPE
    arr = np.array([16, 16, 8, 8], dtype=np.int32)
    for nd, code in ((-1, E.LSPIV_EINVAL), (5, E.LSPIV_EINVAL)):
        assert lib.lspiv_piv_multipass_deform_dev_at(d.c_ptr, 0, 4, H, W, 1, _lib.ptr(arr), nd, -1.0, 0, out.c_ptr, None, None, None) == code
    arr24 = np.array([24, 24, 12, 12], dtype=np.int32)
    assert lib.lspiv_piv_multipass_deform_dev_at(d.c_ptr, 0, 4, H, W, 1, _lib.ptr(arr24), 1, -1.0, 0, out.c_ptr, None, None, None) == E.LSPIV_EUNSUPPORTED
    assert lib.lspiv_deform_required_bytes(1, H, W, 16, 16, 8, 8) == E.LSPIV_ESHAPE
