"""Multi-pass PIV on the GPU against tests/multipass_ref.py, the float64 reference.  Gate, the search-area
tests' own: NaN masks identical, u, v, corr, s2n within 1e-4 (of max(|ref|, 0.05)), planes within 2e-6.  Only windows whose reference
plane has an exact float64 tie for its maximum are set aside, at most 1 % of a case; the predictor is compared as integers.  Inputs,
tie shares and the coarse vectors next to a half-integer are checked on the CPU (tests/test_multipass_host.py)."""
import functools

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, executor, frames, piv, velocimetry, window
from pyorc_amd.device import DeviceFrames
from tests import multipass_ref as ref
from tests.test_gpu_search_area import gate
from tests.test_multipass_host import (CHAIN_STACKS, CHAINS, FFPIV_PASSES, SHIFT_CASES, SIGNAL_CASES, SIGNAL_THRESHOLD, WILD_CASES, chain_ref,
                                       chain_stack, ffpiv_stack, long_stack, shift_offsets, shift_stack, signal_stack, wild_offsets)

pytestmark = pytest.mark.gpu
IDS = [f"{c[0]}@{c[2]}" for c in SHIFT_CASES]


def same_bits(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w, equal_nan=True), (what, k)


@functools.lru_cache(maxsize=None)
def shift_ref(i):   # one reference per case, shared by the tests on uint8 samples
    n, _, ov, _ = SHIFT_CASES[i]
    return ref.shifted_piv(shift_stack(i), n, ov, shift_offsets(i))


# ---- 1. the shifted kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("i", range(len(SHIFT_CASES)), ids=IDS)
def test_shifted_kernel_host_and_device_entry(gpu, i, dtype):
    n, _, ov, _ = SHIFT_CASES[i]
    a, sh = shift_stack(i, dtype), shift_offsets(i)
    r = shift_ref(i) if dtype == np.uint8 else ref.shifted_piv(a.astype(np.float64), n, ov, sh)
    *host, planes = piv.piv_pairs_shifted(a, (n, n), (ov, ov), sh, return_planes=True)
    gate(host, r, planes)
    *dev, dplanes = piv.piv_pairs_shifted(DeviceFrames.from_host(a), (n, n), (ov, ov), sh, return_planes=True)
    if dtype != np.float64:   # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(dev + [dplanes], host + [planes], "host and device entry points differ")
    else:
        gate(dev, r, dplanes)


@pytest.mark.parametrize("i", WILD_CASES, ids=[IDS[i] for i in WILD_CASES])
def test_offsets_outside_the_frame_are_clamped(gpu, i):
    n, (H, W), ov, seed = SHIFT_CASES[i]
    a, wild = shift_stack(i), wild_offsets(i)
    clamped = ref.clamp_shift(wild, (H, W), n, ov).astype(np.int16)
    r = ref.shifted_piv(a, n, ov, wild)
    assert np.array_equal(r["shift"], clamped)
    got = piv.piv_pairs_shifted(a, (n, n), (ov, ov), wild, return_planes=True)
    gate(got[:4], r, got[4])
    same_bits(got, piv.piv_pairs_shifted(a, (n, n), (ov, ov), clamped, return_planes=True), "the clamped offset is not the one used")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("i", SIGNAL_CASES, ids=[IDS[i] for i in SIGNAL_CASES])
def test_signal_threshold_scores_the_shifted_window(gpu, i, dtype):
    n, _, ov, _ = SHIFT_CASES[i]
    a, sh = signal_stack(i), shift_offsets(i)
    r = ref.shifted_piv(a, n, ov, sh, signal_threshold=SIGNAL_THRESHOLD)
    # (the affine map of the float types would move the zeros: the float stacks hold the same sample values)
    got = piv.piv_pairs_shifted(DeviceFrames.from_host(a.astype(dtype)), (n, n), (ov, ov), sh, SIGNAL_THRESHOLD, return_planes=True)
    gate(got[:4], r, got[4])


def test_a_nan_sample_takes_out_its_own_window_only(gpu):
    i = 1                                                    # 16 @ 0 on 48 x 53: windows do not overlap
    n, _, ov, _ = SHIFT_CASES[i]
    a, sh = shift_stack(i, np.float32), shift_offsets(i)
    clean = piv.piv_pairs_shifted(a, (n, n), (ov, ov), sh, return_planes=True)
    b = a.copy()
    b[0, 20, 21] = np.nan                                    # frame 0 is the window of frame t of pair 0 only: window (1, 1)
    got = piv.piv_pairs_shifted(b, (n, n), (ov, ov), sh, return_planes=True)
    hit = np.zeros(clean[0].shape, bool)
    hit[0, 1, 1] = True
    for g, c in zip(got[:4], clean[:4]):
        assert np.isnan(g[hit]).all() and np.array_equal(g[~hit], c[~hit], equal_nan=True)
    assert np.isnan(got[4][0, 1 * 3 + 1]).all() and np.array_equal(np.delete(got[4].reshape(-1, n, n), 4, 0), np.delete(clean[4].reshape(-1, n, n), 4, 0),
                                                                  equal_nan=True)
    # ... and in frame 1 (the shifted window of pair 0, the window of frame t of pair 1) exactly the windows that read the sample
    y0, x0 = ref.grid_origins(a.shape[1:], n, ov)
    by, bx = y0[:, None] + sh[0, :, :, 0], x0[None, :] + sh[0, :, :, 1]
    py, px = int(by[1, 1]) + 3, int(bx[1, 1]) + 4             # a sample of the shifted window (1, 1) of pair 0
    b = a.copy()
    b[1, py, px] = np.nan
    got = piv.piv_pairs_shifted(b, (n, n), (ov, ov), sh)
    reads = np.zeros(clean[0].shape, bool)
    reads[0] = (by <= py) & (py < by + n) & (bx <= px) & (px < bx + n)
    reads[1] = ((y0 <= py) & (py < y0 + n))[:, None] & ((x0 <= px) & (px < x0 + n))[None, :]
    assert reads[0, 1, 1] and 1 <= reads[0].sum() <= 4 and reads[1].sum() <= 1 and not reads[2].any()
    for g, c in zip(got, clean[:4]):
        assert np.isnan(g[reads]).all() and np.array_equal(g[~reads], c[~reads], equal_nan=True)


# ---- 2. / 3. zero offsets, independence of the windows, pair_offset -----------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHIFT_CASES)), ids=IDS)
def test_zero_offsets_are_no_offsets_and_the_plain_pass(gpu, i):
    n, (H, W), ov, _ = SHIFT_CASES[i]
    a = shift_stack(i)
    rows, cols = window.get_array_shape((H, W), (n, n), (ov, ov))
    none = piv.piv_pairs_shifted(a, (n, n), (ov, ov), None, return_planes=True)
    same_bits(piv.piv_pairs_shifted(a, (n, n), (ov, ov), np.zeros((3, rows, cols, 2), np.int16), return_planes=True), none)
    _, _, oracle = po.cross_corr(a, (n, n), (ov, ov))
    r = ref.shifted_piv(a, n, ov)
    assert np.array_equal(r["planes"], oracle)
    gate(none[:4], r, none[4])


@pytest.mark.parametrize("i", [0, 2, 4], ids=[IDS[0], IDS[2], IDS[4]])
def test_a_window_depends_on_its_own_offset_alone(gpu, i):
    n, _, ov, _ = SHIFT_CASES[i]
    a, sh = shift_stack(i), shift_offsets(i)
    d = DeviceFrames.from_host(a)
    base = piv.piv_pairs_shifted(d, (n, n), (ov, ov), sh, 0.02, return_planes=True)
    rows, cols = sh.shape[1:3]
    for (p, r, c) in ((0, 0, 0), (1, rows // 2, cols // 2), (2, rows - 1, cols - 1), (1, 0, 1)):
        sh2 = sh.copy()
        sh2[p, r, c] = -sh[p, r, c] + (1, 1)
        got = piv.piv_pairs_shifted(d, (n, n), (ov, ov), sh2, 0.02, return_planes=True)
        keep = np.ones(base[0].shape, bool)
        keep[p, r, c] = False
        for g, b in zip(got[:4], base[:4]):
            assert np.array_equal(g[keep], b[keep], equal_nan=True), (p, r, c)
        assert np.array_equal(got[4].reshape(-1, n, n)[keep.reshape(-1)], base[4].reshape(-1, n, n)[keep.reshape(-1)], equal_nan=True)
        if not np.array_equal(ref.clamp_shift(sh2, a.shape[1:], n, ov)[p, r, c], sh[p, r, c]):     # (the frame clamp may undo the change)
            assert not np.array_equal(got[4][p, r * cols + c], base[4][p, r * cols + c])
    # the pairs in two calls
    first = piv.piv_pairs_shifted(d[0:2], (n, n), (ov, ov), sh[:1], 0.02, return_planes=True, pair_offset=0)
    rest = piv.piv_pairs_shifted(d[1:4], (n, n), (ov, ov), sh[1:], 0.02, return_planes=True, pair_offset=1)
    same_bits([np.concatenate([f, s]) for f, s in zip(first, rest)], base, "two calls")


# ---- 4. the predictor ---------------------------------------------------------------------------------------------------------------
def random_field(rng, P, rows, cols, scale):
    u = (rng.standard_normal((P, rows, cols)) * scale).astype(np.float32)
    v = (rng.standard_normal((P, rows, cols)) * scale).astype(np.float32)
    half = rng.random((P, rows, cols)) < 0.2                       # exact +-k.5 values
    u[half] = np.rint(u[half]) + np.float32(0.5)
    v[~half & (rng.random((P, rows, cols)) < 0.2)] -= np.float32(0.5)
    for _ in range(3):                                             # NaN patches, in one component or both
        p, r, c = rng.integers(P), rng.integers(rows), rng.integers(cols)
        (u if rng.random() < 0.5 else v)[p, r:r + 3, c:c + 2] = np.nan
    u[rng.random((P, rows, cols)) < 0.05] = np.inf
    big = rng.random((P, rows, cols)) < 0.1                        # finite values far outside the int16 range, up to the largest float32
    v[big] = rng.choice(np.array([3.3e38, -3.3e38, 1e10, -1e10, 2.0 ** 31, -2.0 ** 31, 40000.0, -32768.5, 32767.5], np.float32), size=int(big.sum()))
    return u, v


@pytest.mark.parametrize("coarse,fine", [((64, 32), (32, 16)), ((64, 0), (16, 8)), ((32, 16), (32, 16)), ((20, 10), (16, 8))])
def test_predictor_kernel_equals_the_reference(gpu, coarse, fine):
    dim = (130, 197)
    rows, cols = window.get_array_shape(dim, (coarse[0],) * 2, (coarse[1],) * 2)
    rng = np.random.default_rng(coarse[0] * 100 + fine[0])
    for scale in (3.0, 40.0):
        u, v = random_field(rng, 5, rows, cols, scale)
        want = ref.predict_shift(u, v, dim, coarse, fine)
        got = piv.predict_shift(u, v, dim, coarse, fine)
        assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)
    nanf = np.full((2, rows, cols), np.nan, np.float32)
    assert not piv.predict_shift(nanf, nanf, dim, coarse, fine).any()


HUGE_ROW = np.zeros((1, 1, 62))
HUGE_ROW[0, 0, 0] = 1e10      # (tests/test_multipass_host.py: 16384 at the first fine window)


def test_predictor_kernel_on_the_hand_worked_grids(gpu):
    nan = np.nan
    grids = [([[[3.4]]], [[[-2.6]]], (64, 64), (64, 32), (16, 8)),
             ([[[2.0, 4.0, 12.0]]], [[[0.0, 0.0, 0.0]]], (32, 64), (32, 16), (16, 0)),
             ([[[0.0], [0.0], [0.0]]], [[[2.0], [4.0], [12.0]]], (64, 32), (32, 16), (16, 0)),
             (np.full((1, 3, 3), nan), np.zeros((1, 3, 3)), (64, 64), (32, 16), (32, 16)),
             (np.full((1, 3, 3), 5.0), np.full((1, 3, 3), nan), (64, 64), (32, 16), (32, 16)),
             ([[[1.0, 2.0, 50.0], [4.0, 9.0, 50.0], [50.0, 50.0, 50.0]]], np.zeros((1, 3, 3)), (96, 96), (32, 0), (32, 0)),
             ([[[1.0, nan, 50.0], [4.0, 9.0, 50.0], [50.0, 50.0, 50.0]]], np.zeros((1, 3, 3)), (96, 96), (32, 0), (32, 0)),
             ([[[1.0, 2.0]]], [[[0.0, 0.0]]], (32, 64), (32, 0), (32, 0)),
             ([[[-2.0, -1.0]]], [[[0.0, 0.0]]], (32, 64), (32, 0), (32, 0)),
             (np.full((1, 2, 3), 20.0), np.full((1, 2, 3), 20.0), (130, 197), (64, 0), (16, 8)),
             (np.full((1, 2, 3), -20.0), np.full((1, 2, 3), -20.0), (130, 197), (64, 0), (16, 8)),
             ([[[0.0, 8.0, 16.0]] * 2], np.zeros((1, 2, 3)), (130, 197), (64, 0), (16, 8))]
    grids += [([[[1e10]]], [[[-3.3e38]]], (96, 96), (96, 0), (32, 0)), ([[[np.inf]]], [[[0.0]]], (96, 96), (96, 0), (32, 0)),
              (HUGE_ROW, np.zeros_like(HUGE_ROW), (512, 32000), (512, 0), (16, 0)),
              (np.zeros((1, 62, 1)), HUGE_ROW.reshape(1, 62, 1), (32000, 512), (512, 0), (16, 0))]
    grids += [([[[x]]], [[[-x]]], (96, 96), (96, 0), (32, 0)) for x in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5)]
    for u, v, dim, coarse, fine in grids:
        assert np.array_equal(piv.predict_shift(u, v, dim, coarse, fine), ref.predict_shift(u, v, dim, coarse, fine)), (u, dim, coarse, fine)


# ---- 5. the chain, composed without loss ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(len(CHAINS)), ids=["64-32-16", "32-32"])
@pytest.mark.parametrize("name", CHAIN_STACKS)
def test_chain_is_its_passes(gpu, name, c):
    a, chain = chain_stack(name), CHAINS[c]
    dim = a.shape[1:]
    u, v, cm, sn, planes, shift, per = piv.piv_multipass(a, chain, return_planes=True, return_shift=True, return_passes=True)
    assert len(per) == len(chain) and per[0][4] is None
    n0, o0 = chain[0]
    # (return_passes composes the chain call by call, so this line compares piv_pairs with piv_pairs.  That pass 0 INSIDE the one call is
    # piv_pairs too rests on its being the same fill_params + dispatch on the same frames, grid and pair_offset (api_piv.hip, multipass_dev);
    # what the tests see of it is the one call's final offsets and results equal to the composition's, below, and the one-pass chain.)
    same_bits(per[0][:4], piv.piv_pairs(a, (n0, n0), (o0, o0)), "pass 0 is piv_pairs")
    for k in range(1, len(chain)):
        n, ov = chain[k]
        want = ref.predict_shift(per[k - 1][0], per[k - 1][1], dim, chain[k - 1], chain[k])      # on the GPU's own previous pass: exact
        assert np.array_equal(per[k][4], want), k
        r = ref.shifted_piv(a, n, ov, per[k][4])
        gate(per[k][:4], r, planes if k == len(chain) - 1 else None)
    # the one call is the composition; the host entry and the DeviceFrames entry give the same bits
    same_bits((u, v, cm, sn, shift), per[-1], "one call against the passes")
    same_bits(piv.piv_multipass(DeviceFrames.from_host(a), chain, return_planes=True, return_shift=True), (u, v, cm, sn, planes, shift))
    same_bits(piv.piv_multipass(a, chain, return_planes=True, return_shift=True), (u, v, cm, sn, planes, shift), "host entry")
    # against the reference's own chain: at most 1 % of the windows with another offset, the rest within the gate
    rr = chain_ref(name, c)[-1]
    differ = np.any(shift != rr["shift"], axis=-1)
    print("windows with another offset than the reference's chain:", int(differ.sum()), "of", differ.size)
    assert differ.mean() <= 0.01
    drop = lambda x: np.where(differ, np.nan, x)                   # the windows with another offset are set aside in every variable
    gate(tuple(drop(x).astype(np.float32) for x in (u, v, cm, sn)), dict(rr, **{k: drop(rr[k]) for k in ("u", "v", "corr", "s2n")}))
    assert np.nanmax(np.abs(planes.reshape(differ.shape + planes.shape[-2:])[~differ] - rr["planes"].reshape(differ.shape + planes.shape[-2:])[~differ]),
                     initial=0.0) < 2e-6


def test_one_pass_chain_is_todays_call(gpu):
    a = chain_stack("particles")
    u, v, cm, sn, shift = piv.piv_multipass(a, [(32, 16)], 0.02, return_shift=True)
    same_bits((u, v, cm, sn), piv.piv_pairs(a, (32, 32), (16, 16), 0.02))
    assert not shift.any()


# ---- 6. get_ffpiv / frames.get_piv ------------------------------------------------------------------------------------------------------
class _Lazy:
    """The least a lazy stack offers: ``load()`` and time slicing."""

    def __init__(self, data):
        self._d, self.dtype, self.shape = data, data.dtype, data.shape

    def __len__(self):
        return len(self._d)

    def __getitem__(self, key):
        return _Lazy(self._d[key]) if isinstance(key, slice) else self._d[key]

    def load(self):
        return np.array(self._d)


KEYS = ("v_x", "v_y", "corr", "s2n")


def test_get_ffpiv_chunks_devices_device_stack_and_lazy_stack(gpu):
    a = ffpiv_stack()
    x, y = window.get_rect_coordinates(a.shape[1:], (16, 16), (8, 8))
    run = lambda f, **kw: velocimetry.get_ffpiv(f, y, x, np.full(8, 0.5), (16, 16), (8, 8), (16, 16), 0.02, 0.02, coarse_passes=[(64, 32)], **kw)
    whole = run(a)
    r = ref.multipass(a, FFPIV_PASSES)[-1]
    # back to pixels (dt / res = 25; the float32 storage of m/s and of this product add 6e-8 relative each, far inside the gate)
    gate((np.asarray(whole["v_x"]) * 25.0, np.asarray(whole["v_y"]) * 25.0, np.asarray(whole["corr"]), np.asarray(whole["s2n"])), r)
    direct = piv.piv_multipass(a, FFPIV_PASSES)
    assert np.array_equal(np.asarray(whole["corr"]), direct[2], equal_nan=True)
    for f, kw in ((a, dict(chunksize=2)), (a, dict(chunksize=3)), (a, dict(devices=[0, 0])), (a, dict(chunksize=3, devices=[0, 0])),
                  (DeviceFrames.from_host(a), dict(chunksize=4)), (_Lazy(a), dict()), (_Lazy(a), dict(chunksize=3))):
        got = run(f, **kw)
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (type(f).__name__, kw, k)
    ds = frames.get_piv(a, 16, coarse_passes=[(64, 32)])
    same_bits([np.asarray(ds[k]) for k in KEYS], [direct[0], direct[1], direct[2], direct[3]], "frames.get_piv")
    plain = frames.get_piv(a, 16)
    same_bits([np.asarray(frames.get_piv(a, 16, coarse_passes=cp)[k]) for cp in (None, []) for k in KEYS], [np.asarray(plain[k]) for k in KEYS] * 2)


def test_chain_over_several_chunks_and_workers(gpu):
    """51 pairs: pass 0's anchors (25 pairs on this grid) fall at pairs 25 and 50, so chunksize and devices= really cut the stack --
    asserted on the run's statistics -- and the chain runs at pair offsets 25 and 50."""
    a = long_stack()
    P = len(a) - 1
    assert window.chunk_alignment(window.multipass_spec((16, 16), (8, 8), [(64, 32)]), a.shape[1:], (8, 8)) == 25
    x, y = window.get_rect_coordinates(a.shape[1:], (16, 16), (8, 8))
    run = lambda f, **kw: velocimetry.get_ffpiv(f, y, x, np.full(P, 0.5), (16, 16), (8, 8), (16, 16), 0.02, 0.02, coarse_passes=[(64, 32)], **kw)
    d = DeviceFrames.from_host(a)
    direct = piv.piv_multipass(d, FFPIV_PASSES, return_shift=True)
    whole = run(a)
    assert np.array_equal(np.asarray(whole["corr"]), direct[2], equal_nan=True)
    for f, kw, chunks, workers in ((a, dict(chunksize=2), 3, 1), (a, dict(chunksize=30), 3, 1), (a, dict(devices=[0, 0]), 2, 2),
                                   (a, dict(chunksize=3, devices=[0, 0]), 3, 2), (d, dict(chunksize=4), 3, 1), (_Lazy(a), dict(chunksize=3), 3, 1)):
        got = run(f, **kw)
        st = dict(executor.LAST_STATS)
        assert st["chunks"] >= chunks and st["idle_devices"] == 0 and len(st["per_device"]) == workers, (type(f).__name__, kw, st)
        assert all(w.get("chunks", 0) >= 1 for w in st["per_device"]), st
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(whole[k]), equal_nan=True), (type(f).__name__, kw, k)
    # the chain itself on the anchors, through the DeviceFrames entry and the host entry: two and three calls against the one call
    for src in (d, a):
        for cuts in ((0, 25, P), (0, 25, 50, P)):
            parts = [piv.piv_multipass(src[p0:p1 + 1], FFPIV_PASSES, return_shift=True, pair_offset=p0) for p0, p1 in zip(cuts, cuts[1:])]
            same_bits([np.concatenate(x) for x in zip(*parts)], direct, f"split at {cuts}")
    # ... with the signal threshold and the planes, three passes
    chain = [(64, 32), (32, 16), (16, 8)]
    one = piv.piv_multipass(d, chain, 0.02, return_planes=True, return_shift=True)
    parts = [piv.piv_multipass(d[p0:p1 + 1], chain, 0.02, return_planes=True, return_shift=True, pair_offset=p0) for p0, p1 in ((0, 25), (25, 50), (50, P))]
    same_bits([np.concatenate(x) for x in zip(*parts)], one, "three passes in three calls")


def test_scale_is_numpys_arithmetic(gpu):
    a = ffpiv_stack()
    dt = np.linspace(0.4, 0.6, 8)
    u, v, cm, sn = piv.piv_multipass(a, FFPIV_PASSES)
    for src in (a, DeviceFrames.from_host(a)):
        out = [np.empty_like(u) for _ in range(4)]
        got = piv.piv_multipass(src, FFPIV_PASSES, scale=(0.02, 0.03, dt), out=out)
        assert all(g is o for g, o in zip(got, out))
        vx, vy = np.empty_like(u), np.empty_like(v)
        velocimetry._to_velocity(u, 0.02, dt[:, None, None], out=vx)
        velocimetry._to_velocity(v, 0.03, dt[:, None, None], out=vy)
        same_bits(got, (vx, vy, cm, sn), "scale")
    with pytest.raises(ValueError, match="scale and return_planes"):
        piv.piv_multipass(a, FFPIV_PASSES, scale=(0.02, 0.03, dt), return_planes=True)


@pytest.mark.parametrize("opt,val", [("v_sign", 1), ("border_peak", 1), ("border_peak", 2), ("std_ddof", 1)])
def test_options_follow_the_reference(gpu, opt, val):
    a = ffpiv_stack()
    _lib.set_option(opt, val)
    try:
        with po.semantics(**{opt: val}):
            r = ref.multipass(a, FFPIV_PASSES)[-1]
        ds = frames.get_piv(a, 16, coarse_passes=[(64, 32)])
        gate(tuple(np.asarray(ds[k]) for k in KEYS), r)
        if opt == "v_sign":
            _lib.set_option(opt, 0)
            off = frames.get_piv(a, 16, coarse_passes=[(64, 32)])
            assert np.array_equal(np.asarray(ds["v_y"]), -np.asarray(off["v_y"]), equal_nan=True)
            assert np.array_equal(np.asarray(ds["v_x"]), np.asarray(off["v_x"]), equal_nan=True)
    finally:
        _lib.set_option(opt, 0)


# ---- 7. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    a = ffpiv_stack()
    for opt, val, back in (("norm_clip", 0, 1), ("signal_mode", 1, 0)):
        _lib.set_option(opt, val)
        try:
            for call in (lambda: piv.piv_pairs_shifted(a, (16, 16), (8, 8)), lambda: piv.piv_multipass(a, FFPIV_PASSES, 0.05),
                         lambda: piv.piv_multipass(DeviceFrames.from_host(a), FFPIV_PASSES, 0.05),
                         lambda: frames.get_piv(a, 16, coarse_passes=[64], signal_threshold=0.05)):
                with pytest.raises(ValueError, match=opt) as e:
                    call()
                assert e.value.code == _lib.LSPIV_EUNSUPPORTED
        finally:
            _lib.set_option(opt, back)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        piv.piv_pairs_shifted(a, (24, 24), (12, 12))
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        piv.piv_multipass(a, [(64, 32), (24, 12)])
    with pytest.raises(ValueError, match="shift must have shape"):
        piv.piv_pairs_shifted(a, (16, 16), (8, 8), np.zeros((8, 2, 2, 2), np.int16))
    lib = _lib.load()
    d = DeviceFrames.from_host(a)
    out = DeviceFrames.empty((4, 8, 7 * 11), np.float32)
    arr = (np.array([64, 64, 32, 32, 24, 24, 12, 12], dtype=np.int32))
    assert lib.lspiv_piv_multipass_dev_at(d.c_ptr, 0, 9, 70, 101, 2, _lib.ptr(arr), -1.0, 0, out.c_ptr, None, None, None) == _lib.LSPIV_EUNSUPPORTED
    assert lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, 9, 70, 101, 24, 24, 12, 12, -1.0, 0, None, out.c_ptr, None, None) == _lib.LSPIV_EUNSUPPORTED
    assert lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, 9, 70, 40000, 16, 16, 8, 8, -1.0, 0, None, out.c_ptr, None, None) == _lib.LSPIV_EINVAL
    u = DeviceFrames.empty((2, 1, 16), np.float32)
    assert lib.lspiv_piv_predict_shift_dev(u.c_ptr, u.c_ptr, 1, 64, 40000, 64, 64, 0, 0, 16, 16, 8, 8, out.c_ptr, None) == _lib.LSPIV_EINVAL
    with pytest.raises(NotImplementedError, match="ensemble_corr"):
        frames.get_piv(a, 16, coarse_passes=[64], ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="search_area_size"):
        frames.get_piv(a, 12, search_area_size=32, coarse_passes=[64])
