"""Extended search area on the GPU, the paths tests/test_gpu_search_area.py does not enter: the clip at 1 binding, every window size,
the signal score in every instantiation, non-finite samples, the rescue pass at other sizes and sample types, even and single window
counts, float64 on a large offset.  Reference (tests/search_area_ref.py) and gate are those of test_gpu_search_area.py, unchanged;
each input's property (clip counts, zero ties, signal instances, NaN geometry) is asserted on the CPU in tests/test_search_area_host.py."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames
from tests import search_area_ref as ref
from tests import test_search_area_host as inputs
from tests.test_gpu_search_area import gate

pytestmark = pytest.mark.gpu
DTYPES = (np.uint8, np.float32, np.float64)
DTYPE_IDS = ("uint8", "float32", "float64")


def run(a, n, S, thr=None, planes=True, device=False, ov=None):
    ov = S // 2 if ov is None else ov
    return list(piv.piv_pairs(DeviceFrames.from_host(a) if device else a, (n, n), (ov, ov), thr, search_area_size=(S, S), return_planes=planes))


def assert_bit_equal(got, want, what, where=None):
    for g, w in zip(got, want):
        if where is not None:
            sel = where.reshape(g.shape[:2]) if g.ndim == 4 else where
            g, w = g[sel], w[sel]
        assert np.array_equal(g, w, equal_nan=True), what


@contextlib.contextmanager
def options(**kw):
    """Library options and the oracle's semantics together, reset on the way out."""
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        with po.semantics(**kw):
            yield
    finally:
        for k in kw:
            _lib.set_option(k, 0)


# ---- A. the clip at 1 binds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("i", range(3), ids=[f"{c[0]}in{c[1]}" for c in inputs.CLIP_CASES])
def test_clip_at_one_binds(gpu, i, dtype):
    """8, 14 and 10 of 50 windows have one sample clipped to exactly 1: plane mean re-summed from the clipped plane, bound and
    unbound windows inside one wave, the peak fit around a clipped sample; with and without planes."""
    n, S, density = inputs.CLIP_CASES[i]
    a = inputs.as_samples(inputs.clip_stack(S, density), dtype)
    r = inputs.clip_ref(i, dtype)
    bound = r["corr"] == 1.0
    for device in (False, True):
        *got, planes = run(a, n, S, device=device)
        gate(got, r, planes)
        assert bound.sum() >= 5 and (got[2][bound] == 1.0).all(), "corr is exactly 1 where the reference clips"
        assert_bit_equal(run(a, n, S, planes=False, device=device), got, "with and without planes differ")


# ---- B. every window size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", inputs.SIZES, ids=inputs.SIZE_IDS)
def test_every_window_size(gpu, n, S):
    """All 50 (n, S): the statistics over n^2, the offset (S - n) / 2, the rescue pass's masked window.  The sample type rotates with n."""
    *got, planes = run(inputs.size_samples(n, S), n, S)
    gate(got, inputs.size_ref(n, S), planes)


@pytest.mark.parametrize("n,S", [(n, S) for S in (16, 32, 64) for n in (4, S // 2, S - 2)])
def test_window_sizes_under_the_sample_standard_deviation(gpu, n, S):
    with options(std_ddof=1):
        *got, planes = run(inputs.size_samples(n, S), n, S)
        r = inputs.size_ref(n, S, 1)
    assert not np.array_equal(r["corr"], inputs.size_ref(n, S)["corr"])
    gate(got, r, planes)


# ---- C. the signal score across the instantiations ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("S", [16, 32, 64])
def test_signal_score_in_every_instantiation(gpu, S, dtype):
    """Threshold 0.05 on a stack with a window whose block fails while its area passes, one the other way round and 45 passing:
    per pair and per position (signal_mode 1), planes on and off; float samples have a negative background, where "> 0"
    (signal_positive 1) and "!= 0" give different masks."""
    n = inputs.SIGNAL_CASES[S][0]
    a = inputs.as_samples(inputs.signal_stack(S), dtype)
    masks = {}
    for positive in ((0,) if dtype == np.uint8 else (0, 1)):
        for mode in (0, 1):
            with options(signal_positive=positive, signal_mode=mode):
                r = ref.search_piv(a.astype(np.float64), (n, n), (S, S), (S // 2, S // 2), inputs.SIGNAL_THR)
                *got, planes = run(a, n, S, inputs.SIGNAL_THR)
                bare = run(a, n, S, inputs.SIGNAL_THR, planes=False)
            gate(got, r, planes)
            assert_bit_equal(bare, got, "with and without planes differ")
            masks[positive, mode] = np.isnan(got[2])
    if dtype == np.uint8:
        assert 0 < masks[0, 0].sum() < masks[0, 0].size and 0 < masks[0, 1].sum() < masks[0, 1].size
    else:
        assert not masks[0, 0].any() and masks[1, 0].any() and masks[1, 1].any() and not masks[1, 0].all()


# ---- D. non-finite samples --------------------------------------------------------------------------------------------------------
def partners_of(mask):
    """Windows outside `mask` whose neighbour (2j, 2j + 1) of the same pair is inside it: the two would share a packed inverse transform
    in a kernel that packs two windows per job, as the plain per-pair kernels do."""
    flat = mask.reshape(mask.shape[0], -1)
    out = np.zeros_like(flat)
    w = np.arange(flat.shape[1])
    w = w[(w ^ 1) < flat.shape[1]]
    out[:, w] = flat[:, w ^ 1]
    return (out & ~flat).reshape(mask.shape)


def nonfinite_runs(n, S, density, dtype, device):
    clean, dirty = inputs.nonfinite_stack(n, S, density, dtype)
    return run(clean, n, S, device=device), run(dirty, n, S, device=device), inputs.nonfinite_mask(n, S, clean.shape[1:])


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
@pytest.mark.parametrize("n,S,density", inputs.NONFINITE_CASES, ids=[f"{c[0]}in{c[1]}" for c in inputs.NONFINITE_CASES])
def test_nonfinite_samples_stay_in_their_windows(gpu, n, S, density, dtype):
    """A NaN and a +Inf of frame 1 outside every block and a NaN inside one: pair 0 is NaN where the AREA of frame 1 holds a sample,
    pair 1 only where the BLOCK does (a non-finite sample outside the block stays out of the statistics).  Every other window passes
    the gate against the reference of the clean stack, and is bit for bit the result on the clean stack, planes included."""
    r = ref.search_piv(inputs.nonfinite_stack(n, S, density, dtype)[0].astype(np.float64), (n, n), (S, S), (S // 2, S // 2))
    for device in (False, True):
        want, got, mask = nonfinite_runs(n, S, density, dtype, device)
        for name, g in zip(("u", "v", "corr", "s2n"), got):
            assert np.isnan(g[mask]).all(), f"{name}: a window holding a non-finite sample is not NaN"
        assert np.array_equal(np.isnan(got[2]), mask) and np.array_equal(np.isnan(got[3]), mask)
        assert np.isnan(got[4].reshape(mask.shape + (S, S))[mask]).all()
        masked = dict(r, **{k: np.where(mask, np.nan, r[k]) for k in ("u", "v", "corr", "s2n")},
                      planes=np.where(mask.reshape(2, -1, 1, 1), np.nan, r["planes"]))
        gate(got[:4], masked, got[4])
        assert_bit_equal(got, want, "a window outside the mask differs from the clean stack's", where=~mask)


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
@pytest.mark.parametrize("n,S,density", inputs.NONFINITE_CASES, ids=[f"{c[0]}in{c[1]}" for c in inputs.NONFINITE_CASES])
def test_partner_of_a_skipped_window_is_bit_equal_to_the_clean_run(gpu, n, S, density, dtype):
    """The neighbour (2j, 2j + 1) of a window skipped for a non-finite sample, against the run on the clean stack, bit for bit, planes
    included: the search-area kernels run one window per job at every size, so a window's result is a function of its own samples.
    (With two windows packed into one complex float32 inverse transform, as the 16- and 32-point kernels first did, the 7 neighbours of
    the 9 skipped windows of 16 in 32 moved by up to 5.96e-8 in planes and 1.9e-6 in u / v / corr / s2n.)"""
    for device in (False, True):
        want, got, mask = nonfinite_runs(n, S, density, dtype, device)
        partners = partners_of(mask)
        assert partners.sum() >= 1
        print("partners:", int(partners.sum()), "max |plane diff|", float(np.nanmax(np.abs(got[4] - want[4])[partners.reshape(2, -1)], initial=0.0)))
        assert_bit_equal(got, want, "the neighbour of a skipped window differs from the clean stack's", where=partners)


# ---- E. rescue, window counts, float64 on a large offset -------------------------------------------------------------------------
def rescue_stats():
    st = (C.c_int64 * 5)()
    _lib.check(_lib.load().lspiv_rescue_stats(None, st))
    return np.array(st)


@pytest.mark.parametrize("i", range(len(inputs.RESCUE_CASES)), ids=[f"{c[0]}in{c[1]}-{np.dtype(c[6]).name}" for c in inputs.RESCUE_CASES])
def test_rescue_with_a_masked_window(gpu, i):
    """Single bright pixels (test_rescue_covers_sparse_integer_particles) at 6 in 16, 24 in 64 and in float samples: the float64
    rescue pass rebuilds the masked window at other offsets and from other sample types, and its counters grow."""
    n, S, H, W, seed, count, dtype = inputs.RESCUE_CASES[i]
    a = inputs.sparse_integer_particles(H, W, seed, count, dtype)
    before = rescue_stats()
    for device in (False, True):
        *got, planes = run(a, n, S, device=device)
        gate(got, inputs.rescue_ref(i), planes)
        after = rescue_stats()
        print("rescued:", after[2] - before[2], after[3] - before[3])
        assert (after[2] - before[2]) + (after[3] - before[3]) > 0
        before = after


@pytest.mark.parametrize("S,H,W", inputs.COUNT_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in inputs.COUNT_CASES])
def test_single_and_even_window_counts(gpu, S, H, W):
    """One window (a frame of S x S: the second slot of the job is never valid) and a 2 x 3 grid (every job is full), at n = S / 2."""
    a = inputs.count_stack(H, W)
    for x in (a, inputs.as_samples(a, np.float32)):
        r = ref.search_piv(x.astype(np.float64), (S // 2, S // 2), (S, S), (S // 2, S // 2))
        assert r["u"].shape[1:] == ((1, 1) if H == S else (2, 3))
        for device in (False, True):
            *got, planes = run(x, S // 2, S, device=device)
            gate(got, r, planes)


def test_float64_search_on_a_large_dc_offset_host_entry(gpu):
    """Search-area twin of test_float64_stack_on_a_large_dc_offset, 16 in 32, host entry: the frames are narrowed while they are staged,
    after the frame's integer offset has been taken off (option "narrow_offset")."""
    a = inputs.offset_stack()
    *host, planes = run(a, 16, 32)
    gate(host, ref.search_piv(a, (16, 16), (32, 32), (16, 16)), planes)


def test_float64_search_on_a_large_dc_offset_device_entry(gpu):
    """The same stack as float64 in HBM: the search-area loaders take a float64 sample of the window off each float64 sample before
    they convert it (load_row_f64 of piv_fft_impl.h).  Converted as they are, the samples keep 1e-3 of the texture: u 5.7e-4, v 2.5e-3,
    corr 8.1e-4, s2n 9.1e-4, planes 6.5e-4 against the gate's 1e-4 / 2e-6, measured on an MI355X before the loaders did so."""
    a = inputs.offset_stack()
    *dev, planes = run(a, 16, 32, device=True)
    gate(dev, ref.search_piv(a, (16, 16), (32, 32), (16, 16)), planes)
