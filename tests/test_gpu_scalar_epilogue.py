"""The "scalar_epilogue" form of the per-pair 32 x 32 walking kernels (csrc/piv_fft_impl.h, SCAL; option "scalar_epilogue" = 1) against the
form it replaces ("scalar_epilogue" = 0, on "lds_light" = 1): the first-match searches for the peak's row and column, the near-tie test,
the wrapped neighbour indices and the record word come from ballots and the scalar unit, one value per 32-lane group, instead of DPP
chains and vector arithmetic.  Integer first-match and index arithmetic -- hence the same BITS in u, v, corr, s2n and the planes, NaN
masks and payloads included, and the same rescue records.  No tolerance.

* test hook lspiv_debug_first_match: the ballot first-match and the DPP arg-min (single and paired chain) on whole waves against each
  other and against a numpy model -- the match in each of the 64 lanes, several matches, a match only in the other group, no match in
  one or in both groups (1 << 12, as the DPP form gives);
* the cases of tests/test_gpu_lds_light.py: uint8 and float32 stacks of 64 x 96 (15 windows: an odd count, so a wave holds an invalid job
  and the two groups of a wave sit in different segments), 3 / 25 / 31 / 32 / 33 / 75 pairs (a short segment; the anchor of 25; around
  the 16 iterations = 32 planes after which the staged records are fitted; three segments) at pair offsets 0 and 7, rescue pass on and off;
* the stack with period 16 along x: every window takes the "amb" cold path, which must see the same ip, jp and threshold;
* zero-variance windows (dead planes) and non-finite float32 samples (skipped planes: no first match at all);
* peaks on every border row and column of the plane: a stack with period 32 in both directions whose frames are rolled against each
  other, so that every window's plane has its maximum exactly at the roll -- the wraps of the neighbour indices are what moved to the
  scalar side.  With "border_peak" = 2 the results are the integer peaks, and the test checks that the border was in fact reached."""
import ctypes as C
import functools

import numpy as np
import pytest
from test_gpu_lds_light import tied_stack
from test_gpu_unpack_dpp import H, OV, W, WS, host_stack, options, rescue_lists, same_bytes

from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames

pytestmark = pytest.mark.gpu
NONE = 1 << 12
PAIRS = (3, 25, 31, 32, 33, 75)
OFFSETS = (0, 7)
N_WIN = 15


# ---- the first-match search on whole waves ------------------------------------------------------------------------------------------
def first_match(form, flags):
    flags = np.ascontiguousarray(flags, np.uint32)
    assert flags.ndim == 2 and flags.shape[1] == 64
    out = np.empty_like(flags)
    _lib.check(_lib.load().lspiv_debug_first_match(form, C.c_void_p(flags.ctypes.data), C.c_void_p(out.ctypes.data), flags.shape[0]))
    return out


def first_match_model(flags):
    out = np.empty(flags.shape, np.uint32)
    sh = (np.arange(32) + 16) & 31
    for h in (0, 1):
        m = flags[:, 32 * h:32 * h + 32] != 0
        out[:, 32 * h:32 * h + 32] = np.where(m, sh[None, :], NONE).min(axis=1, keepdims=True)
    return out


def match_waves():
    rng = np.random.default_rng(20261020)
    waves = []
    for l in range(64):                                  # the match in each of the 64 lanes: the other group has none
        w = np.zeros(64, np.uint32)
        w[l] = 1 + l
        waves.append(w)
    for l in range(64):                                  # ... and with one match in the other group as well
        w = np.zeros(64, np.uint32)
        w[l] = 1
        w[(l + 37) % 32 + 32 * (1 - l // 32)] = 0x80000000
        waves.append(w)
    for density in (0.05, 0.2, 0.5, 0.9):                # several matches
        for _ in range(16):
            waves.append((rng.random(64) < density).astype(np.uint32))
    waves.append(np.ones(64, np.uint32))                 # every lane
    for lanes in ((15, 16), (0, 31), (16, 17), (31, 32), (47, 48), (32, 63)):   # around the rotation by 16 and the group boundary
        w = np.zeros(64, np.uint32)
        w[list(lanes)] = 1
        waves.append(w)
    for half in (0, 1):                                  # a match only in one group, in several lanes
        w = np.zeros(64, np.uint32)
        w[32 * half + rng.permutation(32)[:5]] = 7
        waves.append(w)
    waves.append(np.zeros(64, np.uint32))                # no match in either group
    return np.array(waves, np.uint32)


def test_ballot_first_match_is_the_dpp_arg_min(gpu):
    flags = match_waves()
    want = first_match_model(flags)
    assert (want[:64][np.arange(64), 32 * (1 - np.arange(64) // 32)] == NONE).all(), "the first cases leave the other group empty"
    assert (want[-1] == NONE).all()
    dpp, ballot, paired = first_match(0, flags), first_match(1, flags), first_match(2, flags)
    assert ballot.tobytes() == dpp.tobytes(), "ballot + bit scan against the DPP arg-min"
    assert paired.tobytes() == dpp.tobytes(), "the paired DPP chain against the single one"
    assert ballot.tobytes() == want.tobytes(), "against the numpy model"
    with pytest.raises(_lib.LspivError):
        first_match(3, flags[:1])


# ---- the kernels: new form against former form ------------------------------------------------------------------------------------------
def test_option_is_listed(gpu):
    default = _lib.get_option("scalar_epilogue")
    assert default in (0, 1)
    with options(scalar_epilogue=1 - default):
        assert _lib.get_option("scalar_epilogue") == 1 - default
    assert _lib.get_option("scalar_epilogue") == default
    with pytest.raises(_lib.LspivError):
        _lib.set_option("scalar_epilogue", 2)


def to_device(a):
    a = np.ascontiguousarray(a)
    d = DeviceFrames.empty(a.shape, a.dtype)
    _lib.check(_lib.load().lspiv_memcpy_h2d(d.c_ptr, _lib.ptr(a), a.nbytes))
    return d


@functools.lru_cache(maxsize=None)
def dev_stack(kind, pairs):
    return to_device(host_stack(kind)[:pairs + 1])


def scalar_against_former(call, what, want_records=False):
    for rescue in (0, 1):
        with options(rescue=rescue, defer_fit=1, unpack_dpp=1, lds_light=1, scalar_epilogue=0):
            want = call()
            lists_want = rescue_lists() if rescue else None
        with options(rescue=rescue, defer_fit=1, unpack_dpp=1, lds_light=1, scalar_epilogue=1):
            got = call()
            lists_got = rescue_lists() if rescue else None
        same_bytes(got, want, what + ("rescue", rescue))
        if rescue:
            assert np.array_equal(lists_got[0], lists_want[0]), "fit records"
            assert np.array_equal(lists_got[1], lists_want[1]), "amb records"
            if want_records:
                assert lists_got[0].shape[0] + lists_got[1].shape[0] >= 1, "no rescue record: the lists compare nothing"
    return got, lists_got


# (stack, signal threshold, planes, further options): the flagship's kernel and its float32 twin, then every other instantiation once
CONTENT = {"u8": ("u8", None, False, {}), "f32": ("f32", None, False, {})}
OTHER = {"u8-nz-planes": ("u8", 0.02, True, {}), "u8-planes": ("u8", None, True, {}), "u8-nz": ("u8", 0.02, False, {}),
         "f32-nz-planes": ("f32", 0.02, True, {}), "f32-planes": ("f32", None, True, {}), "f32-nz": ("f32", 0.02, False, {}),
         "f64": ("f64", None, False, {}), "f64-planes": ("f64", None, True, {}),
         "u8-flagged": ("u8", None, False, {"rescue_kappa": 200000, "rescue_tau": 1000000})}   # an allowance that fills the rescue lists


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("content", list(CONTENT))
def test_scalar_form_has_the_bits_of_the_former(gpu, content, pairs, offset):
    kind, thr, planes, opts = CONTENT[content]
    d = dev_stack(kind, pairs)

    def call():
        return list(piv.piv_pairs(d, WS, OV, signal_threshold=thr, return_planes=planes, pair_offset=offset))

    with options(**opts):
        got, _ = scalar_against_former(call, (content, pairs, offset))
    assert got[0].shape == (pairs, 3, 5) and np.isfinite(got[0]).any()


@pytest.mark.parametrize("content", list(OTHER))
def test_every_instantiation_has_the_bits_of_the_former(gpu, content):
    kind, thr, planes, opts = OTHER[content]
    d = dev_stack(kind, 33)

    def call():
        return list(piv.piv_pairs(d, WS, OV, signal_threshold=thr, return_planes=planes, pair_offset=7))

    with options(**opts):
        got, _ = scalar_against_former(call, (content,), want_records=content == "u8-flagged")
    assert np.isfinite(got[0]).any()


def test_option_is_ignored_without_its_base_forms(gpu):
    """lds_light = 0, unpack_dpp = 0 or defer_fit = 0: the former kernels run whatever "scalar_epilogue" says -- and give the same bytes."""
    d = dev_stack("u8", 33)

    def call():
        return list(piv.piv_pairs(d, WS, OV, pair_offset=7))

    with options(defer_fit=1, unpack_dpp=1, lds_light=1, scalar_epilogue=0):
        want = call()
    for defer, udpp, lite in ((1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 0, 0)):
        with options(defer_fit=defer, unpack_dpp=udpp, lds_light=lite, scalar_epilogue=1):
            same_bytes(call(), want, ("defer_fit", defer, "unpack_dpp", udpp, "lds_light", lite))


@pytest.mark.parametrize("planes", [False, True])
def test_scalar_form_in_the_amb_cold_path(gpu, planes):
    pairs = 3
    d = to_device(tied_stack()[:pairs + 1])

    def call():
        return list(piv.piv_pairs(d, WS, OV, return_planes=planes))

    _, lists = scalar_against_former(call, ("tied", planes), want_records=True)
    # every window is ambiguous: a record with its second candidate (two samples within tau) or an entry of the "amb" list (more)
    with_second = int((lists[0][:, 2] != 0xffffffff).sum()) if lists[0].size else 0
    assert with_second + lists[1].shape[0] == pairs * N_WIN


def nonfinite_stack():
    f = host_stack("f32").copy()
    f[2, 40, 50] = np.nan        # frame 2: pairs 1 and 2, the four windows over the sample
    f[5, 10, 70] = np.inf
    f[9, 33, 20] = -np.inf
    f[12, :32, :32] = np.nan     # a whole window
    return f[:34]


def test_dead_and_skipped_planes(gpu):
    """Zero-variance windows (exactly-zero planes: every sample ties with the maximum) and non-finite samples (planes without any match)."""
    dead = dev_stack("f32-dead", 33)
    got, _ = scalar_against_former(lambda: list(piv.piv_pairs(dead, WS, OV, pair_offset=7)), ("f32-dead",))
    u, corr = got[0], got[2]
    assert np.all(corr[:, 0, 0] == 0.0) and np.all(np.isnan(u[:, 0, 0])) and np.isfinite(u[:, 1:, 1:]).any()
    u8 = host_stack("u8")[:34].copy()
    u8[:, 32:, 64:] = 200        # window (2, 4) is constant over time, the windows around it partly
    d8 = to_device(u8)
    got, _ = scalar_against_former(lambda: list(piv.piv_pairs(d8, WS, OV, return_planes=True)), ("u8-dead",))
    assert np.all(got[2][:, 2, 4] == 0.0) and np.all(np.isnan(got[0][:, 2, 4]))
    nf = to_device(nonfinite_stack())
    got, _ = scalar_against_former(lambda: list(piv.piv_pairs(nf, WS, OV, return_planes=True)), ("f32-nonfinite",))
    corr = got[2]
    assert np.isnan(corr[1:3, 1:3, 2:4]).all() and np.isnan(corr[11:13, 0, 0]).all() and np.isfinite(corr[0]).all()


# ---- peaks on the border of the plane ---------------------------------------------------------------------------------------------------
EDGE = (-16, -15, 15)   # a roll of -16 is the plane's first row / column whatever the sign convention, -15 and 15 its last under either


def border_rolls():
    rolls = [(e, k) for e in EDGE for k in range(-16, 16)] + [(k, e) for e in EDGE for k in range(-16, 16)]
    return rolls


def border_stack():
    rng = np.random.default_rng(20261023)
    base = np.tile(rng.integers(0, 256, (32, 32), dtype=np.uint8), (H // 32, W // 32))
    frames, pos = [base], np.zeros(2, np.int64)
    for dy, dx in border_rolls():
        pos += (dy, dx)
        frames.append(np.roll(base, tuple(pos), axis=(0, 1)))
    return np.ascontiguousarray(np.array(frames, np.uint8))


def test_peaks_on_every_border_row_and_column(gpu):
    d = to_device(border_stack())
    pairs = len(border_rolls())

    def call():
        return list(piv.piv_pairs(d, WS, OV))

    scalar_against_former(call, ("border", "nan"))              # the default: a peak on the border gives NaN
    with options(border_peak=2):                                # the integer peak: shows where the search went
        got, _ = scalar_against_former(call, ("border", "integer"))
    u, v = got[0], got[1]
    assert u.shape == (pairs, 3, 5)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    jp, ip = np.rint(u + 16).astype(int), np.rint(v + 16).astype(int)   # (a roll of -15 or 15 may sit one sample inside: a sub-pixel fit)
    assert (ip == ip[:, :1, :1]).all() and (jp == jp[:, :1, :1]).all(), "every window of a pair sees the same roll"
    seen = set(zip(ip[:, 0, 0].tolist(), jp[:, 0, 0].tolist()))
    border = {(i, j) for i in range(32) for j in range(32) if i in (0, 31) or j in (0, 31)}
    assert border <= seen, sorted(border - seen)[:8]
