"""The "lds_light" form of the per-pair 32 x 32 walking kernels (csrc/piv_fft_impl.h, LITE; option "lds_light" = 1) against the form it
replaces ("lds_light" = 0): the 32-lane reductions join their two 16-lane rows with v_permlane16_swap instead of ds_swizzle, the integer
ones that come in pairs in one chain (and, in a build with -DLSPIV_UNPACK_GROUP=n, the un-packing sets its lane mask once per n
exchanged values and exchanges in place).  The same expressions on the same operands -- hence the same BITS in u, v, corr, s2n and the planes, NaN masks and payloads included, and the same rescue records.  No tolerance.

The cases are those of tests/test_gpu_unpack_dpp.py: 64 x 96 frames, 32 x 32 windows at 50 % overlap = 15 windows (an odd count: a wave
holds an invalid job, and the two lane groups of a wave sit in different segments); 3, 25, 26 and 76 pairs (one short segment; exactly
the anchor of 25; one pair more; three segments and one pair), each at pair offsets 0 and 7; uint8, float32 and float64 with and without
planes and signal threshold, one NaN sample, one zero-variance window, an allowance that fills the rescue lists.

One more stack reaches the "amb" cold path of the search (its two reductions run only there): particle_stack(seed=5) with its first 16
columns repeated across the frame, so that every window has period 16 along x and its circular correlation plane holds its maximum
twice, 16 columns apart.  test_tied_stack_has_two_maxima checks that on the CPU with the float64 oracle."""
import numpy as np
import pytest
from test_gpu_unpack_dpp import CONTENT as DPP_CONTENT
from test_gpu_unpack_dpp import H, OFFSETS, OV, PAIRS, T_MAX, W, WS, dev_stack, options, rescue_lists, same_bytes

from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames
from pyorc_amd.synth import particle_stack

TAU = 4000e-9          # the library's default "rescue_tau" (include/lspiv.h), in units of the plane maximum
TIED_PAIRS = 3


def tied_stack():
    a = particle_stack(T_MAX, H, W, seed=5)
    return np.ascontiguousarray(np.tile(a[:, :, :16], (1, 1, W // 16)))


@pytest.mark.gpu
def test_option_is_listed(gpu):
    default = _lib.get_option("lds_light")
    assert default in (0, 1)
    with options(lds_light=1 - default):
        assert _lib.get_option("lds_light") == 1 - default
    assert _lib.get_option("lds_light") == default
    with pytest.raises(_lib.LspivError):
        _lib.set_option("lds_light", 2)


def light_against_former(call, what, want_records=False):
    for rescue in (0, 1):
        with options(rescue=rescue, defer_fit=1, unpack_dpp=1, lds_light=0):
            want = call()
            lists_want = rescue_lists() if rescue else None
        with options(rescue=rescue, defer_fit=1, unpack_dpp=1, lds_light=1):
            got = call()
            lists_got = rescue_lists() if rescue else None
        same_bytes(got, want, what + ("rescue", rescue))
        if rescue:
            assert np.array_equal(lists_got[0], lists_want[0]), "fit records"
            assert np.array_equal(lists_got[1], lists_want[1]), "amb records"
            if want_records:
                assert lists_got[0].shape[0] + lists_got[1].shape[0] >= 1, "no rescue record: the lists compare nothing"
    return got, lists_got


@pytest.mark.gpu
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("content", list(DPP_CONTENT))
def test_light_form_has_the_bits_of_the_former(gpu, content, pairs, offset):
    kind, thr, planes, opts = DPP_CONTENT[content]
    d = dev_stack(kind, pairs)

    def call():
        return list(piv.piv_pairs(d, WS, OV, signal_threshold=thr, return_planes=planes, pair_offset=offset))

    with options(**opts):
        got, _ = light_against_former(call, (content, pairs, offset), want_records=content == "u8-flagged")
    u, corr = got[0], got[2]
    assert u.shape == (pairs, 3, 5)
    if kind == "f32-nan":
        assert np.isnan(corr[1:3, 1:3, 2:4]).all() and np.isfinite(corr[0]).all()
    elif kind == "f32-dead":
        assert np.all(corr[:, 0, 0] == 0.0) and np.all(np.isnan(u[:, 0, 0])) and np.isfinite(u[:, 1:, 1:]).any()
    else:
        assert np.isfinite(u).any()


@pytest.mark.gpu
def test_option_is_ignored_without_its_base_forms(gpu):
    """unpack_dpp = 0 or defer_fit = 0: the former kernels run whatever "lds_light" says -- and give the same bytes."""
    d = dev_stack("u8", 26)

    def call():
        return list(piv.piv_pairs(d, WS, OV, pair_offset=7))

    with options(defer_fit=1, unpack_dpp=1, lds_light=0):
        want = call()
    for defer, udpp in ((0, 1), (1, 0), (0, 0)):
        with options(defer_fit=defer, unpack_dpp=udpp, lds_light=1):
            same_bytes(call(), want, ("defer_fit", defer, "unpack_dpp", udpp))


def test_tied_stack_has_two_maxima():
    """CPU only: in the float64 oracle every plane of the tied stack (seed 5) has a second sample within tau of its maximum."""
    from oracle import piv_oracle as po

    _, _, corr = po.cross_corr(tied_stack()[:TIED_PAIRS + 1], WS, OV)
    flat = np.sort(corr.reshape(-1, WS[0] * WS[1]), axis=1)
    assert np.isfinite(flat).all() and (flat[:, -1] > 0).all()
    assert (flat[:, -2] >= flat[:, -1] * (1.0 - TAU)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [False, True])
def test_light_form_in_the_amb_cold_path(gpu, planes):
    a = tied_stack()[:TIED_PAIRS + 1]
    d = DeviceFrames.empty(a.shape, a.dtype)
    _lib.check(_lib.load().lspiv_memcpy_h2d(d.c_ptr, _lib.ptr(a), a.nbytes))

    def call():
        return list(piv.piv_pairs(d, WS, OV, return_planes=planes))

    _, lists = light_against_former(call, ("tied", planes), want_records=True)
    # every window is ambiguous: a record with its second candidate (two samples within tau) or an entry of the "amb" list (more)
    n = TIED_PAIRS * 15
    with_second = int((lists[0][:, 2] != 0xffffffff).sum()) if lists[0].size else 0
    assert with_second + lists[1].shape[0] == n
