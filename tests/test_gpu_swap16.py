"""The 32-lane reductions of csrc/common.h in their two forms (test hook lspiv_debug_half_reduce): the last step -- the join of the two
16-lane rows of a half-wave -- through ds_swizzle (form 0) and through v_permlane16_swap (form 1, what "lds_light" runs).  Both forms
must give the same BYTES in every lane, and those of a numpy model of the fixed reduction order: every lane combines its own value with
its partner's at lane ^ 1, ^ 2, ^ 7 (half mirror), ^ 15 (mirror) and ^ 16, one IEEE float32 / two's-complement operation per step.
The integer reductions also have a paired form (half_reduce2_i, forms 2 and 3: two reductions in one chain, rows joined first), which
must give the same bytes again.

One wave of 64 lanes per row of input, its two halves reduce independently.  Inputs: all-distinct values; all-equal values; the extreme
in each of the 64 lanes in turn; the extreme twice, in lanes l and l ^ 16 (a tie across the two rows of a half); for the float sum values
of mixed magnitude (2^-20 .. 2^20, so the order of the additions shows in the low bits; all normal numbers) and +0 / -0 in every
combination of the two rows."""
import ctypes as C

import numpy as np
import pytest

from pyorc_amd import _lib

pytestmark = pytest.mark.gpu
SUM_F, SUM_I, MIN_I, MAX_I = 0, 1, 2, 3
STEPS = (1, 2, 7, 15, 16)


def run(op, form, words):
    words = np.ascontiguousarray(words, np.uint32)
    assert words.ndim == 2 and words.shape[1] == 64
    out = np.empty_like(words)
    _lib.check(_lib.load().lspiv_debug_half_reduce(op, form, C.c_void_p(words.ctypes.data), C.c_void_p(out.ctypes.data), words.shape[0]))
    return out


def model(op, words):
    lanes = np.arange(64)
    if op == SUM_F:
        v = words.view(np.float32).copy()
    elif op == SUM_I:
        v = words.copy()
    else:
        v = words.view(np.int32).copy()
    with np.errstate(over="ignore"):
        for s in STEPS:
            p = v[:, lanes ^ s]
            v = (v + p) if op in (SUM_F, SUM_I) else np.minimum(v, p) if op == MIN_I else np.maximum(v, p)
    return np.ascontiguousarray(v).view(np.uint32)


def integer_waves(extreme, rest_lo, rest_hi):
    rng = np.random.default_rng(20261021)
    waves = [rng.permutation(np.arange(rest_lo, rest_lo + 64, dtype=np.int64)),   # all distinct
             np.full(64, rest_lo + 5, np.int64)]                                   # all equal
    for l in range(64):                                                            # the extreme in each lane in turn
        w = rng.integers(rest_lo, rest_hi, 64)
        w[l] = extreme
        waves.append(w)
    for l in range(64):                                                            # a tie across the two rows of a half
        w = rng.integers(rest_lo, rest_hi, 64)
        w[l] = w[l ^ 16] = extreme
        waves.append(w)
    return np.array(waves, np.int64).astype(np.int32).view(np.uint32)


def float_waves():
    rng = np.random.default_rng(20261022)
    waves = [rng.permutation(np.arange(1, 65)).astype(np.float32) * np.float32(0.37),
             np.full(64, 0.1, np.float32)]
    for l in range(64):
        w = rng.uniform(-1, 1, 64).astype(np.float32)
        w[l] = 3.0e7
        waves.append(w)
    for l in range(64):
        w = rng.uniform(-1, 1, 64).astype(np.float32)
        w[l] = w[l ^ 16] = -3.0e7
        waves.append(w)
    for _ in range(32):                                                            # mixed magnitude
        waves.append((rng.uniform(-1, 1, 64) * 2.0 ** rng.integers(-20, 21, 64)).astype(np.float32))
    for even, odd in ((0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)):         # +-0 per 16-lane row
        w = np.empty(64, np.float32)
        w[(np.arange(64) & 16) == 0] = even
        w[(np.arange(64) & 16) != 0] = odd
        waves.append(w)
    return np.array(waves, np.float32).view(np.uint32)


CASES = {
    "sum_f": (SUM_F, float_waves),
    "sum_i": (SUM_I, lambda: integer_waves(0x7fffffff, -(1 << 30), 1 << 30)),      # wraps
    "min_i": (MIN_I, lambda: integer_waves(-(1 << 31), -1000, 1 << 12)),
    "max_i": (MAX_I, lambda: integer_waves(0x7fffffff, -1000, 0x3f800000)),        # bit patterns of floats in [0, 1] among them
}


@pytest.mark.parametrize("case", list(CASES))
def test_swap_form_has_the_bytes_of_the_swizzle_form(gpu, case):
    op, make = CASES[case]
    words = make()
    want = model(op, words)
    swz, swp = run(op, 0, words), run(op, 1, words)
    assert swp.tobytes() == swz.tobytes(), "the two forms differ"
    assert swz.tobytes() == want.tobytes(), "ds_swizzle form against the numpy model"
    # every lane of a half holds the half's result
    assert (swp[:, :32] == swp[:, :1]).all() and (swp[:, 32:] == swp[:, 32:33]).all()
    if op != SUM_F:
        # the paired reduction on (own value, value of the same lane of the other half): its first result is the half's own, its second
        # the other half's
        assert run(op, 2, words).tobytes() == want.tobytes(), "paired form, first result"
        assert run(op, 3, words).tobytes() == want[:, np.arange(64) ^ 32].tobytes(), "paired form, second result"


def test_hook_rejects_what_it_does_not_have(gpu):
    w = np.zeros((1, 64), np.uint32)
    with pytest.raises(_lib.LspivError):
        run(4, 0, w)
    with pytest.raises(_lib.LspivError):
        run(0, 2, w)
    with pytest.raises(_lib.LspivError):
        run(1, 4, w)
