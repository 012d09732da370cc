"""The fixed-size instantiations of the rescue pass's fit kernel (csrc/piv_rescue.hip: square 16, 32 and 64 px windows of launches without
a search area) against the run-time-geometry kernel, option "rescue_generic" = 1: the same records, the same float64 sums in the same
order, hence the same BITS in every output and the same counters.  Inputs: the speckle stack that drives the pass in
tests/test_gpu_rescue_modes.py (``multipass_ref.rescue_stack`` over ``RESCUE_GEOMETRIES``; re-fitted counts measured on an MI355X in that
file's docstrings: 652, 141, 24 and 60) -- the smallest shapes at which the three fixed sizes and the row steps of 4, 2 and 1 all occur.
A case whose generic run has no fit record FAILS: it would compare nothing.  Which kernel a run took is read back from the library
(the read-only option "rescue_fit_size": the compile-time window size of the last pass's fit kernel, 0 = the generic one), so a dispatch
that quietly kept the generic kernel fails too.  float64 stacks go in as ``DeviceFrames``: a float64 HOST stack is narrowed to float32
while it is staged and would run the float32 kernels a second time; in HBM it stays float64 and reaches ``<double, double>`` and, in
a deformation pass, ``<double, float>``."""
import contextlib

import numpy as np
import pytest

from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames
from tests import deform_ref as dr
from tests import multipass_ref as mp
from tests import test_search_area_host as sa_inputs
from tests.test_gpu_multipass import same_bits
from tests.test_gpu_search_area_paths import rescue_stats

pytestmark = pytest.mark.gpu
GEOMETRIES = mp.RESCUE_GEOMETRIES
GEO_IDS = [f"{n}@{ov}" for n, ov in GEOMETRIES]
DTYPES = (np.uint8, np.float32, np.float64)
DTYPE_IDS = ("u8", "f32", "f64")


@contextlib.contextmanager
def rescue_generic(value):
    old = _lib.get_option("rescue_generic")
    _lib.set_option("rescue_generic", value)
    try:
        yield
    finally:
        _lib.set_option("rescue_generic", old)


def counted(call):
    """(outputs of ``call``, the growth of lspiv_rescue_stats' three totals during it, its "last" counts after it)."""
    before = rescue_stats()
    got = list(call())
    after = rescue_stats()
    return got, (after - before)[2:], after[:2]


def stack(dtype):
    """The speckle stack as the library sees it in ``dtype``: float64 resident in HBM (see the module docstring), the others from the host."""
    a = mp.rescue_stack(dtype)
    return DeviceFrames.from_host(a) if dtype == np.float64 else a


def both_ways(call, what, fixed):
    """``call`` under the generic and under the default kernels: bit-equal outputs (NaN positions included), equal counters; the default
    run's fit kernel was the instantiation of size ``fixed`` (0: the generic one).  Returns the generic run's (outputs, totals' growth,
    last counts)."""
    with rescue_generic(1):
        want, d_want, last_want = counted(call)
        assert _lib.get_option("rescue_fit_size") == 0
    with rescue_generic(0):
        got, d_got, last_got = counted(call)
        assert _lib.get_option("rescue_fit_size") == fixed, (what, _lib.get_option("rescue_fit_size"), fixed)
    print(what, "| generic run: fit", int(d_want[0]), "whole-plane", int(d_want[1]), "of", int(d_want[2]), "windows")
    assert d_want[0] >= 1, "the generic run has no fit record: the fit kernels are not compared"
    same_bits(got, want, what)
    assert np.array_equal(d_got, d_want) and np.array_equal(last_got, last_want), (d_got, d_want, last_got, last_want)
    return want, d_want, last_want


def test_option_is_listed_and_defaults_to_the_fixed_size_kernels(gpu):
    assert _lib.get_option("rescue_generic") == 0
    with rescue_generic(1):
        assert _lib.get_option("rescue_generic") == 1
    assert _lib.get_option("rescue_generic") == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,ov", GEOMETRIES, ids=GEO_IDS)
def test_plain_launch_is_bit_equal_to_the_generic_kernels(gpu, n, ov, dtype):
    a = stack(dtype)
    both_ways(lambda: piv.piv_pairs(a, (n, n), (ov, ov), return_planes=True), f"piv_pairs {n}@{ov}", n)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,ov", GEOMETRIES, ids=GEO_IDS)
def test_shifted_launch_is_bit_equal_to_the_generic_kernels(gpu, n, ov, dtype):
    """Window B at its clamped offset (p.shift)."""
    a, raw = stack(dtype), mp.rescue_offsets(n, ov)
    both_ways(lambda: piv.piv_pairs_shifted(a, (n, n), (ov, ov), raw, return_planes=True), f"piv_pairs_shifted {n}@{ov}", n)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,ov", GEOMETRIES, ids=GEO_IDS)
def test_deformed_launch_is_bit_equal_to_the_generic_kernels(gpu, n, ov, dtype):
    """Window B from the float32 workspace (TB = float under uint8 / float64 stacks); the field whose warp interpolates.
    ``<double, float, 32, 32>`` is not instantiated (it needs more VGPRs than its generic sibling): that launch keeps the generic kernel."""
    a, nodes = stack(dtype), dr.rescue_nodes(n, ov, "mixed")
    fixed = 0 if (dtype == np.float64 and n == 32) else n
    both_ways(lambda: piv.piv_pairs_deformed(a, (n, n), (ov, ov), nodes, return_planes=True), f"piv_pairs_deformed {n}@{ov}", fixed)


def tie_stack(dtype):
    """The speckle stack plus two frames whose columns alternate and whose rows move by 3 (the construction of
    test_rescue_of_a_many_way_tie_in_a_tall_window): every plane of that pair has 16 exactly equal maxima at 32 x 32 -- whole-plane records."""
    a = mp.rescue_stack(dtype)
    H, W = a.shape[1:]
    rng = np.random.default_rng(5)
    r = rng.integers(4, 50, H + 8)
    col = np.where(np.arange(W) % 2 == 0, 1, 5)
    tie = np.stack([r[t * 3: t * 3 + H, None] * col[None, :] for t in range(2)])
    assert tie.max() <= 250
    a = np.concatenate([a, tie.astype(dtype)])
    return DeviceFrames.from_host(a) if dtype == np.float64 else a


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_both_lists_in_one_launch_at_32(gpu, dtype):
    """Fit records and whole-plane records in the same launch, and a second launch right after it: the same outputs and the same "last"
    counts, i.e. the pass's last block cleared the counters.  Measured on an MI355X, u8 and f32: 140 fit + 154 whole-plane records of
    462 windows."""
    a = tie_stack(dtype)

    def call():
        return piv.piv_pairs(a, (32, 32), (16, 16), return_planes=True)

    want, d, last = both_ways(call, "speckles and a tie pair, 32@16", 32)
    assert last[0] >= 1 and last[1] >= 1, last             # both lists were filled by the ONE launch of the generic run
    again, d2, last2 = counted(call)                       # (the fixed-size kernels: the option is back at 0)
    same_bits(again, want, "second launch")
    assert np.array_equal(last2, last) and np.array_equal(d2, d)


@pytest.mark.parametrize("i", (1, 2), ids=("24in64-u8", "16in32-f32"))
def test_search_area_launch_keeps_the_generic_kernels(gpu, i):
    """p.nw != 0: the option changes nothing (the dispatch condition).  Measured on an MI355X: 24 and 2 fit records of 30 windows."""
    n, S, H, W, seed, count, dtype = sa_inputs.RESCUE_CASES[i]
    a = sa_inputs.sparse_integer_particles(H, W, seed, count, dtype)
    both_ways(lambda: piv.piv_pairs(a, (n, n), (S // 2, S // 2), search_area_size=(S, S), return_planes=True), f"search area {n} in {S}", 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_size_without_an_instantiation_keeps_the_generic_kernels(gpu, dtype):
    """24 x 24 @ 12.  Measured on an MI355X: 281 fit records of 600 windows."""
    a = stack(dtype)
    both_ways(lambda: piv.piv_pairs(a, (24, 24), (12, 12), return_planes=True), "piv_pairs 24@12", 0)
