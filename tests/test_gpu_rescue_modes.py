"""The per-pair float64 rescue pass on a shifted window B (multi-pass PIV) and on a window B cut from the
float32 workspace of a deformation pass (section 2f), on a stack that HAS ill-conditioned fits: single-pixel speckles drifting 1 px per
frame (tests/multipass_ref.py ``rescue_stack``).  Per geometry and sample type: the pass's counters grow, every non-tie window -- the
re-fitted ones included -- passes the sibling file's gate against the float64 reference, and with the pass switched off the same run
keeps every bit but the u, v of re-fitted windows and misses the gate.  The inputs are checked on the CPU (tie shares, finite shares,
offsets the frame clamp changes): tests/test_multipass_host.py, tests/test_deform_host.py."""
import numpy as np
import pytest

from pyorc_amd import _lib, piv
from pyorc_amd.device import DeviceFrames
from tests import deform_ref as dr
from tests import multipass_ref as mp
from tests.test_gpu_deform import gate as deform_gate
from tests.test_gpu_multipass import same_bits
from tests.test_gpu_search_area import gate as shift_gate
from tests.test_gpu_search_area import rel_err
from tests.test_gpu_search_area_paths import rescue_stats

pytestmark = pytest.mark.gpu
TOL = 1e-4
GEOMETRIES = mp.RESCUE_GEOMETRIES
GEO_IDS = [f"{n}@{ov}" for n, ov in GEOMETRIES]
DTYPES = (np.uint8, np.float32, np.float64)
DTYPE_IDS = ("u8", "f32", "f64")


def refitted(call):
    """(result of ``call``, windows the rescue pass re-fitted during it, windows it processed): the cumulative counters, since a batched
    deformation pass has several "last" launches."""
    before = rescue_stats()
    got = call()
    d = rescue_stats() - before
    return got, int(d[2] + d[3]), int(d[4])


def uv_err(got, r):
    ok = ~r["tie"]
    return max(rel_err(got[0][ok], r["u"][ok]), rel_err(got[1][ok], r["v"][ok]))


def check_rescue(run, a, r, gate):
    """The checks every mode shares; returns (windows whose u, v differ with the pass off, re-fitted count)."""
    on, n_fit, n_seen = refitted(lambda: run(a))
    print("re-fitted:", n_fit, "of", n_seen, "windows")
    assert n_fit > 0 and n_seen == r["u"].size
    gate(on[:4], r, on[4])                                         # flagged windows included
    # host and device entry
    dev, n_dev, _ = refitted(lambda: run(DeviceFrames.from_host(a)))
    assert n_dev > 0
    if a.dtype != np.float64:    # (float64 host stacks are narrowed to float32 while staged; in HBM they stay float64)
        same_bits(dev, on, "host and device entry points differ")
        assert n_dev == n_fit
    else:
        gate(dev[:4], r, dev[4])
    same_bits(run(a, planes=False), on[:4], "without planes")
    # the pass switched off
    old = _lib.get_option("rescue")
    _lib.set_option("rescue", 0)
    try:
        off, n_off, _ = refitted(lambda: run(a))
    finally:
        _lib.set_option("rescue", old)
    assert n_off == 0
    same_bits(off[2:], on[2:], "corr, s2n and the planes keep their bits without the pass")
    differ = ~(((off[0] == on[0]) | (np.isnan(off[0]) & np.isnan(on[0]))) & ((off[1] == on[1]) | (np.isnan(off[1]) & np.isnan(on[1]))))
    print("windows that differ without the pass:", int(differ.sum()), "| u, v error with the pass", uv_err(on, r), "without", uv_err(off, r))
    assert 1 <= differ.sum() <= n_fit                              # only re-fitted windows differ: the others keep their bits
    assert uv_err(on, r) <= TOL < uv_err(off, r)                   # the gate above rested on the branch under test
    return differ, n_fit


# ---- the shifted window B (piv_rescue.hip: p.shift, window_shift per pair and window) ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,ov", GEOMETRIES, ids=GEO_IDS)
def test_rescue_reads_the_shifted_window_at_its_clamped_offset(gpu, n, ov, dtype):
    """Offsets that follow the drift on every other column (residual 0), 2 px in y on every other pair, and offsets pointing out of the
    frame on re-fitted windows: the rescued u, v are residual + CLAMPED offset (the reference's ``shift``).
    Measured on an MI355X, u8 / f32 / f64 (the re-fitted count is the same for the three; u, v error with the pass at most 1.2e-5):
      geometry  re-fitted of windows  differ without the pass  of those, offset clamped  u, v error without the pass
      16 @ 8    652 of 1536           52 / 51 / 41             1 / 1 / 1                 4.0e-3 / 4.1e-3 / 4.1e-3
      32 @ 16   141 of 308            71 / 85 / 88             8 / 10 / 10               6.3e-3 / 6.0e-3 / 6.0e-3
      64 @ 32   24 of 60              13 / 14 / 15             3 / 4 / 5                 1.8e-2 / 7.2e-3 / 1.1e-2
      64 @ 48   60 of 180             28 / 37 / 30             4 / 6 / 7                 7.8e-3 / 7.2e-3 / 8.0e-3"""
    a, r, raw = mp.rescue_stack(dtype), mp.rescue_ref(n, ov, dtype), mp.rescue_offsets(n, ov)

    def run(x, planes=True):
        return list(piv.piv_pairs_shifted(x, (n, n), (ov, ov), raw, return_planes=planes))

    differ, _ = check_rescue(run, a, r, shift_gate)
    changed = np.any(r["shift"] != raw, axis=-1)
    print("re-fitted windows whose offset the clamp changed:", int((differ & changed).sum()))
    assert (differ & changed).any()
    same_bits(run(a), list(piv.piv_pairs_shifted(a, (n, n), (ov, ov), r["shift"].astype(np.int16), return_planes=True)), "the clamped offset is not the one used")


# ---- the window B cut from a deformation pass's float32 workspace (p.warped: launch_rescue_t<uint8_t, float>, <float, float>, <double, float>)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("field", dr.RESCUE_FIELDS)
@pytest.mark.parametrize("n,ov", GEOMETRIES, ids=GEO_IDS)
def test_rescue_reads_the_warped_window_from_the_workspace(gpu, n, ov, field, dtype):
    """"uniform": the warp moves frame t+1 by the drift, the residual is exactly 0; "mixed": the warp interpolates.
    Measured on an MI355X, u8 / f32 / f64 (the re-fitted count is the same for the three; u, v error with the pass at most 1.7e-5):
      geometry, field   re-fitted of windows  differ without the pass  u, v error without the pass
      16 @ 8  uniform   648 of 1536           8 / 8 / 8                2.1e-3 / 1.6e-3 / 1.6e-3
      16 @ 8  mixed     650 of 1536           650 / 650 / 650          1.3e-2 / 1.4e-2 / 1.4e-2
      32 @ 16 uniform   140 of 308            20 / 22 / 21             1.2e-2 / 2.2e-2 / 3.3e-2
      32 @ 16 mixed     124 of 308            123 / 124 / 124          3.8e-3 / 5.0e-3 / 3.2e-3
      64 @ 32 uniform   24 of 60              10 / 10 / 7              1.2e-2 / 1.7e-2 / 7.6e-3
      64 @ 32 mixed     26 of 60              26 / 26 / 26             2.7e-3 / 3.1e-3 / 2.2e-3
      64 @ 48 uniform   60 of 180             15 / 13 / 14             1.7e-2 / 1.7e-2 / 1.6e-2
      64 @ 48 mixed     66 of 180             66 / 66 / 66             3.5e-3 / 3.4e-3 / 2.6e-3"""
    a, r, nodes = mp.rescue_stack(dtype), dr.rescue_ref(n, ov, field, dtype), dr.rescue_nodes(n, ov, field)

    def run(x, planes=True):
        return list(piv.piv_pairs_deformed(x, (n, n), (ov, ov), nodes, return_planes=planes))

    check_rescue(run, a, r, deform_gate)
