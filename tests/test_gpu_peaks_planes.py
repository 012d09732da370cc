"""Peaks from caller-supplied planes against a float64 fit of the same samples: ``piv.u_v_displacement`` (csrc/piv_direct.hip,
``peaks_kernel``) and ``Ensemble.finish`` on an imported state, on the planes of tests/peaks_inputs.py -- a chosen arg-max (corners,
edges, lane and iteration boundaries of the 64-lane search, sides of 1 and 2, fewer than 64 samples), exact ties, NaN / inf / signed
zeros / negative samples, Gaussian peaks from sharp to broad and from 1 down to 1e-6 high, clipped neighbours, 70 000 planes in a call.

The reference is ``oracle.piv_oracle.u_v_displacement`` on the kernel's own float32 samples widened to float64.  There is no plane noise
on this path, so the NaN masks agree on EVERY plane and every finite value is held to the project's gate,
|got - ref| <= 1e-4 max(|ref|, 0.05 px) (plus one float32 ulp of side / 2 above 64 samples per side: the result is formed as
(float)i + offset - side / 2).  Nothing the kernel returns decides what is compared; no plane is set aside.

MEASURED on an MI355X, worst relative error |got - ref| / max(|ref|, 0.05) per row of the "fit" family (all sizes, 324 centres each),
"float32" = option rescue = 0, the fit in float32 with v_log_f32 / v_rcp_f32 as before this test, "shipped" = the default, where the
planes common.h's ``peak_cond`` flags at the default rescue_kappa are fitted again in float64 from their five samples (csrc/piv_peaks.h):

    size sigma   h = 1, bg 0          h = 0.3, bg 0.2      h = 0.02, bg 0       h = 1e-6, bg 0         (float32 -> shipped)
    16    0.7    9.3e-6 -> 9.3e-6     9.4e-6 -> 9.4e-6     8.0e-6 -> 8.0e-6     1.2e-5 -> 1.2e-5
    16    1.5    9.3e-6 -> 9.3e-6     1.0e-5 -> 5.0e-6     1.1e-5 -> 1.1e-5     3.3e-5 -> 3.3e-5
    16    3      9.4e-6 -> 8.5e-7     1.6e-5 -> 2.5e-6     2.9e-5 -> 6.0e-6     1.06e-4 -> 3.1e-5
    33    0.7    1.9e-5 -> 1.9e-5     1.8e-5 -> 1.8e-5     1.7e-5 -> 1.7e-5     2.0e-5 -> 2.0e-5
    33    1.5    1.9e-5 -> 1.9e-5     1.8e-5 -> 5.1e-6     2.0e-5 -> 2.0e-5     4.2e-5 -> 4.2e-5
    33    3      1.9e-5 -> 8.5e-7     2.6e-5 -> 5.3e-6     3.2e-5 -> 6.0e-6     1.06e-4 -> 2.9e-5
    33    5      1.9e-5 -> 3.5e-7     2.9e-5 -> 4.0e-8     6.1e-5 -> 1.9e-6     3.27e-4 -> 5.4e-6
    33    8      1.8e-5 -> 5.9e-8     6.5e-5 -> 4.6e-8     1.97e-4 -> 5.3e-8    6.59e-4 -> 5.1e-8
    33   12      1.8e-5 -> 5.6e-8     1.13e-4 -> 5.1e-8    3.14e-4 -> 5.7e-8    2.00e-3 -> 5.1e-8
    64    0.7    3.4e-5 -> 3.4e-5     3.8e-5 -> 3.8e-5     3.3e-5 -> 3.3e-5     3.7e-5 -> 3.7e-5
    64    1.5    3.5e-5 -> 3.5e-5     3.5e-5 -> 1.5e-5     3.6e-5 -> 3.6e-5     4.6e-5 -> 4.6e-5
    64    3      3.6e-5 -> 8.5e-7     4.3e-5 -> 7.8e-6     5.2e-5 -> 6.0e-6     1.21e-4 -> 3.6e-5
    64    5      3.8e-5 -> 3.5e-7     5.2e-5 -> 4.0e-8     6.1e-5 -> 1.9e-6     3.27e-4 -> 5.4e-6
    64    8      3.4e-5 -> 5.9e-8     8.3e-5 -> 4.6e-8     1.97e-4 -> 5.3e-8    6.59e-4 -> 5.1e-8
    64   12      3.7e-5 -> 5.6e-8     1.13e-4 -> 5.1e-8    3.22e-4 -> 5.7e-8    2.02e-3 -> 5.1e-8
    clipped neighbours (one / two / four zeros), all sizes: 9.1e-6 / 4.1e-6 / 0 -> 3.6e-8 / 3.2e-8 / 0; three equal samples: 7.9e-6 both

Planes outside the gate in float32: 4 of 3 946 (16 x 16), 484 of 7 834 (33 x 33), 497 of 7 834 (64 x 64) -- the broad and the low peaks,
as the CPU restatement of tests/test_peaks_host.py predicts (its numpy log2 gives 0 / 560 / 568).  Planes fitted in float64 by the shipped
path: 890, 4 658 and 4 658 (786, 4 254 and 4 262 of them change their bits); none outside the gate, worst 4.6e-5 on a plane nobody
flagged.  "argmax" family: NaN masks equal on all 397 planes, worst 1.8e-5 up to 64 samples per side and 9.7e-5 at 130 x 257 (i = 65,
j = 128: the float32 ulp of the allowance).  Imported ensemble states (48 windows each): worst 5.5e-6 ... 3.1e-5, 20 ... 35 windows flagged.

Without the re-fit (the "float32" column is that kernel) ``test_fit_family`` fails at all three sizes.  The kernel's former ranking (NaN
as +inf, first maximum) takes the interior inf of the ``inf-nan-inf`` planes, whose fit is finite (offset 0), where np.argmax takes the
first NaN even behind an inf and the reference is NaN: the NaN-mask comparison of the "argmax" tests is what catches it."""
import contextlib

import numpy as np
import pytest

from pyorc_amd import _lib, piv
from pyorc_amd.synth import particle_stack
from tests import peaks_inputs as pk
from tests.test_gpu_unpack_dpp import rescue_lists

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def options(**kw):
    old = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def uv(planes):
    """u, v (k,) float32 of (k, wy, wx) planes through the drop-in, as one row of k windows."""
    u, v = piv.u_v_displacement(planes[None], 1, len(planes))
    assert u.shape == v.shape == (1, 1, len(planes)) and u.dtype == v.dtype == np.float32
    return u.ravel(), v.ravel()


def fit_rows(n, u, v):
    """{(sigma, h) or kind: worst relative error} over the size-n "fit" planes."""
    f = pk.fit_family(n)
    ru, rv = pk.fit_reference(n)
    rel = np.maximum(pk.rel_error(u, ru), pk.rel_error(v, rv))
    rows = {}
    for sigma in sorted(set(f.sigma[f.kind == "gauss"])):
        for h, _ in pk.HEIGHTS:
            rows[(sigma, h)] = float(rel[(f.kind == "gauss") & (f.sigma == sigma) & (f.h == h)].max())
    for kind in ("clip1", "clip2", "clip4", "row3"):
        rows[kind] = float(rel[f.kind == kind].max())
    return rows


@pytest.mark.parametrize("shape", pk.ARGMAX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_argmax_family(gpu, shape):
    fam = pk.argmax_family(shape)
    u, v = uv(fam.planes)
    worst = pk.assert_within_gate(u, v, *pk.argmax_reference(shape), shape, f"argmax {shape}")
    print(f"argmax {shape}: {len(fam.planes)} planes, worst relative error {worst:.3e}")


@pytest.mark.parametrize("shape", pk.ARGMAX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("opts", ({"border_peak": 1}, {"border_peak": 2}, {"v_sign": 1}), ids=("centre", "integer", "v-negated"))
def test_argmax_family_under_other_semantics(gpu, shape, opts):
    fam = pk.argmax_family(shape)
    ref_u, ref_v = pk.argmax_reference(shape, **opts)
    with options(**opts):
        u, v = uv(fam.planes)
    pk.assert_within_gate(u, v, ref_u, ref_v, shape, f"argmax {shape} {opts}")
    # border peaks: no arithmetic, the reference's float32 bits
    wy, wx = shape
    flat = fam.planes.reshape(len(fam.planes), -1)
    idx = np.argmax(flat, axis=1)
    i, j = idx // wx, idx % wx
    border = ((i == 0) | (i == wy - 1) | (j == 0) | (j == wx - 1)) & ~np.isnan(flat[np.arange(len(flat)), idx])
    assert border.any()
    if "border_peak" in opts:
        assert np.all(np.isfinite(ref_u[border])) and np.all(np.isfinite(ref_v[border]))
        assert u[border].tobytes() == ref_u[border].astype(np.float32).tobytes(), (shape, opts, "u on border peaks")
        assert v[border].tobytes() == ref_v[border].astype(np.float32).tobytes(), (shape, opts, "v on border peaks")
    else:
        assert np.all(np.isnan(u[border])) and np.all(np.isnan(v[border]))


@pytest.mark.parametrize("n", pk.FIT_SIZES)
def test_fit_family(gpu, n):
    f = pk.fit_family(n)
    u, v = uv(f.planes)
    refitted = _lib.get_option("peaks_refitted")
    rows = fit_rows(n, u, v)
    print(f"fit {n}: {len(f.planes)} planes, {refitted} fitted in float64")
    for key, worst in rows.items():
        print(f"  {key}: worst {worst:.2e}")
    pk.assert_within_gate(u, v, *pk.fit_reference(n), (n, n), f"fit {n}")
    assert 0 < refitted < len(f.planes)


@pytest.mark.parametrize("n", pk.FIT_SIZES)
def test_rescue_0_keeps_the_float32_fits_and_the_others_keep_their_bits(gpu, n):
    f = pk.fit_family(n)
    u, v = uv(f.planes)
    refitted = _lib.get_option("peaks_refitted")
    with options(rescue=0):
        u0, v0 = uv(f.planes)
        assert _lib.get_option("peaks_refitted") == 0
    ru, rv = pk.fit_reference(n)
    outside = (np.abs(u0 - ru) > pk.bound(ru, n)) | (np.abs(v0 - rv) > pk.bound(rv, n))
    differ = (u.view(np.uint32) != u0.view(np.uint32)) | (v.view(np.uint32) != v0.view(np.uint32))
    print(f"fit {n} in float32: {outside.sum()} of {len(f.planes)} planes outside the gate; {differ.sum()} differ from the shipped result, "
          f"{refitted} fitted in float64")
    for key, worst in fit_rows(n, u0, v0).items():
        print(f"  {key}: worst {worst:.2e}")
    assert differ.sum() <= refitted
    assert not np.any(outside & ~differ), "a plane outside the gate in float32 that the shipped path left alone"


def test_results_do_not_depend_on_the_calls_around_them(gpu):
    f = pk.fit_family(33)
    k = len(f.planes)
    small = uv(pk.fit_family(16).planes)                  # a context that has seen nothing larger grows its workspace on the next call
    whole = uv(f.planes)
    cuts = (0, 1, 1 + k // 7, k)                          # three calls of uneven size
    parts = [uv(f.planes[a:b]) for a, b in zip(cuts, cuts[1:])]
    for c in range(2):
        assert np.concatenate([p[c] for p in parts]).tobytes() == whole[c].tobytes(), "one call against three"
    uv(pk.fit_family(64).planes)                          # four times the bytes: the workspace is allocated again
    again = uv(f.planes)
    assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes(), "after a larger volume"
    again16 = uv(pk.fit_family(16).planes)
    assert again16[0].tobytes() == small[0].tobytes() and again16[1].tobytes() == small[1].tobytes()


def test_many_planes_and_none(gpu):
    p = pk.many_family()
    assert len(p) > 65535
    u, v = uv(p)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and u.size == pk.MANY
    pk.assert_within_gate(u, v, *pk.many_reference(), (4, 4), "many")
    u, v = piv.u_v_displacement(np.empty((0, 6, 4, 4), np.float32), 2, 3)
    assert u.shape == v.shape == (0, 2, 3) and u.dtype == v.dtype == np.float32
    u, v = piv.u_v_displacement(np.empty((3, 0, 4, 4), np.float32), 0, 5)
    assert u.shape == v.shape == (3, 0, 5)


ENSEMBLE_WINDOWS = ((16, 16), (32, 32), (64, 64), (24, 24), (9, 9), (24, 16))


@pytest.mark.parametrize("window", ENSEMBLE_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_imported_ensemble_state(gpu, window):
    wy, wx = window
    rows, cols = 6, 8
    n_win = rows * cols
    planes = pk.ensemble_planes(window, n_win)
    count = np.array([1.0, 2.0, 4.0], np.float32)[np.arange(n_win) % 3]
    low = 17
    count_min, n_frames = 0.5, 2.0                        # the filter passes count >= 1
    count[low] = 0.5
    sums = planes * count[:, None, None]                  # powers of two: the mean is exact
    e = piv.Ensemble((rows * wy, cols * wx), window, (0, 0))
    try:
        assert (e.n_rows, e.n_cols) == (rows, cols)
        e.import_state(sums, count)
        u, v, cnt, mean = e.finish(count_min, n_frames, return_mean=True)
        st = e.stats()
    finally:
        e.close()
    assert np.array_equal(cnt, count)
    keep = np.arange(n_win) != low
    assert mean.shape == (1, n_win, wy, wx) and mean[0, keep].tobytes() == planes[keep].tobytes(), "mean planes: the bits of sum / count"
    assert np.all(np.isnan(mean[0, low])) and np.isnan(u.ravel()[low]) and np.isnan(v.ravel()[low])
    ref_u, ref_v = pk.reference(mean[0])
    assert np.all(np.isfinite(ref_u[keep])) and np.all(np.isfinite(ref_v[keep]))
    worst = pk.assert_within_gate(u, v, ref_u, ref_v, window, f"imported state {window}")
    print(f"imported state {window}: worst relative error {worst:.3e}, stats {st}")
    # no frames were used: every flagged window is still reported as left without a re-evaluation from the frames
    assert st["flagged"] > 0 and st["rescued"] == 0 and st["float32_kept"] == st["flagged"], st
    with options(rescue=0):                               # the bare float32 fits, and the windows nobody flagged have their bits
        e = piv.Ensemble((rows * wy, cols * wx), window, (0, 0))
        try:
            e.import_state(sums, count)
            u0, v0, _ = e.finish(count_min, n_frames)
            assert e.stats()["flagged"] == 0
        finally:
            e.close()
    differ = (u.view(np.uint32) != u0.view(np.uint32)) | (v.view(np.uint32) != v0.view(np.uint32))
    assert differ.sum() <= st["flagged"]


def test_plane_volume_path_has_the_bits_of_the_fused_path(gpu):
    """cross_corr -> u_v_displacement against piv_pairs on the windows the fused kernel did not flag: the re-fit of the plane-volume call
    uses the fused kernels' criterion, so it touches flagged windows only."""
    frames = particle_stack(4, 96, 128, seed=11)
    ws, ov = (32, 32), (16, 16)
    u, v, _, _ = piv.piv_pairs(frames, ws, ov)
    fit, amb = rescue_lists()
    x, y, planes = piv.cross_corr(frames, window_size=ws, overlap=ov)
    u2, v2 = piv.u_v_displacement(planes, u.shape[1], u.shape[2])
    flagged = np.zeros(u.size, bool)
    flagged[fit[:, 0].astype(np.int64)] = True
    flagged[amb.astype(np.int64)] = True
    free = ~flagged.reshape(u.shape)
    assert free.sum() > u.size // 2
    assert u2[free].tobytes() == u[free].tobytes() and v2[free].tobytes() == v[free].tobytes()
