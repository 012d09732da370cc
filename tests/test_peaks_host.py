"""CPU side of the plane-volume peak tests (tests/peaks_inputs.py has the planes, tests/test_gpu_peaks_planes.py the GPU side): what has
to hold of the INPUTS for the GPU gate to mean something, shown with a float32 numpy restatement of the kernel's fit.

The restatement (``fit_f32``) is csrc/piv_direct.hip ``peaks_kernel`` / ``subpixel_generic`` operation by operation in float32:
``x + kEpsPeak`` with the constant rounded to float32, ``log2`` (numpy's float32 one, at least as good as the hardware's), common.h
``gauss_offset_fast`` (nom = lm - lp, den = 2 lm - 4 l0 + 2 lp, nom * (1 / den) with the reciprocal rounded on its own), and
``(float)i + off - (float)(wy / 2)`` as two rounded operations; ``flag_f32`` is common.h ``peak_cond`` with ``near_tie = false`` at the
library's default ``rescue_kappa`` (500, in 1e-9 of the plane maximum: k = 2 kappa 1e-9 / (ln 2 * 1e-4)).

Measured here (numpy 2.x float32 log2; the GPU's figures are in tests/test_gpu_peaks_planes.py):

* np.argmax and "first NaN, else first maximum" over the float32 samples agree on every plane of the three families -- 397 "argmax"
  planes, 19 614 "fit" planes, 70 000 "many" planes: nothing is set aside.
* every "fit" plane has its arg-max in the interior.
* "fit" planes outside the gate (1e-4 of max(|ref|, 0.05 px)) under the float32 restatement, against the float64 fit of the same
  samples: 0 of 3 946 at 16 x 16 (sigma <= 3 only), 560 of 7 834 (7.2 %) at 33 x 33, 568 of 7 834 (7.3 %) at 64 x 64 -- 1 128 of 19 614 =
  5.75 % of the family, worst 1.96e-3 (sigma 12, h 1e-6).  With the 3 x 81 centres over [-0.5, 0.5]^2 alone the share was 3.1 %: the
  family was widened by 81 centres within 0.04 px of the plane centre, where the gate is an absolute 5e-6 px.  By row: sigma <= 3 none;
  sigma 5: 23 % at h 1e-6; sigma 8: 13 % at h 0.02, 42 - 44 % at 1e-6; sigma 12: 7 - 10 % at (0.3, 0.2), 22 % at 0.02, 63 - 65 % at 1e-6.
* the restated ``peak_cond`` flags 890 / 4 658 / 4 658 planes (22.6 % / 59.5 % / 59.5 %) and EVERY plane outside the gate; the worst
  plane it does not flag is at 3.2e-5 / 3.2e-5 / 4.7e-5.  The existing criterion can drive a float64 re-fit of the five samples."""
import functools

import numpy as np
import pytest

from tests import peaks_inputs as pk

F = np.float32
EPS = F(1e-7)                       # kEpsPeak
KAPPA_DEFAULT = 500                 # api_core.hip, g_opt_rescue_kappa
K_DEFAULT = F(2.0 * KAPPA_DEFAULT * 1e-9 / (0.6931471805599453 * 1e-4))


def argmax_nan_first(flat):
    """Flat arg-max per row of (k, n) float32: the first NaN if there is one, else the first maximum (-0.0 == +0.0)."""
    nan = np.isnan(flat)
    has = nan.any(axis=1)
    first_nan = nan.argmax(axis=1)
    with np.errstate(invalid="ignore"):
        mx = np.where(nan, -np.inf, flat).max(axis=1)
        first_max = (np.where(nan, -np.inf, flat) == mx[:, None]).argmax(axis=1)
    return np.where(has, first_nan, first_max)


def _log2(x):
    with np.errstate(all="ignore"):
        return np.log2(x.astype(F)).astype(F)


def _offset(lm, l0, lp):
    """gauss_offset_fast: (offset, den), float32 operation by operation."""
    with np.errstate(all="ignore"):
        nom = (lm - lp).astype(F)
        den = ((F(2.0) * lm - F(4.0) * l0).astype(F) + F(2.0) * lp).astype(F)
        rcp = (F(1.0) / den).astype(F)
        off = np.where(den != 0, (nom * rcp).astype(F), F(0.0)).astype(F)
    return off, den


def fit_f32(planes):
    """The kernel's float32 fit of (k, wy, wx) float32 planes whose arg-max is interior: u, v, and the terms peak_cond reads."""
    k, wy, wx = planes.shape
    flat = planes.reshape(k, -1)
    idx = argmax_nan_first(flat)
    i, j = idx // wx, idx % wx
    assert np.all((i > 0) & (i < wy - 1) & (j > 0) & (j < wx - 1))
    r = np.arange(k)
    with np.errstate(all="ignore"):
        vmax = planes[r, i, j]
        cl, cr = (planes[r, i - 1, j] + EPS).astype(F), (planes[r, i + 1, j] + EPS).astype(F)
        cd, cu = (planes[r, i, j - 1] + EPS).astype(F), (planes[r, i, j + 1] + EPS).astype(F)
        l0 = _log2((vmax + EPS).astype(F))
        off_v, den_v = _offset(_log2(cl), l0, _log2(cr))
        off_u, den_u = _offset(_log2(cd), l0, _log2(cu))
        v = ((i.astype(F) + off_v).astype(F) - F(wy // 2)).astype(F)
        u = ((j.astype(F) + off_u).astype(F) - F(wx // 2)).astype(F)
    return u, v, dict(vmax=vmax, cl=cl, cr=cr, cd=cd, cu=cu, den_v=den_v, den_u=den_u)


def flag_f32(u, v, t, k=K_DEFAULT):
    """common.h peak_cond(...).fit with near_tie = false, border = false."""
    with np.errstate(all="ignore"):
        def bad(c_a, c_b, den, res):
            cm = np.minimum(c_a, c_b)
            a = (k * (F(2.0) * t["vmax"].astype(np.float64) + cm).astype(F)).astype(F)
            rhs = ((np.maximum(np.abs(res), F(0.05)) * np.abs(den)).astype(F) * cm).astype(F)
            rhs = np.where(np.isnan(res), F(np.nan), rhs)     # max_abs keeps a NaN
            return ~(a <= rhs)
        return (t["vmax"] > 0) & (bad(t["cl"], t["cr"], t["den_v"], v) | bad(t["cd"], t["cu"], t["den_u"], u))


def all_volumes():
    for shape in pk.ARGMAX_SHAPES:
        yield f"argmax{shape}", pk.argmax_family(shape).planes
    for n in pk.FIT_SIZES:
        yield f"fit{n}", pk.fit_family(n).planes
    yield "many", pk.many_family()


def test_families_hold_what_the_issue_lists():
    assert pk.ARGMAX_SHAPES[0] == (1, 9) and pk.ARGMAX_SHAPES[-1] == (130, 257) and len(pk.ARGMAX_SHAPES) == 14
    wy, wx = 130, 257
    big = pk.argmax_family((wy, wx))
    single = {int(np.argmax(p)) for p, l in zip(big.planes, big.labels) if l.startswith("max-")}    # (two names for one spot: one plane)
    assert single == {0, wx - 1, (wy - 1) * wx, wy * wx - 1, wx // 2, (wy - 1) * wx + wx // 2, (wy // 2) * wx, (wy // 2) * wx + wx - 1,
                      wx + 1, (wy - 2) * wx + wx - 2, (wy // 2) * wx + wx // 2, 63, 64, 65, 127, 128}
    for want in ("nan-after-max", "nan-before-max", "all-nan", "inf-nan-inf", "nan-inf-nan", "all-minus-inf", "all-zero", "all-0.37",
                 "signed-zeros-minus-first", "signed-zeros-plus-first", "negative-max", "negative-neighbour-u", "negative-neighbour-v"):
        assert want in big.labels, want
    for step in ("1", "63", "64", "128", "last"):
        ties = [l for l in big.labels if l.startswith(f"tie-{step}-")]
        assert len(ties) == (1 if step == "last" else 2), (step, ties)     # p interior / q border, and the other way round
    for shape in pk.ARGMAX_SHAPES:
        fam = pk.argmax_family(shape)
        assert fam.planes.dtype == np.float32 and fam.planes.shape[1:] == shape and len(fam.labels) == len(fam.planes)
        assert len(set(fam.labels)) == len(fam.labels)
    for n in pk.FIT_SIZES:
        f = pk.fit_family(n)
        n_sig = 3 if n == 16 else 6
        assert (f.kind == "gauss").sum() == n_sig * 4 * 324
        assert all((f.kind == k).sum() == 18 for k in ("clip1", "clip2", "clip4")) and (f.kind == "row3").sum() == 4
        c = n // 2
        for kind, zeros in (("clip1", 1), ("clip2", 2), ("clip4", 4)):
            p = f.planes[f.kind == kind]
            nb = np.stack([p[:, c - 1, c], p[:, c + 1, c], p[:, c, c - 1], p[:, c, c + 1]], axis=1)
            assert np.all((nb == 0).sum(axis=1) == zeros) and np.all(p[:, c, c] > 0)
    m = pk.many_family()
    assert m.shape == (pk.MANY, 4, 4) and pk.MANY > 65535


def test_argmax_agrees_with_numpy_on_every_plane():
    total = 0
    for name, planes in all_volumes():
        flat = planes.reshape(len(planes), -1)
        assert np.array_equal(np.argmax(flat, axis=1), argmax_nan_first(flat)), name
        total += len(planes)
    print(f"planes: {total}")
    # the finding the kernel is held to: the first NaN wins over an earlier inf
    assert np.argmax(np.array([1, np.inf, np.nan, np.inf], F)) == 2 == argmax_nan_first(np.array([[1, np.inf, np.nan, np.inf]], F))[0]


def test_reference_picks_the_planted_sample():
    for shape in pk.ARGMAX_SHAPES:
        fam = pk.argmax_family(shape)
        wy, wx = shape
        idx = np.argmax(fam.planes.reshape(len(fam.planes), -1), axis=1)
        u2, v2 = pk.argmax_reference(shape, border_peak=2)
        for k, label in enumerate(fam.labels):
            if label.startswith("tie-"):
                p = int(label.split("-p")[1].split("-")[0])
                assert idx[k] == p, (shape, label)
            if label in ("inf-nan-inf", "nan-after-max", "nan-inf-nan", "nan-before-max", "all-nan"):
                assert np.isnan(fam.planes[k].ravel()[idx[k]]) and np.isnan(u2[k]) and np.isnan(v2[k]), (shape, label)
            if label in ("all-minus-inf", "all-zero", "all-0.37") or label.startswith("signed-zeros"):
                assert idx[k] == 0 and u2[k] == -(wx // 2) and v2[k] == -(wy // 2), (shape, label)
            if label == "negative-max":
                assert np.isnan(u2[k]) and np.isnan(v2[k])
            if label == "negative-neighbour-u":
                assert np.isnan(u2[k]) and np.isfinite(v2[k])
            if label == "negative-neighbour-v":
                assert np.isfinite(u2[k]) and np.isnan(v2[k])


@functools.lru_cache(maxsize=None)
def fit_stats(n):
    """(outside the gate, flagged, worst relative error) per plane of the size-n "fit" planes under the float32 restatement."""
    f = pk.fit_family(n)
    ru, rv = pk.fit_reference(n)
    assert np.all(np.isfinite(ru)) and np.all(np.isfinite(rv)), "a fit plane whose arg-max is on the border or whose fit is NaN"
    u, v, terms = fit_f32(f.planes)          # asserts the interior arg-max
    miss = (np.abs(u - ru) > pk.bound(ru, n)) | (np.abs(v - rv) > pk.bound(rv, n))
    rel = np.maximum(pk.rel_error(u, ru), pk.rel_error(v, rv))
    return miss, flag_f32(u, v, terms), rel


def test_fit_family_reaches_the_finding():
    miss = np.concatenate([fit_stats(n)[0] for n in pk.FIT_SIZES])
    print(f"fit family: {miss.size} planes, {miss.sum()} outside the gate in float32 ({miss.mean():.4f})")
    assert miss.mean() >= 0.05, "fewer than 5 % of the fit planes exceed the gate in float32: the family does not reach the finding"


@pytest.mark.parametrize("n", pk.FIT_SIZES)
def test_every_miss_is_flagged(n):
    f = pk.fit_family(n)
    miss, flagged, rel = fit_stats(n)
    print(f"fit {n}: {len(miss)} planes, outside the gate {miss.sum()} ({miss.mean():.4f}), flagged {flagged.sum()} ({flagged.mean():.4f}), "
          f"worst relative error {rel.max():.3e}, worst unflagged {rel[~flagged].max():.3e}")
    for sigma in sorted(set(f.sigma[f.kind == "gauss"])):
        for h, _ in pk.HEIGHTS:
            sel = (f.kind == "gauss") & (f.sigma == sigma) & (f.h == h)
            print(f"  sigma {sigma:4.1f} h {h:7.0e}: worst {rel[sel].max():.2e}, outside {miss[sel].mean():.3f}, flagged {flagged[sel].mean():.3f}, "
                  f"worst unflagged {rel[sel & ~flagged].max() if (sel & ~flagged).any() else 0.0:.2e}")
    for kind in ("clip1", "clip2", "clip4", "row3"):
        sel = f.kind == kind
        print(f"  {kind}: worst {rel[sel].max():.2e}, outside {miss[sel].mean():.3f}, flagged {flagged[sel].mean():.3f}")
    unflagged_miss = np.nonzero(miss & ~flagged)[0]
    assert unflagged_miss.size == 0, (f"{unflagged_miss.size} planes miss the gate in float32 and are not flagged by peak_cond at kappa "
                                      f"{KAPPA_DEFAULT}: first {unflagged_miss[:8].tolist()}, worst {rel[unflagged_miss].max():.3e}")


def test_many_family_is_interior_and_well_inside_the_gate():
    p = pk.many_family()
    ru, rv = pk.many_reference()
    assert np.all(np.isfinite(ru)) and np.all(np.isfinite(rv))
    u, v, _ = fit_f32(p)
    assert np.all(np.abs(u - ru) <= pk.bound(ru, 4)) and np.all(np.abs(v - rv) <= pk.bound(rv, 4))
