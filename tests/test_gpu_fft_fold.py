"""Folded twiddles of the register FFTs (csrc/fft_regs.h, LSPIV_FFT_FOLD): the twiddle scale rides on the first add / sub level of the
next butterfly instead of being multiplied in.  That is another rounding sequence, so this file holds what the parity contract rests on:

* the transforms of 16, 32, 64 in both forms on one library (lspiv_debug_fft_form) against numpy.fft in complex128 -- the folded form
  may be no worse than 1.5 x the un-folded one, which is the yardstick (the max over ~1e5 samples moves by +- 7 % between two forms);
* the float32 planes of the walking kernels against float64 planes computed here: worst |error| / plane maximum <= 4.2e-7, the recorded
  figure the rescue flag's kappa was set against;
* u, v, corr, s2n with the rescue pass on against the C oracle at the suite's 1e-4 on every window but the oracle's exact float64 ties;
* one launch and two launches cut on the chunk alignment give the same bits.

Stacks: 27 frames = 26 pairs, so that every run crosses the segment anchor at pair 25; the smallest frames that still hold a few windows.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from oracle import piv_oracle as po
from pyorc_amd.synth import particle_stack

TOL = 1e-4
PLANE_NOISE = 4.2e-7     # what a float32 plane carries, relative to its maximum
TIE_CAP = 0.01
T_FRAMES = 27
# window -> (overlap, (H, W), seed): seeds chosen so that the ORACLE alone reports <= 1 % exact ties (test_reference_is_clean)
SHAPES = {16: (8, (48, 64), 1601), 32: (16, (64, 96), 3201), 64: (48, (128, 160), 6401)}
CASES = [(n, dt) for n in SHAPES for dt in ("u8", "f32")]


@functools.lru_cache(maxsize=None)
def stack(n, dt):
    ov, (H, W), seed = SHAPES[n]
    fr = particle_stack(T_FRAMES, H, W, seed=seed, density=0.05)
    fr = fr if dt == "u8" else fr.astype(np.float32)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def ref_planes(n):
    """float64 planes (P, n_win, n, n) of the stack, in numpy: the oracle's normalisation ((a - mean) / std, population std, 0 where
    std == 0), its clip of the negative lobes, the circular cross-correlation by float64 FFTs, fft-shifted, / n^2, clipped to [0, 1].
    The uint8 stack and its float32 copy hold the same values, so one reference serves both."""
    ov, (H, W), _ = SHAPES[n]
    fr = stack(n, "u8").astype(np.float64)
    y0, x0 = po.window_origins((H, W), (n, n), (ov, ov))
    iy = y0[:, None] + np.arange(n)[None, :]
    ix = x0[:, None] + np.arange(n)[None, :]
    win = fr[:, iy[:, None, :, None], ix[None, :, None, :]].reshape(T_FRAMES, len(y0) * len(x0), n, n)
    off = win - win.mean(axis=(-2, -1), keepdims=True)
    std = np.sqrt((off * off).mean(axis=(-2, -1), keepdims=True))
    w = np.maximum(np.divide(off, std, out=np.zeros_like(off), where=std != 0), 0.0)
    f = np.fft.fft2(w)
    c = np.fft.ifft2(np.conj(f[:-1]) * f[1:]).real
    c = np.clip(np.fft.fftshift(c, axes=(-2, -1)) / float(n * n), 0.0, 1.0)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(n, dt):
    ov = SHAPES[n][0]
    return c_oracle.piv_pairs(stack(n, dt), (n, n), (ov, ov), return_planes=True, return_cond=True)


@functools.lru_cache(maxsize=None)
def gpu_run(n, dt):
    """(u, v, corr, s2n, planes) of the whole stack, resident in HBM, one launch (lspiv_piv_pairs_dev_at at offset 0, rescue on)."""
    import pyorc_amd
    from pyorc_amd.device import DeviceFrames

    ov = SHAPES[n][0]
    return pyorc_amd.piv_pairs(DeviceFrames.from_host(np.ascontiguousarray(stack(n, dt))), (n, n), (ov, ov), return_planes=True)


def rel_err(got, ref, floor=0.05):
    with np.errstate(all="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(np.abs(ref), floor)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


# ---------------------------------------------------------------------------------------------- the reference itself (no GPU)
@pytest.mark.parametrize("n", list(SHAPES))
def test_reference_is_clean(n):
    """The float64 planes built here are the oracle's (two float64 FFT routes: ~1e-15), the stacks hold several windows and cross the
    anchor, and the oracle alone sets aside at most 1 % of the windows as exact ties."""
    from pyorc_amd import window

    ov, shape, _ = SHAPES[n]
    ref = ref_planes(n)
    assert ref.shape[0] == 26 and ref.shape[1] >= 6
    assert window.chunk_alignment((n, n), shape, (ov, ov)) == 25
    for dt in ("u8", "f32"):
        uo, vo, cmo, sno, planes, cond = oracle(n, dt)
        d = float(np.abs(planes - ref).max())
        tie = c_oracle.exact_tie(cond, cmo)
        print(f"n={n} {dt}: {ref.shape[1]} windows, |oracle - numpy| planes {d:.2e}, ties {tie.mean():.4f}, non-zero planes "
              f"{(ref.max(axis=(-2, -1)) > 0).mean():.3f}")
        assert d <= 1e-12
        assert tie.mean() <= TIE_CAP


# ---------------------------------------------------------------------------------------------- twiddle rows
def _rows(n):
    rng = np.random.default_rng(20260927 + n)
    z = np.zeros((n + 1 + 4096, n), np.complex128)
    z[np.arange(n), np.arange(n)] = 1.0          # the n unit impulses: row j is the twiddle row of input j
    z[n] = 1.0                                   # a constant row
    z[n + 1:] = rng.uniform(-1, 1, (4096, n)) + 1j * rng.uniform(-1, 1, (4096, n))
    return z.astype(np.complex64)


def _fft_form(lib, z, form, inverse):
    from pyorc_amd import _lib

    zin = np.ascontiguousarray(z)
    out = np.empty_like(zin)
    _lib.check(lib.lspiv_debug_fft_form(z.shape[1], form, inverse, _lib.ptr(zin), _lib.ptr(out), z.shape[0]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_folded_rows_no_worse_than_unfolded(gpu, n, inverse):
    from pyorc_amd import _lib

    z = _rows(n)
    z128 = z.astype(np.complex128)
    ref = np.fft.ifft(z128, axis=1) * n if inverse else np.fft.fft(z128, axis=1)
    scale = np.abs(ref).max(axis=1, keepdims=True)
    fig = {}
    for form in (1, 2):
        e = np.abs(_fft_form(gpu, z, form, inverse).astype(np.complex128) - ref) / scale
        fig[form] = (float(e.max()), float(np.sqrt((e * e).mean())))
    print(f"n={n} inverse={inverse}: un-folded max {fig[1][0]:.3e} rms {fig[1][1]:.3e}; folded max {fig[2][0]:.3e} rms {fig[2][1]:.3e}")
    assert fig[2][0] <= 1.5 * fig[1][0]
    assert fig[2][1] <= 1.5 * fig[1][1]
    own = _fft_form(gpu, z, 0, inverse)            # the kernels' transform is one of the two, bit for bit, and the old hook is form 0
    assert any(np.array_equal(own, _fft_form(gpu, z, form, inverse)) for form in (1, 2))
    old = np.empty_like(z)
    _lib.check(gpu.lspiv_debug_fft(n, inverse, _lib.ptr(z), _lib.ptr(old), z.shape[0]))
    assert np.array_equal(old, own)


@pytest.mark.gpu
def test_form_hook_rejects_what_it_does_not_have(gpu):
    from pyorc_amd import _lib

    z = np.zeros((1, 24), np.complex64)
    out = np.empty_like(z)
    assert gpu.lspiv_debug_fft_form(24, 0, 0, _lib.ptr(z), _lib.ptr(out), 1) == _lib.LSPIV_OK          # a prime-factor length: form 0 only
    assert gpu.lspiv_debug_fft_form(24, 2, 0, _lib.ptr(z), _lib.ptr(out), 1) == _lib.LSPIV_EUNSUPPORTED
    assert gpu.lspiv_debug_fft_form(32, 3, 0, _lib.ptr(z), _lib.ptr(out), 1) == _lib.LSPIV_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------- planes and results
@pytest.mark.gpu
@pytest.mark.parametrize("n,dt", CASES)
def test_plane_noise(gpu, n, dt):
    planes = gpu_run(n, dt)[4]
    ref = ref_planes(n)
    assert planes.shape == ref.shape and np.isfinite(planes).all()
    top = ref.max(axis=(-2, -1))
    live = top > 0
    assert live.mean() > 0.9
    err = np.abs(planes.astype(np.float64) - ref).max(axis=(-2, -1))[live] / top[live]
    print(f"n={n} {dt}: worst |error| / plane maximum {err.max():.3e} over {live.sum()} planes (median {np.median(err):.3e})")
    assert err.max() <= PLANE_NOISE


@pytest.mark.gpu
@pytest.mark.parametrize("n,dt", CASES)
def test_results_against_oracle(gpu, n, dt):
    u, v, cm, sn, _ = gpu_run(n, dt)
    uo, vo, cmo, sno, _, cond = oracle(n, dt)
    tie = c_oracle.exact_tie(cond, cmo)
    assert tie.mean() <= TIE_CAP
    ok = ~tie
    for name, g, r in (("u", u, uo), ("v", v, vo)):
        assert np.array_equal(np.isnan(g)[ok], np.isnan(r)[ok]), f"{name}: NaN mask differs"
    for name, g, r in (("corr", cm, cmo), ("s2n", sn, sno)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{name}: NaN mask differs"
    errs = {"u": rel_err(u[ok], uo[ok].astype(np.float64)), "v": rel_err(v[ok], vo[ok].astype(np.float64)),
            "corr": rel_err(cm, cmo.astype(np.float64)), "s2n": rel_err(sn, sno.astype(np.float64))}
    print(f"n={n} {dt}: {errs}, {int(tie.sum())} of {tie.size} windows are exact ties")
    for name, e in errs.items():
        assert e <= TOL, f"{name}: {e:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_two_launches_cut_on_the_anchor_give_the_same_bits(gpu, dt):
    import pyorc_amd
    from pyorc_amd import window
    from pyorc_amd.device import DeviceFrames

    n, (ov, shape, _) = 32, SHAPES[32]
    A = window.chunk_alignment((n, n), shape, (ov, ov))
    assert 0 < A < T_FRAMES - 1
    fr = stack(n, dt)
    whole = gpu_run(n, dt)
    parts = [pyorc_amd.piv_pairs(DeviceFrames.from_host(np.ascontiguousarray(fr[a:b + 1])), (n, n), (ov, ov), return_planes=True, pair_offset=a)
             for a, b in ((0, A), (A, T_FRAMES - 1))]
    for k, name in enumerate(("u", "v", "corr", "s2n", "planes")):
        got = np.concatenate([p[k] for p in parts], axis=0)
        assert np.array_equal(got.view(np.uint32), whole[k].view(np.uint32)), name
