"""Conjugate-pair split-radix register FFTs (csrc/fft_regs.h, fft_sr / LSPIV_FFT_SR; form 4 of lspiv_debug_fft_form) on the GPU.  Another
operation order is another rounding sequence, so this file holds for the new form what tests/test_gpu_fft_fold.py holds for the folded one,
with that file's stacks, references and bounds (imported, not copied):

* the transforms of 16, 32, 64, forward and inverse, on 4 096 random rows, every unit impulse and a constant row against numpy.fft in
  complex128, all three forms in one run: the split-radix form may be no worse than 1.5 x the un-folded one (max and rms of the error
  relative to the row's largest bin) -- the yardstick and the factor of the fold test;
* the walking 32 x 32 kernel, which runs on the split-radix form (kFftSrWalk32), on 26 pairs of a 64 x 96 frame -- the smallest frame with a
  full window grid and both segment kinds: float32 planes against float64 planes within 4.2e-7 of the plane maximum (DESIGN.md section
  3.6), u, v, corr, s2n against the C oracle at 1e-4, every output of the clamped inverse inside [0, 1], a zero-variance pair's plane
  exactly zero;
* 100 pairs of the same frame size, past the anchors at 25, 50 and 75: one launch, two launches cut at 25 and three cut at 25 and 75 give
  the same bits.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from pyorc_amd.synth import particle_stack
from tests.test_gpu_fft_fold import PLANE_NOISE, SHAPES, TIE_CAP, TOL, _fft_form, _rows, gpu_run, oracle, ref_planes, rel_err

FACTOR = 1.5     # tests/test_gpu_fft_fold.py: test_folded_rows_no_worse_than_unfolded
FORMS = ((1, "un-folded"), (2, "folded"), (4, "split radix"))
N = 32
OV, SHAPE, _ = SHAPES[N]


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_split_radix_rows(gpu, n, inverse):
    z = _rows(n)
    z128 = z.astype(np.complex128)
    ref = np.fft.ifft(z128, axis=1) * n if inverse else np.fft.fft(z128, axis=1)
    scale = np.abs(ref).max(axis=1, keepdims=True)
    fig, out = {}, {}
    for form, _ in FORMS:
        out[form] = _fft_form(gpu, z, form, inverse)
        e = np.abs(out[form].astype(np.complex128) - ref) / scale
        fig[form] = (float(e.max()), float(np.sqrt((e * e).mean())))
    print(f"n={n} inverse={inverse}: " + "; ".join(f"{name} max {fig[f][0]:.3e} rms {fig[f][1]:.3e}" for f, name in FORMS))
    assert fig[4][0] <= FACTOR * fig[1][0]
    assert fig[4][1] <= FACTOR * fig[1][1]
    own = _fft_form(gpu, z, 0, inverse)          # what the kernels of the length run is one of the three, bit for bit
    assert any(np.array_equal(own, out[form]) for form, _ in FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_walking_32_plane_noise(gpu, dt):
    planes = gpu_run(N, dt)[4]
    ref = ref_planes(N)
    assert planes.shape == ref.shape and ref.shape[0] == 26 and np.isfinite(planes).all()
    top = ref.max(axis=(-2, -1))
    live = top > 0
    assert live.mean() > 0.9
    err = np.abs(planes.astype(np.float64) - ref).max(axis=(-2, -1))[live] / top[live]
    print(f"n={N} {dt}: worst |error| / plane maximum {err.max():.3e} over {live.sum()} planes (median {np.median(err):.3e})")
    assert err.max() <= PLANE_NOISE


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_walking_32_against_oracle(gpu, dt):
    u, v, cm, sn, _ = gpu_run(N, dt)
    uo, vo, cmo, sno, _, cond = oracle(N, dt)
    tie = c_oracle.exact_tie(cond, cmo)
    assert tie.mean() <= TIE_CAP
    ok = ~tie
    for name, g, r in (("u", u, uo), ("v", v, vo)):
        assert np.array_equal(np.isnan(g)[ok], np.isnan(r)[ok]), f"{name}: NaN mask differs"
    for name, g, r in (("corr", cm, cmo), ("s2n", sn, sno)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{name}: NaN mask differs"
    errs = {"u": rel_err(u[ok], uo[ok].astype(np.float64)), "v": rel_err(v[ok], vo[ok].astype(np.float64)),
            "corr": rel_err(cm, cmo.astype(np.float64)), "s2n": rel_err(sn, sno.astype(np.float64))}
    print(f"n={N} {dt}: {errs}, {int(tie.sum())} of {tie.size} windows are exact ties")
    for name, e in errs.items():
        assert e <= TOL, f"{name}: {e:.3e}"


@functools.lru_cache(maxsize=None)
def long_stack(dt):
    fr = particle_stack(101, *SHAPE, seed=3202, density=0.05)
    fr = fr if dt == "u8" else fr.astype(np.float32)
    fr.setflags(write=False)
    return fr


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_chunkings_on_the_anchors_give_the_same_bits(gpu, dt):
    import pyorc_amd
    from pyorc_amd import window
    from pyorc_amd.device import DeviceFrames

    assert window.chunk_alignment((N, N), SHAPE, (OV, OV)) == 25
    fr = long_stack(dt)
    P = fr.shape[0] - 1

    def run(bounds):
        parts = [pyorc_amd.piv_pairs(DeviceFrames.from_host(np.ascontiguousarray(fr[a:b + 1])), (N, N), (OV, OV), return_planes=True, pair_offset=a)
                 for a, b in zip(bounds[:-1], bounds[1:])]
        return [np.concatenate([p[k] for p in parts], axis=0) for k in range(5)]

    whole = run([0, P])
    assert np.isfinite(whole[4]).all() and (whole[4].max(axis=(-2, -1)) > 0).mean() > 0.9
    for bounds in ([0, 25, P], [0, 25, 75, P]):
        got = run(bounds)
        for k, name in enumerate(("u", "v", "corr", "s2n", "planes")):
            assert np.array_equal(got[k].view(np.uint32), whole[k].view(np.uint32)), f"{name}: cut at {bounds[1:-1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_clamped_inverse(gpu, dt):
    """The clip rides on the last FMA / add / sub of the last inverse transform (clamp modifier): nothing leaves [0, 1]; and a pair with a
    zero-variance window, whose plane shares that transform with its neighbour's, still comes out exactly zero (corr 0, the rest NaN)."""
    import pyorc_amd
    from pyorc_amd.device import DeviceFrames

    planes = gpu_run(N, dt)[4]
    assert planes.min() >= 0.0 and planes.max() <= 1.0
    fr = np.array(long_stack(dt)[:8])
    fr[3, :N, :N] = 7                                              # window (0, 0) of frame 3 is flat: pairs 2 and 3 have no variance there
    u, v, cm, sn, pl = pyorc_amd.piv_pairs(DeviceFrames.from_host(fr), (N, N), (OV, OV), return_planes=True)
    n_cols = u.shape[2]
    pl = pl.reshape(u.shape[0], -1, N, N)
    for p in (2, 3):
        assert not pl[p, 0].any(), f"pair {p}: the plane of the flat window is not exactly zero"
        assert cm[p, 0, 0] == 0.0 and np.isnan(u[p, 0, 0]) and np.isnan(v[p, 0, 0]) and np.isnan(sn[p, 0, 0])
    for p in (1, 4):                                               # its neighbours in time are untouched by it
        assert pl[p, 0].max() > 0 and pl[p, 0].min() >= 0.0 and pl[p, 0].max() <= 1.0
    assert n_cols >= 2 and pl[2, 1].max() > 0
