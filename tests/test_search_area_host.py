"""Extended search area, host side: the reference against the oracle at S == n, argument validation, the grid and the planner follow
the search area, and the CPU check of the inputs the GPU tests rely on (tie shares, the fast-flow case)."""
import numpy as np
import pytest

from oracle import piv_oracle as po
from pyorc_amd import piv, velocimetry, window
from pyorc_amd.synth import particle_stack
from tests import search_area_ref as ref

# (n, S, H, W, overlap, seed, density): odd window counts; widths 3 S + 5 that are no multiple of 4; overlaps 0 and S / 2.  Seeds and
# densities are those for which the REFERENCE has no tie for a plane maximum (checked below on the CPU, cap 1 %): scanned over seeds
# seed, seed + 20, seed + 40 and densities 0.04 ... 0.4 of pyorc_amd.synth.particle_stack.  4 in 16 has none there: a 4 x 4 window is
# smaller than one of that generator's particles, its plane saturates at the clip (>= 15 % ties at every seed and density tried), so
# that case draws finer particles (fine_particles: sigma 0.6 px, density 0.3, seed 0)
CASES = [(4, 16, 36, 53, 8, 0, 0.3), (8, 16, 48, 56, 0, 44, 0.1), (14, 16, 36, 50, 8, 5, 0.04), (16, 32, 70, 101, 16, 6, 0.04),
         (24, 32, 96, 96, 0, 7, 0.04), (30, 32, 70, 100, 16, 8, 0.04), (24, 64, 130, 200, 32, 9, 0.04), (32, 64, 192, 192, 0, 10, 0.04),
         (62, 64, 130, 197, 32, 11, 0.04)]


def fine_particles(T, H, W, seed, density, sigma=0.6, shift=(1.3, -0.8)):
    """Synthetic particles finer than particle_stack's (Gaussian blobs of `sigma` px), uniformly shifted: uint8 (T, H, W)."""
    rng = np.random.default_rng(seed)
    k = int(density * H * W)
    py, px, amp = rng.uniform(-4, H + 4, k), rng.uniform(-4, W + 4, k), rng.uniform(100, 255, k)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((T, H, W), np.uint8)
    for t in range(T):
        img = np.zeros((H, W))
        for q in range(k):
            y0, x0 = int(round(py[q])), int(round(px[q]))
            ys, xs = slice(max(y0 - 3, 0), min(y0 + 4, H)), slice(max(x0 - 3, 0), min(x0 + 4, W))
            img[ys, xs] += amp[q] * np.exp(-((yy[ys, xs] - py[q]) ** 2 + (xx[ys, xs] - px[q]) ** 2) / (2 * sigma ** 2))
        out[t] = np.clip(np.rint(img), 0, 255)
        px, py = px + shift[0], py + shift[1]
    return out


def fast_stack():
    """The fast-flow input: H = W = 160, a uniform shift of (+10, -9) px per frame; for n = 12, S = 32, overlap 16.  Density and particle
    size are those at which the REFERENCE meets the three conditions (test below): particle_stack's particles (a few px across, so
    that a 12 x 12 window truncates most of them) leave the median error at 0.10 - 0.13 px and 70 - 84 % of the windows within 0.5 px
    at densities 0.06 ... 0.2, finer and denser particles (sigma 0.8 px, density 0.2, seed 22) give 0.045 / 0.034 px and 97.5 %."""
    return fine_particles(2, 160, 160, 22, 0.2, sigma=0.8, shift=(10.0, -9.0))


def case_stack(n, S, H, W, ov, seed, density, T=4, dtype=np.uint8):
    a = fine_particles(T, H, W, seed, density) if n == 4 else particle_stack(T, H, W, seed=seed, density=density)
    return a if dtype == np.uint8 else a.astype(dtype) * dtype(0.37) - dtype(11.0)   # (an affine map: the same normalised windows)


def test_reference_equals_oracle_when_search_area_is_the_window():
    a = particle_stack(3, 70, 90, seed=2, density=0.05)
    for n, ov in ((16, 8), (32, 16)):
        _, _, planes = ref.search_planes(a, (n, n), (n, n), (ov, ov), signal_threshold=0.05)
        _, _, oracle = po.cross_corr(a, (n, n), (ov, ov), signal_threshold=0.05)
        assert np.array_equal(planes, oracle, equal_nan=True)


def test_window_counts_are_odd_and_reference_ties_are_rare():
    for n, S, H, W, ov, seed, density in CASES:
        x, y = po.get_rect_coordinates((H, W), (n, n), (ov, ov), search_area_size=(S, S))
        assert (len(x) * len(y)) % 2 == 1, (n, S)
        r = ref.search_piv(case_stack(n, S, H, W, ov, seed, density), (n, n), (S, S), (ov, ov))
        assert r["tie"].mean() <= 0.01, (n, S, float(r["tie"].mean()))


def test_argument_validation(lib):
    for sa, ws in (((48, 48), (16, 16)), ((32, 64), (16, 16)), ((32, 32), (15, 15)), ((32, 32), (32, 30)), ((16, 16), (2, 2)),
                   ((32, 32), (16, 12)), ((16, 16), (32, 32))):
        with pytest.raises(ValueError, match="16, 32, 64.*4 <= window <= search area - 2"):
            window.search_spec(ws, sa)
        assert lib.lspiv_search_supported(sa[0], sa[1], ws[0], ws[1]) == 0
    assert window.search_spec((32, 32), None) == (32, 32) and window.search_spec((32, 32), (32, 32)) == (32, 32)
    spec = window.search_spec((12, 12), (32, 32))
    assert isinstance(spec, window.SearchWindow) and tuple(spec) == (32, 32) and spec.window == (12, 12)
    assert lib.lspiv_search_supported(32, 32, 12, 12) == 1 and lib.lspiv_search_supported(64, 64, 62, 62) == 1


def test_grid_coordinates_and_planner_follow_the_search_area():
    dim = (160, 200)
    spec = window.search_spec((12, 12), (32, 32))
    assert window.get_array_shape(dim, spec, (16, 16)) == window.get_array_shape(dim, (32, 32), (16, 16)) == (9, 11)
    x, y = window.get_rect_coordinates(dim, (12, 12), (16, 16), search_area_size=(32, 32))
    xo, yo = po.get_rect_coordinates(dim, (12, 12), (16, 16), search_area_size=(32, 32))
    assert np.array_equal(x, xo) and np.array_equal(y, yo) and x[0] == 16 and x[1] - x[0] == 16
    assert window.chunk_alignment(spec, dim, (16, 16)) == 1 and window.chunk_alignment(spec) == 1
    need = window.required_memory(10, dim, (12, 12), (16, 16), search_area_size=(32, 32), with_planes=True)
    assert need == window.required_memory(10, dim, (32, 32), (16, 16), with_planes=True) == window.required_memory(10, dim, spec, (16, 16), with_planes=True)
    assert need > window.required_memory(10, dim, (12, 12), (6, 6)) - 10 * 160 * 200 and need >= 10 * 160 * 200 + 9 * 99 * (4 * 4 + 32 * 32 * 4)
    from pyorc_amd import frames
    assert frames.resolve_window(12, None, 32) == ((12, 12), (32, 32), (16, 16))
    assert frames.resolve_window((12, 12), (8, 8), (32, 32)) == ((12, 12), (32, 32), (8, 8))
    assert frames.resolve_window(32) == ((32, 32), (32, 32), (16, 16))


def test_ensemble_with_a_search_area_raises():
    a = np.zeros((3, 64, 64), np.uint8)
    with pytest.raises(NotImplementedError, match="ensemble_corr=True with search_area_size != window_size"):
        velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), (12, 12), (16, 16), (32, 32), 1.0, 1.0, ensemble_corr=True)


def fast_flow_shares(u, v):
    eu, ev = np.abs(u - 10.0), np.abs(v + 9.0)
    with np.errstate(invalid="ignore"):
        good = (eu <= 0.5) & (ev <= 0.5)
    return float(np.nanmedian(eu)), float(np.nanmedian(ev)), float(good.mean())


def test_fast_flow_input_meets_its_conditions_in_the_reference():
    """The point of the feature, on the CPU: a uniform shift of (+10, -9) px is recovered by 12 in 32 and lost by plain 12 x 12."""
    a = fast_stack()
    r = ref.search_piv(a, (12, 12), (32, 32), (16, 16))
    mu, mv, share = fast_flow_shares(r["u"], r["v"])
    print("search 12 in 32:", mu, mv, share)
    assert mu < 0.1 and mv < 0.1 and share >= 0.95
    _, _, planes = po.cross_corr(a, (12, 12), (6, 6))
    y12, x12 = (len(c) for c in po.get_rect_coordinates((160, 160), (12, 12), (6, 6))[::-1])
    u12, v12 = po.u_v_displacement(planes, y12, x12)
    plain = fast_flow_shares(u12, v12)[2]
    print("plain 12 x 12:", plain)
    assert plain < 0.2
