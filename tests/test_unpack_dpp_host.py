"""The column-to-lane map of the 32 x 32 walking kernels under "unpack_dpp" (csrc/piv_fft_impl.h, unpack_col), read from the library
through lspiv_debug_unpack_map, and a numpy restatement of the un-packing in the permuted layout against the natural-order one.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from pyorc_amd import _lib

N, H = 32, 16


@pytest.fixture(scope="module")
def maps(lib):
    col, col_rt, lane = np.zeros(N, int), np.zeros(N, int), np.zeros(N, int)
    for i in range(N):
        a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        _lib.check(lib.lspiv_debug_unpack_map(i, C.byref(a), C.byref(b), C.byref(c)))
        col[i], col_rt[i], lane[i] = a.value, b.value, c.value
    return col, col_rt, lane


def test_map_is_the_one_of_the_design(maps):
    col, col_rt, lane = maps
    want = [0, 16] + [0] * 30
    for j in range(1, 16):
        want[2 * j], want[2 * j + 1] = j, 32 - j
    assert col.tolist() == want
    assert col_rt.tolist() == want, "the branch-free run-time form of the second transpose"


def test_map_is_a_bijection_with_its_inverse(maps):
    col, _, lane = maps
    assert sorted(col.tolist()) == list(range(N))
    assert sorted(lane.tolist()) == list(range(N))
    assert all(lane[col[l]] == l for l in range(N)) and all(col[lane[k]] == k for k in range(N))


def test_quad_partner_holds_the_mirrored_column(maps):
    col = maps[0]
    for l in range(2, N):
        assert col[l ^ 1] == (-col[l]) % N, l
    # the two columns that mirror onto themselves sit in lanes 0 and 1, and DC stays in lane 0 (the plane means are read there)
    assert col[0] == 0 and col[1] == 16
    assert all((-col[l]) % N == col[l] for l in (0, 1))


def test_out_of_range_is_refused(lib):
    a = C.c_int()
    assert lib.lspiv_debug_unpack_map(32, C.byref(a), C.byref(a), C.byref(a)) != 0
    assert lib.lspiv_debug_unpack_map(-1, C.byref(a), C.byref(a), C.byref(a)) != 0


def unpack(xr, xi, fpr, fpi, mirror):
    """unpack_step for ky = 0 .. 16 in float32 with the kernel's expressions and order; x[ky, lane], mirror(v) = v of the mirrored lane.
    Returns the packed spectra and the new carry."""
    xr, xi, fpr, fpi = xr.copy(), xi.copy(), fpr.copy(), fpi.copy()
    f = np.float32
    for ky in range(H + 1):
        kn = (N - ky) % N
        mr, mi = mirror(xr[kn]), mirror(xi[kn])
        pr, pi = xr[ky] + mr, xi[ky] - mi
        ar = f(fpr[ky] * pr) + f(fpi[ky] * pi)
        ai = f(fpr[ky] * pi) - f(fpi[ky] * pr)
        fpr[ky] = xi[ky] + mi
        fpi[ky] = mr - xr[ky]
        qr, qi = fpr[ky], fpi[ky]
        br = f(pr * qr) + f(pi * qi)
        bi = f(pr * qi) - f(pi * qr)
        xr[ky] = ar - bi
        xi[ky] = ai + br
        if 1 <= ky < H:
            xr[kn] = mirror(ar + bi)
            xi[kn] = -mirror(ai - br)
    return xr, xi, fpr, fpi


def test_unpack_in_the_paired_layout_equals_the_natural_one(maps):
    col = maps[0]
    rng = np.random.default_rng(7)
    xr, xi = rng.standard_normal((2, N, N)).astype(np.float32)          # [ky, kx]
    fpr, fpi = rng.standard_normal((2, H + 1, N)).astype(np.float32)
    xr[3, 5] = np.nan
    natural = unpack(xr, xi, fpr, fpi, lambda v: v[(-np.arange(N)) % N])

    def quad_swap(v):   # quad_perm:[1,0,3,2], lanes 0 and 1 keep their own value
        w = v[np.arange(N) ^ 1]
        w[:2] = v[:2]
        return w

    paired = unpack(xr[:, col], xi[:, col], fpr[:, col], fpi[:, col], quad_swap)
    for got, want in zip(paired, natural):
        assert got.tobytes() == want[:, col].tobytes()
