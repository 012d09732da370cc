"""CPU tests of frame stabilisation: the float64 reference tests/stabilize_ref.py against the oracle's remap
pieces and against itself, the gain on the shaken scene, the conditions on the inputs that tests/test_gpu_stabilize.py relies on, and the
argument errors of pyorc_amd.stabilize.  No kernel runs here."""
import numpy as np
import pytest

from oracle import project_oracle as pj
from pyorc_amd import stabilize
from tests import stabilize_ref as sr

SHAPE = (70, 150)      # two full 64-px blocks and a partial one, an odd height


def _frames(dtype, T=1, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(T,) + SHAPE)
    return f.astype(np.uint8) if dtype == np.uint8 else (f + rng.random((T,) + SHAPE)).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-70, 5), (64, 64), (-1, -1)])
def test_restated_walk_and_blend_are_the_oracles(dtype, shift):
    """warp_map inverts its matrix; for the identity and integer translations the inverse is exact, so A = inv(M)[:2] is known."""
    tx, ty = shift
    M = np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
    A = np.array([[1.0, 0.0, -tx], [0.0, 1.0, -ty]])
    want = pj.warp_map(M, SHAPE)
    got = sr.walk(A, SHAPE)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    f = _frames(dtype)[0]
    a, b = sr.blend(f, *got), pj.remap_linear(f, *want)
    assert a.dtype == b.dtype == dtype and np.array_equal(a, b)
    # a fractional map through both blends: the same table, the same order
    rng = np.random.default_rng(5)
    ix, iy = rng.integers(-3, SHAPE[1] + 3, size=SHAPE), rng.integers(-3, SHAPE[0] + 3, size=SHAPE)
    frac = rng.integers(0, 1024, size=SHAPE)
    assert np.array_equal(sr.blend(f, ix, iy, frac), pj.remap_linear(f, ix, iy, frac))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_identity_returns_the_inputs_bits(dtype):
    f = _frames(dtype, T=3)
    out = sr.warp(f, np.broadcast_to(sr.IDENTITY, (3, 2, 3)))
    assert out.dtype == f.dtype and np.array_equal(out.view(np.uint8), f.view(np.uint8))


def _exact_vectors(P, n, o, shape, outliers, seed, nan=0):
    xc, yc = sr.centres(n, o, shape)
    X, Y = np.meshgrid(xc, yc)
    u = (P[0, 0] - 1.0) * X + P[0, 1] * Y + P[0, 2]
    v = P[1, 0] * X + (P[1, 1] - 1.0) * Y + P[1, 2]
    rng = np.random.default_rng(seed)
    idx = rng.permutation(u.size)
    bad = idx[:int(outliers * u.size)]
    ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(3.0, 8.0, len(bad))
    u.ravel()[bad] += mag * np.cos(ang)
    v.ravel()[bad] += mag * np.sin(ang)
    u.ravel()[idx[len(bad):len(bad) + nan]] = np.nan
    return u, v, u.size - len(bad) - nan


MODEL_P = {"translation": np.array([[1.0, 0.0, 2.25], [0.0, 1.0, -1.5]]),
           "similarity": np.array([[1.002 * np.cos(0.004), -1.002 * np.sin(0.004), 1.75], [1.002 * np.sin(0.004), 1.002 * np.cos(0.004), -2.5]]),
           "affine": np.array([[1.003, -0.002, 1.25], [0.004, 0.998, 0.75]])}


@pytest.mark.parametrize("model", sr.MODELS)
def test_fit_recovers_the_model_under_gross_outliers(model):
    P = MODEL_P[model]
    u, v, n_good = _exact_vectors(P, 32, 16, sr.SCENE_DIM, 0.20, seed=3, nan=4)
    got, n_used = sr.fit(u, v, 32, 16, sr.SCENE_DIM, model)
    assert n_used == n_good
    assert sr.corner_error(got, P, sr.SCENE_DIM) < 1e-10
    # a model with fewer unknowns than the data needs cannot reach that: the check above is not vacuous
    if model == "affine":
        assert sr.corner_error(sr.fit(u, v, 32, 16, sr.SCENE_DIM, "translation")[0], P, sr.SCENE_DIM) > 0.1


@pytest.mark.parametrize("model", sr.MODELS)
def test_degenerate_fits_are_the_identity(model):
    u, v, _ = _exact_vectors(MODEL_P[model], 32, 16, sr.SCENE_DIM, 0.0, seed=1)
    few = np.full(u.shape, np.nan)
    few.ravel()[[3, 17, 40, 55, 80]] = u.ravel()[[3, 17, 40, 55, 80]]        # 5 finite vectors < min_vectors = 6
    P, n_used = sr.fit(few, v, 32, 16, sr.SCENE_DIM, model)
    assert n_used == 0 and np.array_equal(P, sr.IDENTITY)
    # one row of windows: y is constant, "affine" is not determined; the other two models are
    shape = (40, 200)
    u1, v1, _ = _exact_vectors(MODEL_P[model], 32, 16, shape, 0.0, seed=1)
    assert u1.shape[0] == 1
    P, n_used = sr.fit(u1, v1, 32, 16, shape, model)
    if model == "affine":
        assert n_used == 0 and np.array_equal(P, sr.IDENTITY)
    else:
        assert n_used == u1.size and sr.corner_error(P, MODEL_P[model], shape) < 1e-10
    # a single window determines a translation only
    P, n_used = sr.fit(np.full((1, 1), 1.5), np.full((1, 1), -0.5), 32, 16, (40, 40), model, min_vectors=1)
    assert (n_used == 0) == (model != "translation")


def test_chain_is_sequential_unfused_and_carries():
    rng = np.random.default_rng(2)
    P = sr.IDENTITY + rng.normal(size=(9, 2, 3)) * [[1e-3, 1e-3, 2.0]]
    A, carry = sr.chain(P)
    assert np.array_equal(A[0], sr.IDENTITY) and np.array_equal(carry, A[-1])
    for t in range(9):          # element by element with Python floats: one rounding per operation
        for i in range(2):
            for j in range(3):
                want = (float(P[t, i, 0]) * float(A[t, 0, j]) + float(P[t, i, 1]) * float(A[t, 1, j])) + float(P[t, i, 2]) * (1.0 if j == 2 else 0.0)
                assert A[t + 1, i, j] == want
    A2, carry2 = sr.chain(P[4:], carry=A[4])
    assert np.array_equal(A2, A[4:]) and np.array_equal(carry2, carry)


def test_chunked_reference_is_the_whole_reference():
    sc = sr.GPU_SCENE
    f = sr.scene(*sc)["frames"]
    whole = sr.scene_ref(*sc)
    n, o = sr.SCENE_WINDOW
    for cut in (4, 3):        # 4 + 4 frames, and an odd start
        a = sr.estimate(f[:cut + 1], sr.stable_mask(), n, o)
        b = sr.estimate(f[cut:], sr.stable_mask(), n, o, carry=a["carry"])
        A = np.concatenate([a["A"], b["A"][1:]])
        assert np.array_equal(A, whole["A"]) and np.array_equal(b["carry"], whole["carry"])
        assert np.array_equal(np.concatenate([a["n_used"], b["n_used"]]), whole["n_used"])
        frames = np.concatenate([sr.warp(f[:cut], a["A"][:cut]), sr.warp(f[cut:], b["A"])])
        assert np.array_equal(frames, whole["frames"])


@pytest.mark.parametrize("sc", sr.SCENES)
def test_stabilising_helps_on_the_shaken_scene(sc):
    """The figures of INTEGRATION.md section 2l's gain table (7 frames, 32 @ 16): printed, then asserted."""
    s = sr.scene(*sc)
    f = s["frames"][:7]
    n, o = sr.SCENE_WINDOW
    uv = tuple(q[:6] for q in sr.scene_vectors(*sc))
    raw = sr.water_score(sr.plain_piv(f))
    line = f"seed {sc[0]}, shake {sc[1]} px / {sc[2]} rad: raw median {raw[1]:.3f} px share {raw[0]:.2f}"
    for model in ("similarity", "affine"):
        r = sr.estimate(f, sr.stable_mask(), n, o, model, uv=uv)
        ce = float(sr.corner_error(r["pairwise"], s["P_true"][:6], sr.SCENE_DIM).max())
        line += f"; {model}: corner error <= {ce:.3f} px, n_used {r['n_used'].min()}..{r['n_used'].max()}"
        if model == "similarity":
            st = sr.water_score(sr.plain_piv(sr.warp(f, r["A"])))
            line += f", stabilised median {st[1]:.3f} px share {st[0]:.2f} ({st[2]} windows)"
            assert st[0] > raw[0] and st[1] < raw[1]
            assert st[0] >= 0.95
            assert ce < 0.5 * sc[1] + 0.25      # the pose is recovered far below the shake itself
    print(line)


def test_gpu_scene_is_qualified():
    """What tests/test_gpu_stabilize.py relies on: no residual of the reference within 1e-3 px of a rejection threshold (the kernel's
    vectors differ from the reference's by up to 1e-4 px, the PIV gate: the selections must come out the same) and at least 30 windows
    used in every pair."""
    sc = sr.GPU_SCENE
    u, v = sr.scene_vectors(*sc)
    n, o = sr.SCENE_WINDOW
    for t in range(len(u)):
        P, n_used, res = sr.fit(u[t], v[t], n, o, sr.SCENE_DIM, details=True)
        assert n_used >= 30
        for r, lim in zip(res, sr.REJECT):
            gap = float(np.abs(r - lim).min())
            print(f"pair {t}: limit {lim} px, nearest residual {gap:.4f} px away, n_used {n_used}")
            assert gap >= 1e-3


def test_gate_corner_move_constant_covers_the_measurement():
    """u, v of the reference perturbed by uniform +-1e-4 px (the PIV parity gate), 20 draws: the largest movement of a corner of any A_t
    is what stabilize_ref.GATE_CORNER_MOVE records (the GPU end-to-end test allows 4 x the constant)."""
    sc = sr.GPU_SCENE
    u, v = sr.scene_vectors(*sc)
    n, o = sr.SCENE_WINDOW
    f = sr.scene(*sc)["frames"]
    ref = sr.scene_ref(*sc)
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(20):
        du, dv = (rng.uniform(-1e-4, 1e-4, size=u.shape) for _ in range(2))
        r = sr.estimate(f, sr.stable_mask(), n, o, uv=(u + du, v + dv))
        assert np.array_equal(r["n_used"], ref["n_used"])
        worst = max(worst, float(sr.corner_error(r["A"], ref["A"], sr.SCENE_DIM).max()))
    print(f"largest corner movement under +-1e-4 px: {worst:.3e} px (constant {sr.GATE_CORNER_MOVE:.1e})")
    assert 0.25 * sr.GATE_CORNER_MOVE <= worst <= sr.GATE_CORNER_MOVE


def test_argument_errors(lib):
    f = np.zeros((3, 64, 80), dtype=np.uint8)
    m = np.ones((64, 80), dtype=bool)
    with pytest.raises(ValueError, match="stable_mask"):
        stabilize.estimate(f, np.ones((64, 81), dtype=bool))
    for n in (8, 24, 128, 32.5):
        with pytest.raises(ValueError, match="window_size"):
            stabilize.estimate(f, m, window_size=n)
    with pytest.raises(ValueError, match="model"):
        stabilize.estimate(f, m, model="homography")
    for rej in ((0.5, 2.0), (2.0, 2.0), (2.0, 0.0), (2.0, -1.0), (np.inf, 0.5), (2.0,)):
        with pytest.raises(ValueError, match="reject"):
            stabilize.estimate(f, m, reject=rej)
    with pytest.raises(ValueError, match="2 frames"):
        stabilize.estimate(f[:1], m)
    with pytest.raises(ValueError, match="carry"):
        stabilize.estimate(f, m, carry=np.eye(3))
    for call in (lambda: stabilize.estimate(f.astype(np.float64), m), lambda: stabilize.warp(f.astype(np.float64), np.zeros((3, 2, 3))),
                 lambda: stabilize.stabilize(f.astype(np.float64), m)):
        with pytest.raises(TypeError, match="float64"):
            call()
    with pytest.raises(ValueError, match="A must have shape"):
        stabilize.warp(f, np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match="out must"):
        stabilize.warp(f, np.zeros((3, 2, 3)), out=np.zeros((3, 64, 80), dtype=np.float32))
    with pytest.raises(TypeError, match="float64"):
        sr.warp(f.astype(np.float64), np.zeros((3, 2, 3)))


def test_c_abi_argument_errors(lib):
    """LSPIV_EINVAL with a message, before any device is touched."""
    import ctypes as C

    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(pairs=1, rows=9, cols=11, n=32, oy=16, ox=16, H=160, W=200, model=1, r0=2.0, r1=0.5, mv=6)
    for change, word in ((dict(n=24), b"window"), (dict(rows=8), b"grid"), (dict(model=3), b"model"), (dict(r0=0.5, r1=2.0), b"reject"),
                         (dict(mv=0), b"min_vectors"), (dict(pairs=0), b"pairs"), (dict(ox=32), b"overlap")):
        a = dict(ok, **change)
        for fn, tail in ((lib.lspiv_stabilize_fit_dev, (None,)), (lib.lspiv_stabilize_fit, ())):
            rc = fn(p, p, a["pairs"], a["rows"], a["cols"], a["n"], a["oy"], a["ox"], a["H"], a["W"], a["model"], a["r0"], a["r1"], a["mv"], p, p, *tail)
            assert rc == -1 and word in lib.lspiv_last_error(), (change, lib.lspiv_last_error())
    assert lib.lspiv_stabilize_fit_dev(None, p, 1, 9, 11, 32, 16, 16, 160, 200, 1, 2.0, 0.5, 6, p, p, None) == -1
    assert lib.lspiv_stabilize_chain_dev(None, 3, None, p, None, None) == -1 and lib.lspiv_stabilize_chain(p, -1, None, p, None) == -1
    q = C.c_void_p(p.value + 8)
    assert lib.lspiv_warp_affine_dev(p, 2, 1, 4, 4, p, q, None) == -1 and b"dtype" in lib.lspiv_last_error()
    assert lib.lspiv_warp_affine(p, 0, 1, 4, 40000, p, q) == -1 and b"shape" in lib.lspiv_last_error()
    assert lib.lspiv_warp_affine_dev(p, 0, 1, 4, 4, p, p, None) == -1 and b"another buffer" in lib.lspiv_last_error()
