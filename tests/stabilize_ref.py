"""Float64 numpy reference of frame stabilisation: camera shake estimated by PIV on the static part of the
image (the banks), one robust transform fit per frame pair, the chain of poses, and the affine warp that locks every frame to frame 0.
The semantics are this project's own: unpinned against pyorc's ``Video(stabilize=...)`` and against ``cv2.warpAffine``.

  vectors   tests/masked_ref.piv under the static mask; u column shift, v row shift, rows downward (SEMANTICS["v_sign"] undone once)
  fit       P_t (2 x 3) with x_{t+1} = P_t (x_t, y_t, 1) for a static point: (u, v) = (P - I)(x, y, 1) by least squares through the normal
            equations, float64 sums, closed-form solves, three rounds (all finite vectors; those within reject[0] of round 1; those within
            reject[1] of round 2 -- each selection from the finite set); coordinates relative to ((W - 1) / 2, (H - 1) / 2)
  chain     C_0 = carry, C_{t+1} = [P_t; 0 0 1] C_t, every product and sum a separately rounded float64 operation; A_t = the pose of frame t
  warp      out[t](y, x) = bilinear sample of frames[t] at A_t (x, y, 1): the fixed-point walk of oracle.project_oracle.warp_map after its
            inversion with w = 1, then remap_linear -- both RESTATED here (the oracle stays as it is; tests/test_stabilize_host.py pins
            the restatement to it on matrices whose inverse is exact)

Also the shaken scene tests/test_stabilize_host.py and tests/test_gpu_stabilize.py share, computed once per process."""
import functools

import numpy as np

from oracle import piv_oracle as po
from tests import masked_ref

WINDOWS = (16, 32, 64)
MODELS = ("translation", "similarity", "affine")
REJECT = (2.0, 0.5)
MIN_VECTORS = 6
COVERAGE_MIN = 0.5
SINGULAR_RTOL = 1e-9      # the determinant test: relative to the product of the normal matrix's diagonal (see _solve)
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS
BLOCK_W = 64


# ---- warp ----------------------------------------------------------------------------------------------------------------------------
def _round_half_even_to_int(a):
    a = np.clip(np.nan_to_num(a, nan=0.0, posinf=2.0**31 - 1, neginf=-2.0**31), -2.0**31, 2.0**31 - 1)
    return np.rint(a).astype(np.int64)


def walk(A, shape):
    """(ix, iy, frac) of every destination pixel of ``shape`` = (H, W) for the inverse map A (2, 3): the 64-pixel block walk, every
    operation a separately rounded float64 operation, 1/32 px, NaN -> 0, clipped to int32, round half to even."""
    a = [float(q) for q in np.asarray(A, dtype=np.float64).reshape(6)]
    H, W = shape
    xs = np.arange(W)
    xb = (xs // BLOCK_W) * BLOCK_W
    x1 = (xs - xb).astype(np.float64)
    xb = xb.astype(np.float64)
    y = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X0 = a[0] * xb + a[1] * y + a[2]
        Y0 = a[3] * xb + a[4] * y + a[5]
        fX = np.clip((X0 + a[0] * x1) * float(INTER_TAB_SIZE), -2.0**31, 2.0**31 - 1)
        fY = np.clip((Y0 + a[3] * x1) * float(INTER_TAB_SIZE), -2.0**31, 2.0**31 - 1)
        X = _round_half_even_to_int(fX)
        Y = _round_half_even_to_int(fY)
    return X >> INTER_BITS, Y >> INTER_BITS, (Y & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (X & (INTER_TAB_SIZE - 1))


def blend(img, ix, iy, frac):
    """Bilinear blend of one uint8 or float32 frame at (ix, iy) + frac / 32: uint8 with integer weights and (acc + 2^14) >> 15, float32
    with the float32 weight table added left to right; neighbours outside the frame count as 0."""
    img = np.asarray(img)
    if img.dtype not in (np.uint8, np.float32):
        raise TypeError(f"uint8 and float32 frames only, got {img.dtype}")
    Hs, Ws = img.shape
    ix = np.clip(ix, -32768, 32767)
    iy = np.clip(iy, -32768, 32767)
    fx = (frac & (INTER_TAB_SIZE - 1)).astype(np.int64)
    fy = (frac >> INTER_BITS).astype(np.int64)

    def px(yy, xx):
        ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
        return np.where(ok, img[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)], 0)

    p00, p01, p10, p11 = px(iy, ix), px(iy, ix + 1), px(iy + 1, ix), px(iy + 1, ix + 1)
    if img.dtype == np.uint8:
        w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
        acc = p00.astype(np.int64) * w00 + p01.astype(np.int64) * w01 + p10.astype(np.int64) * w10 + p11.astype(np.int64) * w11
        return ((acc + (1 << 14)) >> 15).astype(np.uint8)
    a, b = fx.astype(np.float32) / np.float32(32), fy.astype(np.float32) / np.float32(32)
    one = np.float32(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    f = lambda p: p.astype(np.float32)  # noqa: E731
    with np.errstate(all="ignore"):
        return ((f(p00) * w00 + f(p01) * w01) + f(p10) * w10) + f(p11) * w11


def warp(frames, A):
    """out[t] = frames[t] sampled at A[t] (x, y, 1); (T, H, W) uint8 or float32, A (T, 2, 3)."""
    frames = np.asarray(frames)
    if frames.dtype not in (np.uint8, np.float32):
        raise TypeError(f"uint8 and float32 stacks only, got {frames.dtype}")
    A = np.asarray(A, dtype=np.float64).reshape(-1, 2, 3)
    if len(A) != len(frames):
        raise ValueError(f"{len(A)} transforms for {len(frames)} frames")
    return np.stack([blend(f, *walk(a, f.shape)) for f, a in zip(frames, A)])


# ---- fit -----------------------------------------------------------------------------------------------------------------------------
def centres(n, overlap, shape):
    """(xc (cols,), yc (rows,)) of the window grid: col (n - ox) + (n - 1) / 2, row (n - oy) + (n - 1) / 2."""
    H, W = shape
    oy, ox = (overlap, overlap) if np.isscalar(overlap) else overlap
    rows, cols = po.get_axis_shape(H, n, oy), po.get_axis_shape(W, n, ox)
    return np.arange(cols) * float(n - ox) + (n - 1) / 2.0, np.arange(rows) * float(n - oy) + (n - 1) / 2.0


def _solve(model, x, y, u, v, min_vectors):
    """The coefficients (a, b, c, d, e, f) of u = a x + b y + c, v = d x + e y + f over the given vectors, or None: fewer than min_vectors,
    or a singular normal matrix.  Closed forms, float64.  The determinant test is scale-aware: the determinant is compared with
    SINGULAR_RTOL times the product of the normal matrix's diagonal (a dimensionless ratio in [0, 1] that no unit of length changes):
      translation  never singular
      similarity   N S2 - Sx^2 - Sy^2  <=  rtol N S2          (S2 = Sxx + Syy; the 4 x 4 determinant is the square of the left side)
      affine       det [[Sxx Sxy Sx] [Sxy Syy Sy] [Sx Sy N]]  <=  rtol N Sxx Syy"""
    N = len(x)
    if N < max(int(min_vectors), 1):
        return None
    Nf = float(N)
    Su, Sv = float(u.sum()), float(v.sum())
    if model == "translation":
        return 0.0, 0.0, Su / Nf, 0.0, 0.0, Sv / Nf
    Sx, Sy, Sxx, Sxy, Syy = float(x.sum()), float(y.sum()), float((x * x).sum()), float((x * y).sum()), float((y * y).sum())
    Sxu, Syu, Sxv, Syv = float((x * u).sum()), float((y * u).sum()), float((x * v).sum()), float((y * v).sum())
    if model == "similarity":      # u = a x - b y + c, v = b x + a y + d
        S2 = Sxx + Syy
        D = Nf * S2 - Sx * Sx - Sy * Sy
        if not D > SINGULAR_RTOL * (Nf * S2):
            return None
        a = (Nf * (Sxu + Syv) - Sx * Su - Sy * Sv) / D
        b = (Nf * (Sxv - Syu) - Sx * Sv + Sy * Su) / D
        c = (Su - a * Sx + b * Sy) / Nf
        d = (Sv - b * Sx - a * Sy) / Nf
        return a, -b, c, b, a, d
    if model != "affine":
        raise ValueError(f"unknown model {model!r}")
    # the adjugate of the symmetric normal matrix [[Sxx Sxy Sx] [Sxy Syy Sy] [Sx Sy N]]
    c00, c01, c02 = Syy * Nf - Sy * Sy, Sx * Sy - Sxy * Nf, Sxy * Sy - Syy * Sx
    c11, c12, c22 = Sxx * Nf - Sx * Sx, Sxy * Sx - Sxx * Sy, Sxx * Syy - Sxy * Sxy
    det = Sxx * c00 + Sxy * c01 + Sx * c02
    if not det > SINGULAR_RTOL * (Nf * Sxx * Syy):
        return None
    sol = []
    for r0, r1, r2 in ((Sxu, Syu, Su), (Sxv, Syv, Sv)):
        sol += [(c00 * r0 + c01 * r1 + c02 * r2) / det, (c01 * r0 + c11 * r1 + c12 * r2) / det, (c02 * r0 + c12 * r1 + c22 * r2) / det]
    return tuple(sol)


def fit(u, v, n, overlap, shape, model="similarity", reject=REJECT, min_vectors=MIN_VECTORS, details=False):
    """(P (2, 3), n_used) of ONE pair from its (rows, cols) vectors; with ``details`` also the residuals (px, finite vectors only) that
    rounds 2 and 3 selected from, for the margin checks of the tests."""
    if model not in MODELS:
        raise ValueError(f"unknown model {model!r}")
    H, W = shape
    xc, yc = centres(n, overlap, shape)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    X, Y = np.meshgrid(xc - (W - 1) / 2.0, yc - (H - 1) / 2.0)
    ok = np.isfinite(u) & np.isfinite(v)
    x, y, u, v = X[ok], Y[ok], u[ok], v[ok]
    sel = np.ones(len(x), dtype=bool)
    res = []
    co = None
    for rnd in range(3):
        co = _solve(model, x[sel], y[sel], u[sel], v[sel], min_vectors)
        if co is None:
            return (IDENTITY.copy(), 0, res) if details else (IDENTITY.copy(), 0)
        if rnd < 2:
            du = u - ((co[0] * x + co[1] * y) + co[2])
            dv = v - ((co[3] * x + co[4] * y) + co[5])
            r2 = du * du + dv * dv
            sel = r2 <= float(reject[rnd]) * float(reject[rnd])
            res.append(np.sqrt(r2))
    a, b, c, d, e, f = co
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    P = np.array([[1.0 + a, b, (c - a * cx) - b * cy], [d, 1.0 + e, (f - d * cx) - e * cy]])
    return (P, int(sel.sum()), res) if details else (P, int(sel.sum()))


def fit_pairs(u, v, n, overlap, shape, model="similarity", reject=REJECT, min_vectors=MIN_VECTORS):
    r = [fit(a, b, n, overlap, shape, model, reject, min_vectors) for a, b in zip(u, v)]
    return np.stack([q[0] for q in r]), np.array([q[1] for q in r], dtype=np.int32)


# ---- chain ---------------------------------------------------------------------------------------------------------------------------
def chain(P, carry=None):
    """(A (T, 2, 3), carry_out (2, 3)) for P (T - 1, 2, 3): A[0] = carry (identity by default), then [P_t; 0 0 1] [A_t; 0 0 1], each
    element (p0 c0 + p1 c1) + p2 c2 with separately rounded float64 products and sums (no fused multiply-add)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2, 3)
    C = np.vstack([IDENTITY if carry is None else np.asarray(carry, dtype=np.float64).reshape(2, 3), [[0.0, 0.0, 1.0]]])
    A = [C[:2].copy()]
    with np.errstate(all="ignore"):
        for p in P:
            p3 = np.vstack([p, [[0.0, 0.0, 1.0]]])
            C = (p3[:, 0:1] * C[0:1, :] + p3[:, 1:2] * C[1:2, :]) + p3[:, 2:3] * C[2:3, :]
            A.append(C[:2].copy())
    return np.stack(A), A[-1].copy()


# ---- the whole mode ------------------------------------------------------------------------------------------------------------------
def vectors(frames, mask, n=32, overlap=None, coverage_min=COVERAGE_MIN):
    """(u, v) (T - 1, rows, cols) float32-valued: masked PIV under the static mask, kernel orientation."""
    o = n // 2 if overlap is None else overlap
    with po.semantics(v_sign=0):
        r = masked_ref.piv(frames, n, o, mask, coverage_min)
    return r["u"].astype(np.float32), r["v"].astype(np.float32)


def estimate(frames, mask, n=32, overlap=None, model="similarity", coverage_min=COVERAGE_MIN, reject=REJECT, min_vectors=MIN_VECTORS,
             carry=None, uv=None):
    """dict(A, pairwise, n_used, carry); ``uv``: vectors computed before (the scene's)."""
    o = n // 2 if overlap is None else overlap
    u, v = vectors(frames, mask, n, o, coverage_min) if uv is None else uv
    P, n_used = fit_pairs(u, v, n, o, np.asarray(frames).shape[1:], model, reject, min_vectors)
    A, carry_out = chain(P, carry)
    return dict(A=A, pairwise=P, n_used=n_used, carry=carry_out)


def apply(P, pts):
    """P (..., 2, 3) applied to points (k, 2) = (x, y): (..., k, 2)."""
    pts = np.asarray(pts, dtype=np.float64)
    return np.einsum("...ij,kj->...ki", np.asarray(P)[..., :2], pts) + np.asarray(P)[..., None, :, 2]


def corners(shape):
    H, W = shape
    return np.array([[0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0]])


def corner_error(P, Q, shape):
    """Largest distance (px) between P c and Q c over the frame's four corners, per leading index."""
    d = apply(P, corners(shape)) - apply(Q, corners(shape))
    return np.hypot(d[..., 0], d[..., 1]).max(axis=-1)


# ---- the shaken scene ----------------------------------------------------------------------------------------------------------------
TRUTH = (3.3, -2.4)
SCENE_DIM = (160, 200)
SCENE_FRAMES = 8          # 7 frames are the issue's scene; the eighth lets the chunk tests cut 4 + 4
SCENE_WINDOW = (32, 16)
# (seed, shake in px per frame, shake in rad per frame): the rows of INTEGRATION.md's gain table
SCENES = ((1, 1.5, 0.002), (2, 1.5, 0.002), (1, 3.0, 0.004), (3, 0.5, 0.001))
GPU_SCENE = SCENES[0]     # the one the GPU end-to-end test runs (qualified by tests/test_stabilize_host.py)
# Largest movement (px) of a corner of any A_t of GPU_SCENE when the reference's u, v are perturbed by uniform +-1e-4 px (the PIV parity
# gate), 20 draws (tests/test_stabilize_host.py measures it again and checks that this constant covers it); the GPU test allows 4 x this
GATE_CORNER_MOVE = 2.5e-4   # measured 2.449e-4


def bank_line(y):
    return 84 + 18 * np.sin(2 * np.pi * y / 97) + 6 * np.sin(2 * np.pi * y / 23)


def _erode(m, r):
    """Binary erosion by a (2 r + 1)-square; outside the image counts as set."""
    out = m.copy()
    H, W = m.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            s = np.ones_like(m)
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            s[yd, xd] = m[ys, xs]
            out &= s
    return out


@functools.lru_cache(maxsize=None)
def stable_mask():
    """The bank (left of the wavy line) eroded by 8 px."""
    H, W = SCENE_DIM
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return _erode(x < bank_line(y), 8)


@functools.lru_cache(maxsize=None)
def water_windows(n=32, o=16, margin=12):
    """(rows, cols) bool: windows that lie wholly right of the bank line by ``margin`` px."""
    H, W = SCENE_DIM
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    M = po.sliding_window_stack((x >= bank_line(y) + margin)[None], (n, n), (o, o))[0]
    rows, cols = po.get_axis_shape(H, n, o), po.get_axis_shape(W, n, o)
    return M.all(axis=(-2, -1)).reshape(rows, cols)


def _splat(img, xs, ys, amp, sigma):
    H, W = img.shape
    r = int(np.ceil(4 * sigma))
    for x0, y0, a0 in zip(xs, ys, amp):
        ix, iy = int(round(x0)), int(round(y0))
        xa, xb, ya, yb = max(ix - r, 0), min(ix + r + 1, W), max(iy - r, 0), min(iy + r + 1, H)
        if xa >= xb or ya >= yb:
            continue
        gx = np.exp(-((np.arange(xa, xb) - x0) ** 2) / (2 * sigma * sigma))
        gy = np.exp(-((np.arange(ya, yb) - y0) ** 2) / (2 * sigma * sigma))
        img[ya:yb, xa:xb] += a0 * gy[:, None] * gx[None, :]


@functools.lru_cache(maxsize=None)
def scene(seed, shake_px, shake_rad, n_frames=SCENE_FRAMES):
    """dict(frames (T, H, W) uint8, P_true (T - 1, 2, 3), A_true (T, 2, 3)): static blobs on the bank, tracers moving by TRUTH in the water,
    seen by a camera whose pose is a random walk -- per frame a translation of shake_px (rms) and a rotation of shake_rad (rms) about the
    frame centre.  Rendered analytically (Gaussians at A_t (world position)): no resampling enters the truth."""
    H, W = SCENE_DIM
    rng = np.random.default_rng(1000 + seed)
    pad = 40
    nb = int(0.06 * (H + 2 * pad) * (W + 2 * pad))
    bx, by = rng.uniform(-pad, W + pad, nb), rng.uniform(-pad, H + pad, nb)
    bamp = rng.uniform(60, 160, nb)
    tx, ty = rng.uniform(-pad, W + pad, nb), rng.uniform(-pad, H + pad, nb)
    tamp = rng.uniform(120, 220, nb)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    P_true = []
    for _ in range(n_frames - 1):
        th = rng.normal() * shake_rad
        d = rng.normal(size=2) * shake_px / np.sqrt(2.0)
        c, s = np.cos(th), np.sin(th)
        P_true.append([[c, -s, cx - c * cx + s * cy + d[0]], [s, c, cy - s * cx - c * cy + d[1]]])
    P_true = np.array(P_true)
    A_true, _ = chain(P_true)
    frames = []
    span_x, span_y = W + 2 * pad, H + 2 * pad
    for t in range(n_frames):
        img = np.zeros((H, W))
        keep = bx < bank_line(by)
        q = apply(A_true[t], np.stack([bx[keep], by[keep]], axis=1))
        _splat(img, q[:, 0], q[:, 1], bamp[keep], 1.3)
        wx = (tx + t * TRUTH[0] + pad) % span_x - pad
        wy = (ty + t * TRUTH[1] + pad) % span_y - pad
        keep = wx >= bank_line(wy)
        q = apply(A_true[t], np.stack([wx[keep], wy[keep]], axis=1))
        _splat(img, q[:, 0], q[:, 1], tamp[keep], 1.1)
        frames.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return dict(frames=np.stack(frames), P_true=P_true, A_true=A_true)


@functools.lru_cache(maxsize=None)
def scene_vectors(seed, shake_px, shake_rad):
    n, o = SCENE_WINDOW
    return vectors(scene(seed, shake_px, shake_rad)["frames"], stable_mask(), n, o)


@functools.lru_cache(maxsize=None)
def scene_ref(seed, shake_px, shake_rad, model="similarity"):
    """The reference on a scene: estimate() plus the stabilised frames."""
    n, o = SCENE_WINDOW
    f = scene(seed, shake_px, shake_rad)["frames"]
    r = estimate(f, stable_mask(), n, o, model, uv=scene_vectors(seed, shake_px, shake_rad))
    r["frames"] = warp(f, r["A"])
    return r


def water_score(uv, n=32, o=16):
    """(share of the fully-water windows within 0.5 px of TRUTH, their median error in px, their count) for ``uv`` = (u, v), the plain PIV
    of a stack in kernel orientation (:func:`plain_piv`); NaN counts as a miss."""
    u, v = uv
    sel = np.broadcast_to(water_windows(n, o), u.shape)
    with np.errstate(invalid="ignore"):
        err = np.hypot(np.asarray(u, np.float64) - TRUTH[0], np.asarray(v, np.float64) - TRUTH[1])[sel]
    miss = ~(err <= 0.5)
    return float(1.0 - miss.mean()), float(np.median(np.where(np.isnan(err), np.inf, err))), int(sel.sum())


def plain_piv(frames, n=32, o=16):
    """(u, v) of the oracle's plain PIV, kernel orientation."""
    f = np.asarray(frames)
    rows, cols = po.get_axis_shape(f.shape[1], n, o), po.get_axis_shape(f.shape[2], n, o)
    with po.semantics(v_sign=0):
        u, v, _, _ = po.get_uv_timestep(f, cols, rows, (n, n), (o, o))
    return u, v
