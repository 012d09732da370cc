"""Float64 numpy reference of the window deformation passes: the node predictor, the dense field, the warp,
one pass and the chain, composed of tests/multipass_ref.py and the oracle's own pieces, which it leaves as they are.  Like the rest of
the PIV path it is this project's reading: unpinned against a real ffpiv.  Kernel orientation throughout (u column shift, v row shift,
rows downward); SEMANTICS["v_sign"] is applied once, to the result of a pass or of a chain.

Also the inputs tests/test_deform_host.py and tests/test_gpu_deform.py share, computed once per process."""
import functools
import warnings

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd import synth
from tests import ensemble_multipass_ref as emp
from tests import multipass_ref as mp

Q = 64                      # sub-pixel positions per pixel; the nodes are in 1 / (2 Q) px
DEFORM_WINDOWS = (16, 32, 64)
QMAX = 32767 * Q


def predict_nodes(u, v):
    """(u, v) float32 (P, rows, cols) -> int64 nodes (P, rows, cols, 2) = {v, u} in 1 / 128 px: q = rint(64 x) in float32 (half to even;
    the product is exact) clamped to +-32767 * 64, valid when u and v are finite; twice the 3 x 3 median over the valid neighbours."""
    u = np.asarray(u, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32)
    if u.ndim == 2:
        u, v = u[None], v[None]
    out = np.zeros(u.shape + (2,), dtype=np.int64)
    for p in range(u.shape[0]):
        valid = np.isfinite(u[p]) & np.isfinite(v[p])
        with np.errstate(invalid="ignore", over="ignore"):
            qu = np.clip(np.where(valid, np.rint(np.float32(Q) * u[p]), 0), -QMAX, QMAX).astype(np.int64)
            qv = np.clip(np.where(valid, np.rint(np.float32(Q) * v[p]), 0), -QMAX, QMAX).astype(np.int64)
        out[p, :, :, 0] = mp._median2(qv, valid)
        out[p, :, :, 1] = mp._median2(qu, valid)
    return out


def _axis2(npix, n, s, count):
    """(i0, i1, w0, w1) per pixel on doubled coordinates: node i at 2 i s + n - 1, pixel p at 2 p."""
    d = 2 * np.arange(npix, dtype=np.int64) - (n - 1)
    S2 = 2 * s
    i0 = np.clip(np.floor_divide(d, S2), 0, max(count - 2, 0))
    w1 = np.clip(d - i0 * S2, 0, S2) if count > 1 else np.zeros_like(d)
    return i0, np.minimum(i0 + 1, count - 1), S2 - w1, w1


def dense64(nodes, dim_size, n, overlap):
    """The dense field of ONE pair's nodes (rows, cols, 2): (dv64, du64) int64 (H, W) in 1 / 64 px, exact integers."""
    H, W = dim_size
    m = np.asarray(nodes, dtype=np.int64)
    rows, cols = m.shape[:2]
    s = n - overlap
    iy0, iy1, wy0, wy1 = _axis2(H, n, s, rows)
    ix0, ix1, wx0, wx1 = _axis2(W, n, s, cols)
    den = 4 * s * s
    out = []
    for comp in (0, 1):
        c = m[:, :, comp]
        num = ((wy0[:, None] * wx0[None, :]) * c[iy0[:, None], ix0[None, :]] + (wy0[:, None] * wx1[None, :]) * c[iy0[:, None], ix1[None, :]] +
               (wy1[:, None] * wx0[None, :]) * c[iy1[:, None], ix0[None, :]] + (wy1[:, None] * wx1[None, :]) * c[iy1[:, None], ix1[None, :]])
        out.append(np.floor_divide(num + den, 2 * den))
    return out[0], out[1]


def warp64(frame, dv64, du64):
    """Frame t+1 sampled at (64 y + dv64, 64 x + du64) / 64, clamped to the frame (the edge is replicated), bilinear in 1 / 64 px.
    uint8: float64, exact (an integer / 4096); float32 and float64 frames: narrowed to float32, then a fixed order of float32 products
    and sums -- what the device computes, bit for bit -- returned as float64."""
    frame = np.asarray(frame)
    H, W = frame.shape
    Y = np.clip(Q * np.arange(H, dtype=np.int64)[:, None] + dv64, 0, Q * (H - 1))
    X = np.clip(Q * np.arange(W, dtype=np.int64)[None, :] + du64, 0, Q * (W - 1))
    iy, fy, ix, fx = Y >> 6, Y & 63, X >> 6, X & 63
    fy = np.where(iy == H - 1, Q, fy)
    iy = np.where(iy == H - 1, H - 2, iy)
    fx = np.where(ix == W - 1, Q, fx)
    ix = np.where(ix == W - 1, W - 2, ix)
    w00, w01, w10, w11 = (Q - fy) * (Q - fx), (Q - fy) * fx, fy * (Q - fx), fy * fx
    if frame.dtype == np.uint8:
        I = frame.astype(np.int64)
        num = w00 * I[iy, ix] + w01 * I[iy, ix + 1] + w10 * I[iy + 1, ix] + w11 * I[iy + 1, ix + 1]
        return num.astype(np.float64) / 4096.0
    I = frame.astype(np.float32)
    f = lambda w: w.astype(np.float32)
    with np.errstate(all="ignore"):
        t = f(w00) * I[iy, ix]
        t = t + f(w01) * I[iy, ix + 1]
        t = t + f(w10) * I[iy + 1, ix]
        t = t + f(w11) * I[iy + 1, ix + 1]
        t = t * np.float32(1.0 / 4096.0)
    assert t.dtype == np.float32
    return t.astype(np.float64)


def warp_stack(imgs, n, overlap, nodes):
    """(T-1, H, W) float64: frame t+1 of every pair warped by the pair's nodes."""
    imgs = np.asarray(imgs)
    return np.stack([warp64(imgs[t + 1], *dense64(nodes[t], imgs.shape[1:], n, overlap)) for t in range(imgs.shape[0] - 1)])


def deformed_piv(imgs, n, overlap, nodes=None, signal_threshold=None):
    """One deformation pass (``overlap`` an int, or a pair (oy, ox) with oy == ox: like the library's, the node grid of this pass has one
    stride for both axes): the plain oracle between frame t and the warped frame t+1 on the grid (n, overlap), plus the window's own
    node.  dict(u, v, corr, s2n (T-1, rows, cols), planes (T-1, n_win, n, n), tie, nodes, warped, x, y).  ``imgs`` in the stack's own
    sample type (the warp of float frames is float32 arithmetic)."""
    imgs = np.asarray(imgs)
    T, H, W = imgs.shape
    if n not in DEFORM_WINDOWS:
        raise ValueError(f"window {n} not in {DEFORM_WINDOWS}")
    oy, ox = mp.overlap_pair(overlap)
    if oy != ox:
        raise ValueError(f"overlap {(oy, ox)}: the deformation pass takes one overlap for both axes")
    overlap = oy
    if po.SEMANTICS["signal_mode"] == 1 or not po.SEMANTICS["norm_clip"]:
        raise NotImplementedError("deformation pass: signal_mode = 1 and norm_clip = 0 are not supported")
    x, y = po.get_rect_coordinates((H, W), (n, n), (overlap, overlap))
    y0, x0 = mp.grid_origins((H, W), n, overlap)
    rows, cols = len(y0), len(x0)
    nodes = np.zeros((T - 1, rows, cols, 2), dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(T - 1, rows, cols, 2)
    warped = warp_stack(imgs, n, overlap, nodes)
    sa = po.sliding_window_stack(imgs.astype(np.float64), (n, n), (overlap, overlap))          # (T, n_win, n, n)
    sb = po.sliding_window_stack(warped, (n, n), (overlap, overlap))                           # (T-1, n_win, n, n)
    planes = np.full((T - 1, rows * cols, n, n), np.nan)
    for t in range(T - 1):
        A, B = sa[t], sb[t]
        keep = po.signal_mask(A, B, signal_threshold)
        if keep.any():
            planes[t, keep] = po.ncc(A[keep], B[keep])
    with po.semantics(v_sign=0):
        u, v = po.u_v_displacement(planes, rows, cols)
    u = nodes[..., 1] / 128.0 + u
    v = nodes[..., 0] / 128.0 + v
    if po.SEMANTICS["v_sign"]:
        v = -v
    shape = (T - 1, rows, cols)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        cm = np.nanmax(planes, axis=(-2, -1))
        s2n = cm / np.nanmean(planes, axis=(-2, -1))
    top = np.sort(planes.reshape(planes.shape[:2] + (-1,)), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        tie = ((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (cm > 0)
    return dict(u=u, v=v, corr=cm.reshape(shape), s2n=s2n.reshape(shape), planes=planes, tie=tie.reshape(shape), nodes=nodes, warped=warped, x=x, y=y)


def chain(imgs, passes, deform_passes, signal_threshold=None):
    """The chain of multipass_ref followed by ``deform_passes`` deformation passes on the final grid, each fed with the float32 (u, v) of
    the pass before it.  A list of per-pass dicts in the kernels' orientation, except that the LAST one's v carries SEMANTICS["v_sign"]."""
    n, ov = passes[-1]
    with po.semantics(v_sign=0):
        out = mp.multipass(imgs, passes, signal_threshold)
        for _ in range(deform_passes):
            nodes = predict_nodes(out[-1]["u"].astype(np.float32), out[-1]["v"].astype(np.float32))
            out.append(deformed_piv(imgs, n, ov, nodes, signal_threshold))
    if po.SEMANTICS["v_sign"]:
        out[-1] = dict(out[-1], v=-out[-1]["v"])
    return out


def flow_error(u, v, dim_size, n, overlap):
    """Euclidean distance of every vector (kernel orientation) to synth.flow_field at the true window centres origin + n / 2 - 0.5."""
    H, W = dim_size
    y0, x0 = mp.grid_origins(dim_size, n, overlap)
    yc, xc = np.meshgrid(y0 + n / 2 - 0.5, x0 + n / 2 - 0.5, indexing="ij")
    tu, tv = synth.flow_field(H, W, yc, xc)
    return np.hypot(np.asarray(u, np.float64) - tu, np.asarray(v, np.float64) - tv)


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------------
PASS_CASES = emp.PASS_CASES                       # 16 @ 8 on 48 x 53, 32 @ 16 on 96 x 131, 64 @ 32 on 160 x 200
PASS_DTYPES = (np.uint8, np.float32, np.float64)
PASS_T = 4
GRID_CASES = {"one-row": (32, 16, (40, 131)), "75%": (64, 48, (96, 130))}
ACCURACY_SEEDS = (5, 6)
ACCURACY_CHAIN = [(64, 32), (32, 16)]
SIGNAL_THR = 0.3


@functools.lru_cache(maxsize=None)
def pass_stack(case, dtype=np.uint8):
    n, ov, (H, W) = PASS_CASES[case] if case in PASS_CASES else GRID_CASES[case]
    a = synth.particle_stack(PASS_T, H, W, seed=20 + n, density=0.05, uniform_shift=(float(emp.PASS_SHIFT[0]), float(emp.PASS_SHIFT[1])))
    return emp.as_samples(a, dtype)


@functools.lru_cache(maxsize=None)
def hand_nodes(case):
    """Hand-made nodes (P, rows, cols, 2) int32 {v, u} in 1 / 128 px: the stack's uniform displacement plus a smooth field of up to 1.5 px
    plus a scatter of +-0.4 px per window -- and, at a few windows of the grid's edge, values of tens of pixels that push samples
    across the frame edge (the warp replicates the edge there)."""
    n, ov, dim = PASS_CASES[case] if case in PASS_CASES else GRID_CASES[case]
    y0, x0 = mp.grid_origins(dim, n, ov)
    rows, cols = len(y0), len(x0)
    rng = np.random.default_rng(300 + n + rows)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    out = np.empty((PASS_T - 1, rows, cols, 2), dtype=np.int32)
    for p in range(PASS_T - 1):
        smooth_u = 1.5 * np.sin(2 * np.pi * (rr + p) / max(rows, 2)) * np.cos(np.pi * cc / max(cols, 2))
        smooth_v = 1.0 * np.cos(2 * np.pi * (cc - p) / max(cols, 2))
        out[p, :, :, 1] = np.rint(128 * (emp.PASS_SHIFT[0] + smooth_u + rng.uniform(-0.4, 0.4, (rows, cols))))
        out[p, :, :, 0] = np.rint(128 * (emp.PASS_SHIFT[1] + smooth_v + rng.uniform(-0.4, 0.4, (rows, cols))))
    out[0, 0, 0] = (-40 * 128, -25 * 128)
    out[1, rows - 1, cols - 1] = (33 * 128 + 7, 60 * 128 + 1)
    out[2, 0, cols - 1] = (-9 * 128, 45 * 128 + 64)
    return out


@functools.lru_cache(maxsize=None)
def pass_ref(case, dtype=np.uint8, nodes="hand", signal_threshold=None):
    n, ov, _ = PASS_CASES[case] if case in PASS_CASES else GRID_CASES[case]
    return deformed_piv(pass_stack(case, dtype), n, ov, hand_nodes(case) if nodes == "hand" else None, signal_threshold)


@functools.lru_cache(maxsize=None)
def signal_stack(case):
    """Samples below 40 set to zero and the upper left quarter of every frame empty: a threshold of 0.3 takes out some windows."""
    a = pass_stack(case).copy()
    a[a < 40] = 0
    a[:, :a.shape[1] // 2, :a.shape[2] // 2] = 0
    return a


@functools.lru_cache(maxsize=None)
def signal_ref(case):
    n, ov, _ = PASS_CASES[case]
    return deformed_piv(signal_stack(case), n, ov, hand_nodes(case), SIGNAL_THR)


def signal_fractions(case):
    """(fa, fb): the non-zero fractions of every window of frame t and of the warped frame t+1 of signal_ref's input."""
    n, ov, _ = PASS_CASES[case]
    a, r = signal_stack(case), signal_ref(case)
    sa = po.sliding_window_stack(a.astype(np.float64), (n, n), (ov, ov))[:-1]
    sb = po.sliding_window_stack(r["warped"], (n, n), (ov, ov))
    return (sa != 0).mean(axis=(-2, -1)), (sb != 0).mean(axis=(-2, -1))


@functools.lru_cache(maxsize=None)
def accuracy_stack(seed):
    return synth.particle_stack(4, 160, 200, seed=seed, density=0.06)


@functools.lru_cache(maxsize=None)
def accuracy_ref(seed):
    """The reference chain 64 -> 32 + one deformation pass on the sheared stack: (integer chain's last pass, deformation pass)."""
    out = chain(accuracy_stack(seed), ACCURACY_CHAIN, 1)
    return out[-2], out[-1]


def accuracy_figures(u, v):
    """(median error, share within 0.1 px) of a field on the final grid of ACCURACY_CHAIN, over the finite vectors."""
    n, ov = ACCURACY_CHAIN[-1]
    e = flow_error(u, v, (160, 200), n, ov)
    e = e[np.isfinite(e)]
    return float(np.median(e)), float((e <= 0.1).mean())


# ---- the float64 rescue pass on warped windows: the inputs of tests/test_gpu_rescue_modes.py (stack and geometries: tests/multipass_ref.py) ----
RESCUE_FIELDS = ("uniform", "mixed")


@functools.lru_cache(maxsize=None)
def rescue_nodes(n, overlap, field):
    """int32 nodes (P, rows, cols, 2) {v, u} in 1 / 128 px.  "uniform": u = 1 px everywhere, the speckles' drift (the warp is a whole-pixel
    move, the residual exactly 0); "mixed": every other column of nodes at u = 0.5 px, every other row at v = -37 / 128 px (the warp
    interpolates: the speckles spread over two to four samples)."""
    rows, cols = (len(q) for q in mp.grid_origins(mp.RESCUE_DIM, n, overlap))
    nodes = np.zeros((mp.RESCUE_T - 1, rows, cols, 2), dtype=np.int32)
    nodes[..., 1] = 128
    if field == "mixed":
        nodes[:, :, 1::2, 1] = 64
        nodes[:, 1::2, :, 0] = -37
    return nodes


@functools.lru_cache(maxsize=None)
def rescue_ref(n, overlap, field, dtype=np.uint8):
    return deformed_piv(mp.rescue_stack(dtype), n, overlap, rescue_nodes(n, overlap, field))
