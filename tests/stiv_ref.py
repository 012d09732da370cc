"""The semantics of space-time image velocimetry (pyorc_amd.stiv) in float64 / float32 numpy, the scene
generator of its tests and the inputs of the GPU parity tests.  Unpinned against any other STIV code: this file IS the statement.

    points -> space_time_images (float32, every operation rounded on its own: the GPU gives the same bits)
           -> orientation (float64 on the float32 samples: the GPU agrees within the GATE_* bounds below)
           -> velocity (one float64 multiplication chain)
"""
import functools

import numpy as np

MAX_SMOOTH = 3
# the gates of the GPU parity tests.  Tensor: n <= 1e5 float64 additions (1e-11) and the cancellation inside the integer-tap gradients,
# relative to the trace; slope and coherency follow from the tensor through one square root and one division.
GATE_TENSOR = 1e-9     # |J - J_ref| <= GATE_TENSOR * (Jxx + Jtt)
GATE_SLOPE = 1e-8      # |m - m_ref| <= GATE_SLOPE * (1 + m_ref^2)
GATE_COHERENCY = 1e-8
# what a parity input must have for the slope gate to mean something (checked on the CPU for every input)
PARITY_MIN_COHERENCY = 0.3
PARITY_MAX_SLOPE = 4.0


# ---- 1. sample points -----------------------------------------------------------------------------------------------------------------
def line_points(lines, samples):
    """(S, L, 2) float64 (x, y): s = i / (L - 1), x = x0 + s (x1 - x0), y alike."""
    a = np.asarray(lines, dtype=np.float64)
    s = np.arange(samples, dtype=np.float64) / (samples - 1)
    return np.stack([a[:, 0:1] + s * (a[:, 2:3] - a[:, 0:1]), a[:, 1:2] + s * (a[:, 3:4] - a[:, 1:2])], axis=2)


def line_spacing(lines, samples):
    a = np.asarray(lines, dtype=np.float64)
    return np.hypot(a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]) / (samples - 1)


def points_valid(points, H, W):
    """Per line: every point finite and inside [0, W - 1] x [0, H - 1]."""
    p = np.asarray(points, dtype=np.float64)
    ok = (p[..., 0] >= 0.0) & (p[..., 0] <= W - 1) & (p[..., 1] >= 0.0) & (p[..., 1] <= H - 1)
    return ok.all(axis=1)


# ---- 2. space-time image --------------------------------------------------------------------------------------------------------------
def space_time_images(frames, points):
    """sti (S, T, L) float32: ix = min(floor(x), W - 2), fx = float32(x - ix); top = a + fx (b - a), bot = c + fx (d - c),
    value = top + fy (bot - top), every operation one float32 operation (numpy fuses nothing)."""
    f = np.asarray(frames)
    T, H, W = f.shape
    p = np.asarray(points, dtype=np.float64)
    assert points_valid(p, H, W).all() and H >= 2 and W >= 2
    ix = np.minimum(np.floor(p[..., 0]), W - 2).astype(np.int64)
    iy = np.minimum(np.floor(p[..., 1]), H - 2).astype(np.int64)
    fx = (p[..., 0] - ix).astype(np.float32)
    fy = (p[..., 1] - iy).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = f[:, iy, ix].astype(np.float32), f[:, iy, ix + 1].astype(np.float32)       # (T, S, L)
        c, d = f[:, iy + 1, ix].astype(np.float32), f[:, iy + 1, ix + 1].astype(np.float32)
        top = a + fx * (b - a)
        bot = c + fx * (d - c)
        val = top + fy * (bot - top)
    assert val.dtype == np.float32
    return np.ascontiguousarray(val.transpose(1, 0, 2))


# ---- 3. time windows ------------------------------------------------------------------------------------------------------------------
def window_starts(T, time_window=None, time_stride=None):
    """(Tw, stride, starts): K = floor((T - Tw) / stride) + 1 windows, window k on rows k stride .. k stride + Tw - 1."""
    Tw = T if time_window is None else int(time_window)
    stride = Tw if time_stride is None else int(time_stride)
    K = (T - Tw) // stride + 1
    return Tw, stride, [k * stride for k in range(K)]


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------
def binomial_row(m):
    row = np.array([1.0])
    for _ in range(m):
        row = np.convolve(row, [1.0, 1.0])
    return row


def taps(k):
    """(b, dx): b = b_{2k+2}, dx = [-1, 0, 1] * b_{2k}; both 2k + 3 integers.  k passes of the 3 x 3 binomial before a Sobel pair are
    Gx = dx(i) (x) b(t), Gt = b(i) (x) dx(t) up to a common scale, which cancels in slope and coherency."""
    return binomial_row(2 * k + 2), np.convolve([-1.0, 0.0, 1.0], binomial_row(2 * k))


def _correlate_last(g, tap):
    """Valid positions along the last axis, tap j on sample i + j, the products added with j ascending."""
    n = len(tap)
    m = g.shape[-1] - n + 1
    acc = tap[0] * g[..., 0:m]
    for j in range(1, n):
        acc = acc + tap[j] * g[..., j:j + m]
    return acc


def gradients(win, k):
    """(Gx, Gt) of a window (..., Tw, L) float64 at the (Tw - 2k - 2)(L - 2k - 2) positions whose stencil lies inside it: along the
    line first, then along time."""
    b, dx = taps(k)
    hx, hb = _correlate_last(win, dx), _correlate_last(win, b)
    gx = _correlate_last(np.swapaxes(hx, -1, -2), b)
    gt = _correlate_last(np.swapaxes(hb, -1, -2), dx)
    return np.swapaxes(gx, -1, -2), np.swapaxes(gt, -1, -2)


# ---- 5. tensor, slope, coherency ------------------------------------------------------------------------------------------------------
def closed_form(tensor):
    """(slope, coherency) of tensor (..., 3) = (Jxx, Jtt, Jxt): the half-angle form of the total-least-squares orientation."""
    Jxx, Jtt, Jxt = tensor[..., 0], tensor[..., 1], tensor[..., 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = Jxx - Jtt
        r = np.sqrt(d * d + 4.0 * Jxt * Jxt)
        return (-2.0 * Jxt) / (d + r), r / (Jxx + Jtt)


def orientation(sti, time_window=None, time_stride=None, smooth=1, detrend=True):
    """(tensor (S, K, 3), slope (S, K), coherency (S, K)) float64 of sti (S, T, L) float32."""
    sti = np.asarray(sti)
    assert sti.dtype == np.float32 and sti.ndim == 3 and 0 <= smooth <= MAX_SMOOTH
    S, T, L = sti.shape
    Tw, stride, starts = window_starts(T, time_window, time_stride)
    n = 2 * smooth + 3
    assert L >= n and n <= Tw <= T and stride >= 1
    tensor = np.empty((S, len(starts), 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, t0 in enumerate(starts):
            win = sti[:, t0:t0 + Tw].astype(np.float64)
            if detrend:
                total = np.zeros((S, L))
                for t in range(Tw):          # t ascending
                    total = total + win[:, t]
                win = win - (total / Tw)[:, None, :]
            gx, gt = gradients(win, smooth)
            tensor[:, k, 0] = (gx * gx).sum(axis=(1, 2))
            tensor[:, k, 1] = (gt * gt).sum(axis=(1, 2))
            tensor[:, k, 2] = (gx * gt).sum(axis=(1, 2))
    slope, coh = closed_form(tensor)
    return tensor, slope, coh


def velocity(slope, ds, resolution=1.0, dt=1.0):
    """v = ((slope ds) resolution) / dt, float64."""
    return slope * np.asarray(ds, dtype=np.float64)[:, None] * float(resolution) / float(dt)


def stiv(frames, lines, samples, time_window=None, time_stride=None, smooth=1, detrend=True, resolution=1.0, dt=1.0):
    """(v, slope, coherency, tensor, ds) as pyorc_amd.stiv.stiv gives them."""
    sti = space_time_images(frames, line_points(lines, samples))
    tensor, slope, coh = orientation(sti, time_window, time_stride, smooth, detrend)
    ds = line_spacing(lines, samples)
    return velocity(slope, ds, resolution, dt), slope, coh, tensor, ds


# ---- the river scene ------------------------------------------------------------------------------------------------------------------
SCENE_SHAPE = (48, 96, 160)
SCENE_SAMPLES = 129
SCENE_AMPLITUDE = 22.0
SCENE_SPEEDS = (0.15, 1.6)


def _texture(rng, H, N, sigma):
    """White noise filtered by a Gaussian of `sigma` px (periodic, through the FFT), scaled to unit standard deviation."""
    ky, kx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(N)[None, :]
    g = np.exp(-2.0 * (np.pi * sigma) ** 2 * (kx * kx + ky * ky))
    t = np.fft.ifft2(np.fft.fft2(rng.normal(size=(H, N))) * g).real
    return t / t.std()


def scene_speed(y):
    """The speed along +x of the water at row y, px per frame: a sine profile between the banks."""
    lo, hi = SCENE_SPEEDS
    return lo + (hi - lo) * np.sin(np.pi * np.asarray(y, dtype=np.float64) / (SCENE_SHAPE[1] - 1))


@functools.lru_cache(maxsize=None)
def river_scene(seed, noise_sigma, static=True):
    """48 frames of 96 x 160 uint8: a Gaussian-filtered random texture (sigma 2 px, 22 grey levels) advected along +x at a speed that
    depends on the row (0.15 .. 1.6 px per frame), a static texture of the same amplitude (the bed) and white noise.  The advection is
    a Fourier shift of each row of a periodic strip wider than the frame: exact for any sub-pixel shift."""
    T, H, W = SCENE_SHAPE
    N = 256
    rng = np.random.default_rng(seed)
    moving = np.fft.fft(_texture(rng, H, N, 2.0), axis=1)
    bed = _texture(rng, H, N, 2.0)[:, :W] if static else 0.0
    k = np.fft.fftfreq(N)[None, :]
    u = scene_speed(np.arange(H))[:, None]
    frames = np.empty((T, H, W), dtype=np.uint8)
    for t in range(T):
        row = np.fft.ifft(moving * np.exp(-2j * np.pi * k * u * t), axis=1).real[:, :W]
        f = 128.0 + SCENE_AMPLITUDE * row + SCENE_AMPLITUDE * bed + noise_sigma * rng.normal(size=(H, W))
        frames[t] = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return frames


def scene_lines():
    """14 horizontal lines of 129 samples, ds = 1, at fractional offsets (0.3, 0.25); their true slopes."""
    y = 6.25 + 6.0 * np.arange(14)
    lines = np.stack([np.full(14, 15.3), y, np.full(14, 15.3 + SCENE_SAMPLES - 1), y], axis=1)
    return lines, scene_speed(y)


def scene_error(frames, smooth, detrend, reverse=False):
    """(median |slope - truth| over the 14 lines, lowest coherency, slopes) of the reference on a scene."""
    lines, truth = scene_lines()
    if reverse:
        lines = lines[:, [2, 3, 0, 1]]
        truth = -truth
    _, slope, coh, _, _ = stiv(frames, lines, SCENE_SAMPLES, smooth=smooth, detrend=detrend)
    return float(np.median(np.abs(slope[:, 0] - truth))), float(coh.min()), slope[:, 0]


# ---- inputs of the GPU parity tests of the orientation --------------------------------------------------------------------------------
# (S, T, L, time_window, time_stride, smooth, omega, m0): Tw and L at 2k + 3 exactly and above for every k; T in {3, 7, 33}; S in {1, 5};
# L below, at and above a wave, no multiple of it, and beyond one strip of 256 columns; windows that overlap, abut, leave gaps, and K = 1.
# omega (rad per sample) and m0 (samples per frame) shape the texture of the case: a window of exactly 2k + 3 rows leaves one row of
# stencils, where detrending turns the time smoothing into a second difference, and k passes of the binomial pass low frequencies only,
# so each case gets a texture that its filter passes and that moves enough inside its window -- the slope gate needs coherency >=
# PARITY_MIN_COHERENCY and |slope| < PARITY_MAX_SLOPE on EVERY case (tests/test_stiv_host.py checks that on the reference).
PARITY_SHAPES = [
    (1, 3, 3, 3, 3, 0, 2.0, 0.8),
    (1, 7, 5, 5, 1, 1, 1.7, 0.5),
    (1, 7, 7, 7, 7, 2, 1.0, 0.5),
    (1, 33, 9, 9, 9, 3, 0.8, 0.8),
    (5, 3, 37, 3, 1, 0, 2.0, 0.8),
    (5, 7, 64, 5, 1, 1, 1.8, 0.5),
    (5, 7, 65, 7, 7, 2, 1.4, 0.5),
    (1, 33, 130, 16, 8, 1, 1.3, 0.8),
    (5, 33, 130, 11, 11, 3, 0.6, 0.8),
    (5, 33, 65, 33, 33, 2, 1.0, 0.5),
    (1, 33, 64, 10, 23, 0, 1.0, 0.5),
    (1, 7, 300, 7, 7, 1, 1.5, 0.5),
    (5, 33, 37, 12, 7, 3, 0.6, 0.8),
]
PARITY_CASES = [shape + (detrend,) for shape in PARITY_SHAPES for detrend in (True, False)]


@functools.lru_cache(maxsize=None)
def moving_texture(S, T, L, omega=1.0, m0=0.5, seed=0):
    """A space-time image (S, T, L) float32 of two sine textures (omega and 1.25 omega rad per sample) that travel along each line at a
    slope of its own (m0 .. m0 + 0.3 samples per frame, the sign alternating from line to line), on a static offset with a slow
    static ripple and a little noise: what the orientation parity runs on."""
    rng = np.random.default_rng(1000 * S + 10 * T + L + seed)
    i, t = np.arange(L)[None, None, :], np.arange(T)[None, :, None]
    m = np.linspace(m0, m0 + 0.3, S) * np.where(np.arange(S) % 2, -1.0, 1.0) if S > 1 else np.array([m0 + 0.1])
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(S, 1, 1))
    z = i - m[:, None, None] * t
    g = 120.0 + 40.0 * np.sin(omega * z + phase) + 15.0 * np.sin(1.25 * omega * z + 2.0 * phase) + 10.0 * np.cos(0.05 * i) \
        + 0.5 * rng.normal(size=(S, T, L))
    out = g.astype(np.float32)
    out.setflags(write=False)
    return out
