"""Space-time image velocimetry (STIV; Fujita et al.): one velocity per search line from all T frames of a stack.

The other standard method of image-based river gauging next to PIV (Fudaa-LSPIV, Hydro-STIV and RIVeR offer both; pyorc has none).  The
brightness along a short search line laid along the flow is sampled in every frame and stacked into a space-time image; the speed along
the line is the orientation of the streaks in that image.  It needs no discrete tracers, only advected texture, and gives velocities
where a hydrologist wants them: at the stations of a transect:

    lines = stiv.lines_across(transect_xy, length=128.0)               # one line per station, across the transect
    r = stiv.stiv(frames, lines, samples=129, resolution=0.01, dt=1 / 25)    # Stiv: .v (S, K) m/s, .slope, .coherency, .tensor, .ds
    sti = stiv.space_time_images(frames, lines, 129)                   # (S, T, L) float32: host array, or DeviceFrames for a DeviceFrames
    o = stiv.orientation(sti, time_window=250, time_stride=125)        # Orientation: .tensor (S, K, 3), .slope (S, K), .coherency (S, K)

The semantics are this project's own -- unpinned against any other STIV code; tests/stiv_ref.py is their float64 / float32 numpy
statement.  A long video runs in chunks: ``space_time_images(chunk, lines, L, out=sti, t_offset=a)`` fills rows ``[a, a + len(chunk))``
of one space-time image, bit for bit what one call over the whole stack gives.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _lib, device
from .device import DeviceFrames, is_device

MAX_SMOOTH = 3


class Orientation(NamedTuple):
    """``tensor`` (S, K, 3) float64: (Jxx, Jtt, Jxt) of every line and time window; ``slope`` (S, K): samples per frame, positive from
    point 0 of the line towards its last point; ``coherency`` (S, K): 0 (no orientation) .. 1 (one orientation).  NaN for a constant
    window and for one that holds a NaN."""
    tensor: np.ndarray
    slope: np.ndarray
    coherency: np.ndarray


class Stiv(NamedTuple):
    """``v`` (S, K) = slope * ds * resolution / dt: the velocity along each line; ``slope``, ``coherency``, ``tensor`` as in
    ``Orientation``; ``ds`` (S,): the sample spacing of each line in pixels."""
    v: np.ndarray
    slope: np.ndarray
    coherency: np.ndarray
    tensor: np.ndarray
    ds: np.ndarray


def _check_lines(lines, samples):
    a = np.asarray(lines, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"lines must be (S, 4) rows of (x0, y0, x1, y1), got shape {a.shape}")
    if isinstance(samples, bool) or int(samples) != samples:
        raise TypeError(f"samples must be an integer, got {samples!r}")
    if int(samples) < 3:
        raise ValueError(f"samples {samples!r} < 3")
    return a, int(samples)


def line_points(lines, samples: int) -> np.ndarray:
    """The sample points (S, L, 2) = (x, y) of the lines ``(x0, y0, x1, y1)``: x = x0 + s (x1 - x0) with s = i / (L - 1), y alike."""
    a, L = _check_lines(lines, samples)
    s = np.arange(L, dtype=np.float64) / (L - 1)
    with np.errstate(invalid="ignore"):      # (a line that is not finite is reported by the caller's check, not by a warning)
        return np.stack([a[:, 0:1] + s * (a[:, 2:3] - a[:, 0:1]), a[:, 1:2] + s * (a[:, 3:4] - a[:, 1:2])], axis=2)


def line_spacing(lines, samples: int) -> np.ndarray:
    """``ds`` (S,) = hypot(x1 - x0, y1 - y0) / (L - 1) px."""
    a, L = _check_lines(lines, samples)
    return np.hypot(a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]) / (L - 1)


def lines_across(transect_xy, length: float, direction=None) -> np.ndarray:
    """One search line of ``length`` px centred on every point of ``transect_xy`` (N, 2), as (N, 4) rows (x0, y0, x1, y1).

    ``direction``: the direction of every line from its point 0 to its last point -- an angle in radians (from +x towards +y, i.e.
    clockwise on the screen) or a vector (dx, dy) (normalised here).  Default: perpendicular to the local tangent of the transect
    (central differences, one-sided at the ends), the tangent turned by +90 degrees from +x towards +y: (tx, ty) -> (-ty, tx).  Walk the
    transect the other way round to flip the lines.  Host numpy only."""
    p = np.asarray(transect_xy, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"transect_xy must be (N, 2), got shape {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("transect_xy holds a value that is not finite")
    length = float(length)
    if not (length > 0.0 and np.isfinite(length)):
        raise ValueError(f"length {length!r} must be positive")
    if direction is None:
        if len(p) < 2:
            raise ValueError("a transect of one point has no tangent: give direction")
        t = np.gradient(p, axis=0)
        norm = np.hypot(t[:, 0], t[:, 1])
        if (norm == 0.0).any():
            raise ValueError(f"transect point {int(np.argmax(norm == 0.0))} repeats its neighbours: no tangent there")
        n = np.stack([-t[:, 1], t[:, 0]], axis=1) / norm[:, None]
    else:
        d = np.asarray(direction, dtype=np.float64)
        if d.ndim == 0:
            d = np.array([np.cos(d), np.sin(d)])
        if d.shape != (2,) or not np.isfinite(d).all() or np.hypot(d[0], d[1]) == 0.0:
            raise ValueError(f"direction must be an angle or a vector (dx, dy) that is not zero, got {direction!r}")
        n = np.broadcast_to(d / np.hypot(d[0], d[1]), p.shape)
    h = 0.5 * length
    return np.concatenate([p - h * n, p + h * n], axis=1)


def _check_points(points, lines, H, W):
    """Every point finite and inside [0, W - 1] x [0, H - 1]: the ValueError names the first line that is not."""
    ok = (points[..., 0] >= 0.0) & (points[..., 0] <= W - 1) & (points[..., 1] >= 0.0) & (points[..., 1] <= H - 1)   # False for NaN
    if not ok.all():
        s = int(np.argmax(~ok.all(axis=1)))
        i = int(np.argmax(~ok[s]))
        raise ValueError(f"line {s} {tuple(float(q) for q in lines[s])} leaves the frame [0, {W - 1}] x [0, {H - 1}] (or is not finite) at "
                         f"sample {i}: ({float(points[s, i, 0])!r}, {float(points[s, i, 1])!r})")


def space_time_images(frames, lines, samples: int, out=None, t_offset: int = 0):
    """``sti[s, t_offset + t, i]`` (float32) = the bilinear sample of ``frames[t]`` at point i of line s.

    ``frames``: (T, H, W) uint8 or float32, a host array (a host array (S, T, L) comes back) or a ``DeviceFrames`` (a ``DeviceFrames``
    of shape (S, T, L) and dtype float32 comes back, the same bits).  ``lines``: (S, 4) rows (x0, y0, x1, y1) in pixels, every sample
    inside [0, W - 1] x [0, H - 1]; ``samples``: L >= 3 points per line, end points included.  ``out``: a space-time image
    (S, T_total, L) of the same kind to write rows ``[t_offset, t_offset + T)`` of -- the other rows are left alone, so a video that comes
    in chunks fills one image."""
    a = device.check_stack(frames, "stiv", side_min=2)
    T, H, W = a.shape
    ln, L = _check_lines(lines, samples)
    S = len(ln)
    pts = np.ascontiguousarray(line_points(ln, L))
    _check_points(pts, ln, H, W)
    if isinstance(t_offset, bool) or int(t_offset) != t_offset or int(t_offset) < 0:
        raise ValueError(f"t_offset {t_offset!r} must be an integer >= 0")
    t_offset = int(t_offset)
    dev = is_device(a)
    if out is None:
        if t_offset:
            raise ValueError(f"t_offset {t_offset} needs out, the space-time image it is a row of")
        out = DeviceFrames.empty((S, T, L), np.float32) if dev else np.empty((S, T, L), dtype=np.float32)
    elif not device.out_fits(out, dev, np.float32) or len(out.shape) != 3 or (out.shape[0], out.shape[2]) != (S, L) or out.shape[1] < t_offset + T:
        raise ValueError(f"out must be a writable C-contiguous float32 {'DeviceFrames' if dev else 'array'} of shape ({S}, >= {t_offset + T}, {L}), "
                         f"got {type(out).__name__} {getattr(out, 'shape', None)} {getattr(out, 'dtype', None)}")
    if T == 0 or S == 0:
        return out
    lib = _lib.load()
    _lib.require_device()
    code = _lib.DTYPE_CODES[np.dtype(a.dtype)]
    if dev:
        _lib.check(lib.lspiv_sti_gather_dev(a.c_ptr, code, T, H, W, _lib.ptr(pts), S, L, out.c_ptr, t_offset, out.shape[1], None))
    else:
        _lib.check(lib.lspiv_sti_gather(_lib.ptr(a), code, T, H, W, _lib.ptr(pts), S, L, _lib.ptr(out), t_offset, out.shape[1]))
    return out


def time_windows(T: int, L: int, time_window=None, time_stride=None, smooth: int = 1):
    """``(Tw, stride, K)`` of a space-time image of T rows and L columns: ``time_window`` defaults to T, ``time_stride`` to the window;
    K = (T - Tw) // stride + 1 windows, window k on rows k * stride .. k * stride + Tw - 1.  L and Tw must reach 2 * smooth + 3."""
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)):
        raise TypeError(f"smooth must be an integer, got {smooth!r}")
    if not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError(f"smooth {smooth!r} outside 0 .. {MAX_SMOOTH}")
    n = 2 * int(smooth) + 3
    for name, val in (("time_window", time_window), ("time_stride", time_stride)):
        if val is not None and (isinstance(val, bool) or int(val) != val):
            raise TypeError(f"{name} must be an integer, got {val!r}")
    Tw = int(T) if time_window is None else int(time_window)
    stride = Tw if time_stride is None else int(time_stride)
    if L < n:
        raise ValueError(f"{L} samples per line: smooth {smooth} needs {n}")
    if not n <= Tw <= T:
        raise ValueError(f"time_window {Tw} outside {n} .. {T} (smooth {smooth}, {T} frames)")
    if stride < 1:
        raise ValueError(f"time_stride {time_stride!r} < 1")
    return Tw, stride, (int(T) - Tw) // stride + 1


def orientation(sti, time_window: Optional[int] = None, time_stride: Optional[int] = None, smooth: int = 1,
                detrend: bool = True) -> Orientation:
    """The orientation of the streaks of every space-time image ``sti[s]`` ((S, T, L) float32, host array or ``DeviceFrames``) in windows
    of ``time_window`` rows (default: all T) every ``time_stride`` rows (default: the window), by the structure tensor.

    All arithmetic in float64.  ``detrend``: every column's mean over the window is taken off it first -- this removes everything static
    (bed texture, glare, banks), which otherwise pulls the slope towards zero.  ``smooth`` = k in 0 .. 3: k passes of the 3 x 3 binomial
    before the Sobel pair, as one (2k + 3) x (2k + 3) integer stencil; raise it on noisy footage."""
    if is_device(sti):
        a = sti
    else:
        a = np.asarray(sti)
    if len(a.shape) != 3:
        raise ValueError(f"sti must be (S, T, L), got shape {tuple(a.shape)}")
    if np.dtype(a.dtype) != np.float32:
        raise TypeError(f"sti must be float32, got {np.dtype(a.dtype)}")
    S, T, L = (int(q) for q in a.shape)
    Tw, stride, K = time_windows(T, L, time_window, time_stride, smooth)
    tensor, slope, coh = np.empty((S, K, 3)), np.empty((S, K)), np.empty((S, K))
    if S == 0:
        return Orientation(tensor, slope, coh)
    lib = _lib.load()
    _lib.require_device()
    if is_device(a):
        d_t, d_s, d_c = (device.buffer(nbytes=q.nbytes) for q in (tensor, slope, coh))
        _lib.check(lib.lspiv_sti_orientation_dev(a.c_ptr, S, T, L, Tw, stride, int(smooth), int(bool(detrend)), d_t.c_ptr, d_s.c_ptr, d_c.c_ptr, None))
        return Orientation(*(device.download(d, q.shape, np.float64) for d, q in ((d_t, tensor), (d_s, slope), (d_c, coh))))
    a = np.ascontiguousarray(a)
    _lib.check(lib.lspiv_sti_orientation(_lib.ptr(a), S, T, L, Tw, stride, int(smooth), int(bool(detrend)), _lib.ptr(tensor), _lib.ptr(slope),
                                         _lib.ptr(coh)))
    return Orientation(tensor, slope, coh)


def stiv(frames, lines, samples: int, time_window: Optional[int] = None, time_stride: Optional[int] = None, smooth: int = 1,
         detrend: bool = True, resolution: float = 1.0, dt: float = 1.0) -> Stiv:
    """``space_time_images`` then ``orientation``; ``v = slope * ds * resolution / dt`` with ``resolution`` in metres per pixel and ``dt``
    the seconds between two frames: the velocity along each line (S, K), positive from its point 0 towards its last point.

    Lay the lines along the flow and choose the spacing so that |slope| stays below about 2 samples per frame (INTEGRATION.md
    section 2m has the limits); ``coherency`` tells how far a window had one orientation at all."""
    resolution, dt = float(resolution), float(dt)
    if not (np.isfinite(resolution) and resolution > 0.0):
        raise ValueError(f"resolution {resolution!r} must be positive")
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError(f"dt {dt!r} must be positive")
    a = device.check_stack(frames, "stiv", side_min=2)
    ln, L = _check_lines(lines, samples)
    time_windows(a.shape[0], L, time_window, time_stride, smooth)      # the window errors before any work
    o = orientation(space_time_images(a, ln, L), time_window, time_stride, smooth, detrend)
    ds = line_spacing(ln, L)
    return Stiv(o.slope * ds[:, None] * resolution / dt, o.slope, o.coherency, o.tensor, ds)
