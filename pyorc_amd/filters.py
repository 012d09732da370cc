"""Mirror of the element-wise ``Frames`` filters of pyorc on the MI355X.

``normalize`` (pyorc/api/frames.py:279-306), ``minmax`` (:344-362) and ``time_diff`` (:409-436) are plain
numpy/xarray arithmetic in the reference and are reproduced bit for bit.  ``smooth`` (:438-467) and ``edge_detect``
(:308-342) are ``cv2.GaussianBlur`` calls (pyorc/cv.py:142-183): OpenCV cannot be installed here, so its published
algorithm is restated (coefficient tables, separable float32 filter, BORDER_REFLECT_101) -- expect ~1e-6 agreement
with a real cv2, not bit identity.
"""

from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from .device import DeviceFrames, is_device


def time_diff(frames, thres: float = 0.0, abs: bool = False) -> np.ndarray:
    """``Frames.time_diff``: (T, H, W) -> (T-1, H, W) float32; values <= thres (and NaN) become 0.
    A ``DeviceFrames`` stack stays in HBM (``lspiv_time_diff_dev``) -- so do all the filters below."""
    if is_device(frames):
        T, H, W = frames.shape
        out = DeviceFrames.empty((T - 1, H, W), np.float32)
        _lib.check(_lib.load().lspiv_time_diff_dev(frames.c_ptr, frames.dtype_code, T, H, W, float(thres), int(bool(abs)), out.c_ptr, None))
        return out
    a = _lib.as_frames(frames)
    _lib.require_device()
    out = np.empty((a.shape[0] - 1,) + a.shape[1:], dtype=np.float32)
    _lib.check(_lib.load().lspiv_time_diff(_lib.ptr(a), _lib.DTYPE_CODES[a.dtype], a.shape[0], a.shape[1], a.shape[2],
                                           float(thres), int(bool(abs)), _lib.ptr(out)))
    return out


def reduce_rolling(frames, samples: int = 25) -> np.ndarray:
    """``Frames.reduce_rolling`` on uint8 frames: trailing rolling mean of ``samples`` frames removed, clipped at 0,
    per-frame stretch to uint8 (the first ``samples - 1`` frames have no complete window and come out 0)."""
    a = frames if is_device(frames) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("reduce_rolling expects a (T, H, W) uint8 stack (grayscale camera frames)")
    if len(a) < samples:
        raise AssertionError(f"Amount of frames is smaller than requested rolling of {samples} samples")
    if is_device(a):
        out = DeviceFrames.empty(a.shape, np.uint8)
        _lib.check(_lib.load().lspiv_reduce_rolling_dev(a.c_ptr, a.shape[0], a.shape[1], a.shape[2], int(samples), out.c_ptr, None))
        return out
    a = np.ascontiguousarray(a)
    _lib.require_device()
    out = np.empty_like(a)
    _lib.check(_lib.load().lspiv_reduce_rolling(_lib.ptr(a), a.shape[0], a.shape[1], a.shape[2], int(samples), _lib.ptr(out)))
    return out


def range(frames) -> np.ndarray:  # noqa: A001 -- the reference's method name
    """``Frames.range``: (T, H, W) -> (H, W) in the frames' own dtype, maximum minus minimum through time (NaN skipped)."""
    if is_device(frames):
        out = np.empty(frames.shape[1:], dtype=frames.dtype)
        d_out = DeviceFrames.empty((1,) + frames.shape[1:], frames.dtype)
        _lib.check(_lib.load().lspiv_time_range_dev(frames.c_ptr, frames.dtype_code, *frames.shape, d_out.c_ptr, None))
        return d_out.to_host()[0]
    a = _lib.as_frames(frames)
    _lib.require_device()
    out = np.empty(a.shape[1:], dtype=a.dtype)
    _lib.check(_lib.load().lspiv_time_range(_lib.ptr(a), _lib.DTYPE_CODES[a.dtype], a.shape[0], a.shape[1], a.shape[2], _lib.ptr(out)))
    return out


def minmax(frames, min=-np.inf, max=np.inf) -> np.ndarray:
    """``Frames.minmax`` on float32 frames: ``np.maximum(np.minimum(x, max), min)`` (NaN propagates)."""
    if is_device(frames):
        if frames.dtype != np.float32:
            raise ValueError("minmax on a device stack expects float32 frames (the output of edge_detect / smooth / time_diff)")
        out = DeviceFrames.empty(frames.shape, np.float32)
        _lib.check(_lib.load().lspiv_minmax_dev(frames.c_ptr, int(np.prod(frames.shape)), float(min), float(max), out.c_ptr, None))
        return out
    a = np.ascontiguousarray(frames, dtype=np.float32)
    _lib.require_device()
    out = np.empty_like(a)
    _lib.check(_lib.load().lspiv_minmax(_lib.ptr(a), a.size, float(min), float(max), _lib.ptr(out)))
    return out


def normalize(frames, samples: int = 15) -> np.ndarray:
    """``Frames.normalize`` on uint8 frames: sampled temporal mean removed, per-frame stretch to uint8."""
    a = frames if is_device(frames) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("normalize expects a (T, H, W) uint8 stack (grayscale camera frames)")
    if round(len(a) / samples) == 0:
        raise AssertionError(f"Amount of frames is too small to provide {samples} samples")
    if is_device(a):
        out = DeviceFrames.empty(a.shape, np.uint8)
        _lib.check(_lib.load().lspiv_normalize_dev(a.c_ptr, a.shape[0], a.shape[1], a.shape[2], int(samples), out.c_ptr, None))
        return out
    a = np.ascontiguousarray(a)
    _lib.require_device()
    out = np.empty_like(a)
    _lib.check(_lib.load().lspiv_normalize(_lib.ptr(a), a.shape[0], a.shape[1], a.shape[2], int(samples), _lib.ptr(out)))
    return out


def _blur(frames, k1: int, k2: int) -> np.ndarray:
    if is_device(frames):
        T, H, W = frames.shape
        out = DeviceFrames.empty(frames.shape, np.float32)
        lib = _lib.load()
        if k2:
            rc = lib.lspiv_edge_detect_dev(frames.c_ptr, frames.dtype_code, T, H, W, k1, k2, out.c_ptr, None)
        else:
            rc = lib.lspiv_gaussian_blur_dev(frames.c_ptr, frames.dtype_code, T, H, W, k1, out.c_ptr, None)
        _lib.check(rc)
        return out
    a = np.asarray(frames)
    single = a.ndim == 2
    a = _lib.as_frames(a[None] if single else a)
    _lib.require_device()
    out = np.empty(a.shape, dtype=np.float32)
    lib = _lib.load()
    if k2:
        rc = lib.lspiv_edge_detect(_lib.ptr(a), _lib.DTYPE_CODES[a.dtype], a.shape[0], a.shape[1], a.shape[2], k1, k2, _lib.ptr(out))
    else:
        rc = lib.lspiv_gaussian_blur(_lib.ptr(a), _lib.DTYPE_CODES[a.dtype], a.shape[0], a.shape[1], a.shape[2], k1, _lib.ptr(out))
    _lib.check(rc)
    return out[0] if single else out


def smooth(frames, wdw: int = 1) -> np.ndarray:
    """``Frames.smooth``: Gaussian blur with a (2 wdw + 1)^2 kernel, float32."""
    return _blur(frames, 2 * int(wdw) + 1, 0)


def edge_detect(frames, wdw_1: int = 1, wdw_2: int = 2) -> np.ndarray:
    """``Frames.edge_detect``: blur(2 wdw_2 + 1) - blur(2 wdw_1 + 1), float32."""
    return _blur(frames, 2 * int(wdw_1) + 1, 2 * int(wdw_2) + 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recipe's frame filters as one chain on the device
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN_OPS = ("normalize", "edge_detect", "minmax", "smooth")
_CHAIN_LOCK = threading.Lock()   # lspiv_normalize_apply_dev keeps its temporaries in the context's scratch: one caller's launches at a time


class Chain:
    """``Frames`` filter calls ``[(op, params), ...]`` (the reference's names and parameters: ``normalize(samples)``,
    ``edge_detect(wdw_1, wdw_2)``, ``minmax(min, max)``, ``smooth(wdw)``) as the sequence of ``*_dev`` entry points that computes them
    on a piece of a uint8 camera stack.  The one place that knows that sequence: ``pipeline.CameraToVelocity`` and the resident stack of
    ``velocimetry.get_ffpiv`` (``pyorc_amd.resident``) both run it.

    * ``normalize`` first, against a mean plane computed once for the whole stack (:meth:`mean_plane`): ``lspiv_normalize_apply_dev``;
    * ``edge_detect`` and a ``minmax`` right after it: ONE ``lspiv_edge_detect_clip_dev`` call (the bits of the two);
    * ``smooth``: ``lspiv_gaussian_blur_dev``;
    * any other ``minmax`` (on float32 frames): ``lspiv_minmax_dev``, in place.

    At most one Gaussian stage, so a piece needs one uint8 scratch stack (with ``normalize``) and one float32 one (with a Gaussian
    stage): :attr:`scratch_bytes_per_pixel`."""

    def __init__(self, ops):
        self.ops = tuple((str(op), dict(p)) for op, p in ops)
        self.steps = []
        self.samples = None
        floats = False
        for i, (op, p) in enumerate(self.ops):
            if op == "normalize":
                if i != 0:
                    raise ValueError("normalize works on the uint8 camera frames: first in the chain")
                self.samples = int(p["samples"])
                self.steps.append(["normalize"])
            elif op in ("edge_detect", "smooth"):
                if floats:
                    raise ValueError("one Gaussian stage per chain")
                floats = True
                if op == "edge_detect":
                    self.steps.append(["edge", 2 * int(p["wdw_1"]) + 1, 2 * int(p["wdw_2"]) + 1, -np.inf, np.inf, False])
                else:
                    self.steps.append(["smooth", 2 * int(p["wdw"]) + 1])
            elif op == "minmax":
                if not floats:
                    raise ValueError("minmax in the chain works on float32 frames (after edge_detect or smooth)")
                lo, hi = float(p["min"]), float(p["max"])
                last = self.steps[-1]
                if last[0] == "edge" and not last[5]:
                    last[3:] = [lo, hi, True]       # rides in the filter's store
                else:
                    self.steps.append(["minmax", lo, hi])
            else:
                raise ValueError(f"no device chain for Frames.{op}")
        self.float_out = floats

    @property
    def names(self):
        return [op for op, _ in self.ops]

    @property
    def scratch_bytes_per_pixel(self) -> int:
        """Bytes per camera pixel a piece occupies in HBM while it runs: the upload, plus the stages' outputs."""
        return 1 + (1 if self.samples else 0) + (4 if self.float_out else 0)

    def mean_plane(self, sampled) -> DeviceFrames:
        """The float32 mean plane ``normalize`` removes, from the SAMPLED frames only (``frames[::round(T / samples)]`` of the whole
        stack, uint8): ``lspiv_normalize_mean_dev`` over that compact stack with every frame sampled -- integer sums, so the bits of
        the whole-stack mean.  A ``(1, H, W)`` ``DeviceFrames``."""
        d = sampled if is_device(sampled) else DeviceFrames.from_host(np.ascontiguousarray(sampled, dtype=np.uint8))
        n, H, W = d.shape
        mean = DeviceFrames.empty((1, H, W), np.float32)
        _lib.check(_lib.load().lspiv_normalize_mean_dev(d.c_ptr, n, H, W, n, mean.c_ptr, None))
        return mean

    def run_dev(self, d_src: int, T: int, H: int, W: int, d_mean=None, d_u8=None, d_f32=None, stream=None):
        """Device pointers: ``T`` uint8 frames at ``d_src`` through the chain; ``d_u8`` / ``d_f32`` receive the uint8 / float32 stages'
        outputs (``T * H * W`` samples each; needed with ``normalize`` / a Gaussian stage), ``d_mean`` is :meth:`mean_plane`'s.  Kernels
        on ``stream`` (None: the library's).  Returns (pointer, dtype) of the chain's output."""
        lib = _lib.load()
        vp = lambda p: None if p is None else C.c_void_p(int(p))      # noqa: E731
        src, dt = int(d_src), np.dtype(np.uint8)
        s = vp(stream)
        with _CHAIN_LOCK:
            for step in self.steps:
                kind = step[0]
                if kind == "normalize":
                    _lib.check(lib.lspiv_normalize_apply_dev(vp(src), T, H, W, vp(d_mean), vp(d_u8), s))
                    src = int(d_u8)
                elif kind == "edge":
                    _lib.check(lib.lspiv_edge_detect_clip_dev(vp(src), _lib.DTYPE_CODES[dt], T, H, W, step[1], step[2], step[3], step[4],
                                                              vp(d_f32), s))
                    src, dt = int(d_f32), np.dtype(np.float32)
                elif kind == "smooth":
                    _lib.check(lib.lspiv_gaussian_blur_dev(vp(src), _lib.DTYPE_CODES[dt], T, H, W, step[1], vp(d_f32), s))
                    src, dt = int(d_f32), np.dtype(np.float32)
                else:
                    _lib.check(lib.lspiv_minmax_dev(vp(src), T * H * W, step[1], step[2], vp(src), s))
        return src, dt

    def apply(self, frames: DeviceFrames, mean=None) -> DeviceFrames:
        """A ``DeviceFrames`` piece of uint8 camera frames through the chain, on the library's stream; scratch from the pool, per call
        (the resident stack's loader threads stage pieces side by side).  Returns the output stack."""
        T, H, W = frames.shape
        if frames.dtype != np.uint8:
            raise ValueError(f"the chain starts on uint8 camera frames, got {frames.dtype}")
        if self.samples and mean is None:
            raise ValueError("normalize needs the stack's mean plane (Chain.mean_plane)")
        u8 = DeviceFrames.empty(frames.shape, np.uint8) if self.samples else None
        f32 = DeviceFrames.empty(frames.shape, np.float32) if self.float_out else None
        self.run_dev(frames.ptr, T, H, W, None if mean is None else mean.ptr, None if u8 is None else u8.ptr,
                     None if f32 is None else f32.ptr)
        return f32 if f32 is not None else (u8 if u8 is not None else frames)
