"""Frame stabilisation: camera shake estimated by PIV on the static part of the image, every frame warped back onto frame 0.

What pyorc does in ``Video(stabilize=...)`` (pyorc/cv.py: feature tracks on the banks, ``cv2.warpAffine`` per frame on the CPU) so that a
handheld, drone or pole-mounted video can enter the fixed-camera chain ``normalize -> project -> get_piv`` at all.  Here the masked
per-pair PIV kernels under a static mask of the banks are the motion sensor, and three kernels follow them:

    tr = stabilize.estimate(frames, stable_mask)          # Transforms: .A (T, 2, 3), .pairwise, .n_used, .carry
    steady = stabilize.warp(frames, tr.A)                 # same kind of stack as ``frames``: host array or DeviceFrames
    steady, tr = stabilize.stabilize(frames, stable_mask)

The semantics are this project's own -- unpinned against pyorc and OpenCV; tests/stabilize_ref.py is their float64 numpy statement.
A long video runs in chunks with a one-frame halo: ``estimate(frames[a:b + 1], mask, carry=previous.carry)`` continues the chain, bit
for bit what one call over the whole stack gives.
"""

from __future__ import annotations

import warnings
from typing import NamedTuple, Optional

import numpy as np

from . import _lib, device, piv
from .device import DeviceFrames, is_device

WINDOWS = (16, 32, 64)
MODELS = {"translation": 0, "similarity": 1, "affine": 2}


class Transforms(NamedTuple):
    """``A`` (T, 2, 3) float64: A[t] maps a pixel (x, y, 1) of the reference frame (frame 0 of the run) to its position in frame t;
    ``pairwise`` (T - 1, 2, 3): P[t] with x_{t+1} = P[t] (x_t, y_t, 1) for a static point; ``n_used`` (T - 1,) int32: vectors of the last
    round of each fit, 0 where the fit fell back to the identity; ``carry`` (2, 3): the pose at the last frame, the next chunk's ``carry``."""
    A: np.ndarray
    pairwise: np.ndarray
    n_used: np.ndarray
    carry: np.ndarray


def estimate(frames, stable_mask, window_size: int = 32, overlap: Optional[int] = None, model: str = "similarity",
             mask_coverage_min: float = 0.5, reject=(2.0, 0.5), min_vectors: int = 6, carry=None) -> Transforms:
    """The pose of every frame of ``frames`` (T, H, W) relative to its first one, from the displacement of the image under ``stable_mask``
    ((H, W), non-zero = does not move in the world: banks, buildings, rocks).

    Vectors: ``piv.piv_pairs_masked`` with square windows of ``window_size`` (16, 32 or 64) px at ``overlap`` (default half a window) under
    the mask, windows with less than ``mask_coverage_min`` of their samples on it dropped.  Per pair a least-squares fit of ``model``
    ("translation", "similarity" -- shift, rotation, scale; the default -- or "affine") in three rounds: all finite vectors, those within
    ``reject[0]`` px of the first fit, those within ``reject[1]`` px of the second.  A pair left with fewer than ``min_vectors`` vectors, or
    with vectors that do not determine the model (one row of windows under "affine"), gets the identity and ``n_used`` 0 -- warned about
    once per call.  ``carry``: the pose (2, 3) of the first frame, ``Transforms.carry`` of the chunk before (default: the identity).
    The shake between two frames must stay below about half a window less the width of the correlation peak."""
    lib = _lib.load()
    a = device.check_stack(frames, "stabilize")
    T, H, W = a.shape
    n = int(window_size)
    if n not in WINDOWS or n != window_size:
        raise ValueError(f"window_size {window_size!r} not in {WINDOWS}")
    o = n // 2 if overlap is None else int(overlap)
    if not 0 <= o < n:
        raise ValueError(f"overlap {overlap!r} outside 0 .. {n - 1}")
    if model not in MODELS:
        raise ValueError(f"unknown model {model!r}: one of {tuple(MODELS)}")
    try:
        r0, r1 = (float(q) for q in reject)
    except (TypeError, ValueError):
        raise ValueError(f"reject must be two numbers, got {reject!r}") from None
    if not (r1 > 0.0 and r0 > r1 and np.isfinite(r0)):
        raise ValueError(f"reject {reject!r} must be positive and decreasing")
    if int(min_vectors) < 1:
        raise ValueError(f"min_vectors {min_vectors!r} < 1")
    mask = np.asarray(stable_mask)
    if mask.shape != (H, W):
        raise ValueError(f"stable_mask has shape {mask.shape}, the frames are {(H, W)}")
    if T < 2:
        raise ValueError(f"need at least 2 frames, got {T}")
    carry_in = None
    if carry is not None:
        carry_in = np.ascontiguousarray(carry, dtype=np.float64)
        if carry_in.shape != (2, 3):
            raise ValueError(f"carry must have shape (2, 3), got {carry_in.shape}")
    u, v = piv.piv_pairs_masked(a, (n, n), (o, o), image_mask=mask, mask_coverage_min=mask_coverage_min)[:2]
    if _lib.get_option("v_sign"):    # the fit wants the row shift, rows downward: the option is undone once, and left as it is
        v = -v
    P_, rows, cols = u.shape
    # vectors up, fit -> chain on the library's stream, transforms down: no host round trip between the two kernels
    d_u, d_v = device.buffer(np.ascontiguousarray(u)), device.buffer(np.ascontiguousarray(v))
    d_P, d_n, d_A, d_c = (device.buffer(nbytes=q) for q in (P_ * 48, P_ * 4, T * 48, 48))
    d_carry = device.buffer(carry_in) if carry_in is not None else None
    _lib.check(lib.lspiv_stabilize_fit_dev(d_u.c_ptr, d_v.c_ptr, P_, rows, cols, n, o, o, H, W, MODELS[model], r0, r1, int(min_vectors),
                                           d_P.c_ptr, d_n.c_ptr, None))
    _lib.check(lib.lspiv_stabilize_chain_dev(d_P.c_ptr, P_, None if d_carry is None else d_carry.c_ptr, d_A.c_ptr, d_c.c_ptr, None))
    tr = Transforms(device.download(d_A, (T, 2, 3), np.float64), device.download(d_P, (P_, 2, 3), np.float64), device.download(d_n, (P_,), np.int32),
                    device.download(d_c, (2, 3), np.float64))
    if (tr.n_used == 0).any():
        warnings.warn(f"stabilize.estimate: {int((tr.n_used == 0).sum())} of {P_} pairs had too few consistent vectors on the stable mask "
                      f"for model {model!r}; their transform is the identity", RuntimeWarning, stacklevel=2)
    return tr


def warp(frames, A, out=None):
    """``out[t](y, x)`` = the bilinear sample of ``frames[t]`` at ``A[t] (x, y, 1)`` (1/32 px, neighbours outside the frame count as 0): with
    ``Transforms.A`` every frame comes to lie on frame 0.  ``frames``: (T, H, W) uint8 or float32, a host array (a host array comes back)
    or a ``DeviceFrames`` (a ``DeviceFrames`` comes back, the same bits); ``A``: (T, 2, 3).  ``out``: a stack of the same kind, shape and
    dtype to write into (not ``frames`` itself)."""
    lib = _lib.load()
    a = device.check_stack(frames, "stabilize")
    T, H, W = a.shape
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.shape != (T, 2, 3):
        raise ValueError(f"A must have shape {(T, 2, 3)}, got {A.shape}")
    dev = is_device(a)
    if out is None:
        out = DeviceFrames.empty(a.shape, a.dtype) if dev else np.empty(a.shape, dtype=a.dtype)
    elif not device.out_fits(out, dev, a.dtype) or tuple(out.shape) != a.shape:
        raise ValueError(f"out must be a writable C-contiguous {'DeviceFrames' if dev else 'array'} of shape {a.shape} and dtype {a.dtype}")
    if T == 0:
        return out
    _lib.require_device()
    code = _lib.DTYPE_CODES[np.dtype(a.dtype)]
    if dev:
        d_A = device.buffer(A)
        _lib.check(lib.lspiv_warp_affine_dev(a.c_ptr, code, T, H, W, d_A.c_ptr, out.c_ptr, None))
    else:
        if np.shares_memory(a, out):
            raise ValueError("out must not overlap frames")
        _lib.check(lib.lspiv_warp_affine(_lib.ptr(a), code, T, H, W, _lib.ptr(A), _lib.ptr(out)))
    return out


def stabilize(frames, stable_mask, **kw):
    """``(warp(frames, tr.A), tr)`` for ``tr = estimate(frames, stable_mask, **kw)``."""
    tr = estimate(frames, stable_mask, **kw)
    return warp(frames, tr.A), tr
