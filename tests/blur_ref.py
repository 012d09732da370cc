"""Float64 reference of ``smooth`` / ``edge_detect`` and the cases of the tests built on it.  TEST INFRASTRUCTURE, CPU only: nothing here
imports the library.

The reference is the filter the library restates (cv2.GaussianBlur(img.astype("float32"), (k, k), 0): the float32 taps of
``oracle.filters_oracle.gaussian_kernel``, rows then columns, BORDER_REFLECT_101, symmetric evaluation) with EVERY operation in float64,
so its own error (a few 2^-53 of the range) is nothing next to a float32 kernel's.  ``gate`` says how far a CORRECT float32 kernel can be
from it; it is derived from the number of roundings, not from what any kernel gave:

  * a 1-D pass of radius R computes k0*x0 + sum_j kj*(x[-j] + x[+j]) -- per output and term one rounding, and the taps are non-negative
    and sum to 1, so the error of the pass is at most (R + 2) u max|x| with u = 2^-24 (a fused multiply-add only removes roundings);
  * two passes double that; the float32 taps themselves are allowed 1 u max|x| per pass;
  * smooth: (2 (R + 2) + 2) u max|x|; edge_detect: (2 (Ra + 2) + 2 (Rb + 2) + 3) u max|x| (two filters, their taps, the subtraction);
  * max|x| over the finite samples of the frame, floored at 1.  For k = 31 that is 2.1e-6 of the range;
  * uint8 frames at windows <= 3 (OpenCV's dyadic tables for k = 1, 3, 5, 7): every float32 operation of either pass is exact (integers
    below 2^20 over 4096), so the gate is 0 -- EQUALITY with the reference;
  * the clip is 1-Lipschitz: the same gate after it.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle.filters_oracle import gaussian_kernel

U = 2.0 ** -24


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _pass(x: np.ndarray, k: np.ndarray, axis: int) -> np.ndarray:
    r = len(k) // 2
    idx = np.arange(x.shape[axis])
    out = k[r] * x
    for j in range(1, r + 1):                                       # only the taps within the radius: none is multiplied by zero
        out = out + k[r + j] * (np.take(x, _reflect101(idx - j, len(idx)), axis=axis) + np.take(x, _reflect101(idx + j, len(idx)), axis=axis))
    return out


def blur(img, ksize: int) -> np.ndarray:
    """(..., H, W) -> float64, the last two axes filtered.  The frame is narrowed to float32 first, like the reference and the library do."""
    a = np.asarray(img).astype(np.float32).astype(np.float64)
    k = gaussian_kernel(ksize).astype(np.float64)
    with np.errstate(invalid="ignore"):                             # Inf - Inf where both signs meet
        return _pass(_pass(a, k, -1), k, -2)


def smooth(frames, wdw: int) -> np.ndarray:
    return blur(frames, 2 * wdw + 1)


def edge_detect(frames, w1: int, w2: int) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return blur(frames, 2 * w2 + 1) - blur(frames, 2 * w1 + 1)


def clip(x, lo, hi) -> np.ndarray:
    """Frames.minmax: NaN stays NaN."""
    return np.maximum(np.minimum(x, hi), lo)


def max_abs(frames) -> np.ndarray:
    """max|x| over the finite samples of every frame (as float32), floored at 1: (T, 1, 1)."""
    a = np.abs(np.asarray(frames).astype(np.float32).astype(np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    return np.maximum(a.reshape(a.shape[0], -1).max(axis=1), 1.0)[:, None, None]


def gate(w1: int, w2, max_abs, dtype=None):
    """The largest |kernel - reference| of a correct float32 kernel (module docstring); 0 -- equality -- for uint8 frames at windows <= 3."""
    if dtype is not None and np.dtype(dtype) == np.uint8 and max(w1, w2 or 0) <= 3:
        return 0.0 * max_abs
    n = 2 * (w1 + 2) + 2 if w2 is None else 2 * (w1 + 2) + 2 * (w2 + 2) + 3
    return n * U * max_abs


def family(dtype, w1: int, w2, W: int) -> str:
    """The kernel family the library runs: launch_blur_clip in pyorc_amd/csrc/filters.hip restated, for aligned buffers and no A/B
    switch in the environment.  Every GPU test asserts the family it means to reach through this function: when the dispatch rule
    changes, restate it here and the tests say which of them no longer cover what they claim."""
    edge = w2 is not None
    R = w2 if edge else w1
    unrolled = (R <= 3 and 1 <= w1 < R) if edge else (1 <= w1 <= 3)
    if unrolled:
        return "strip4" if np.dtype(dtype) == np.uint8 and W % 4 == 0 and W >= 12 else "strip"
    if R <= 5:
        return "stripr5"
    return "stripr10" if R <= 10 else "ring"


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_blur_reference.py (tests/test_blur_ref_host.py runs the float32 oracle over the same stacks)
# ---------------------------------------------------------------------------------------------------------------------------------
# windows: an int is smooth(wdw), a pair edge_detect(w1, w2); the value is the family the case means to reach
UNROLLED = (1, 2, 3, (1, 2), (1, 3), (2, 3))
RUNTIME = {4: "stripr5", 5: "stripr5", 6: "stripr10", 10: "stripr10", (2, 4): "stripr5", (6, 10): "stripr10", (1, 5): "stripr5",
           (0, 4): "stripr5", (5, 5): "stripr5"}
RING = (11, 15, (11, 15), (3, 12))
F, U8 = ("float32", "float64"), ("uint8",)
# row of the table -> (windows with their family, [(shape, dtypes)]): the smallest shapes at which each kernel can still go wrong
TABLE = {
    "strip": ({w: "strip" for w in UNROLLED}, [
        ((2, 130, 67), F + U8),       # second block row (4 x 32 rows), a 2-row last strip below the halo, a 3-column last tile
        ((1, 33, 64), F), ((1, 2, 70), F + U8), ((1, 1, 1), F + U8), ((1, 3, 129), F + U8)]),
    "strip4": ({w: "strip4" for w in UNROLLED}, [
        ((1, 1, 12), U8), ((2, 2, 16), U8), ((1, 3, 260), U8),    # below the halo in an edge-only block, and in edge + interior + edge
        ((1, 34, 516), U8),           # the last interior block ends exactly at W
        ((1, 130, 264), U8), ((1, 32, 256), U8)]),
    "stripr": (RUNTIME, [
        ((1, 258, 70), F + U8),       # second block row (4 x 64 rows) with a 2-row strip
        ((2, 65, 64), F + U8), ((1, 64, 130), F + U8), ((1, 7, 9), F + U8), ((1, 1, 1), F + U8)]),
    "ring": ({w: "ring" for w in RING}, [
        ((1, 130, 70), F + U8),       # second block row (4 x 32 rows)
        ((2, 33, 65), F + U8), ((1, 29, 31), F + U8), ((1, 5, 7), F + U8)]),   # reflect101 wraps once / several times
}


def split(w):
    """A window spec -> (w1, w2 or None)."""
    return (w, None) if isinstance(w, int) else (w[0], w[1])


def _scaled(x: np.ndarray, dtype: str) -> np.ndarray:
    return x if dtype == "uint8" else x.astype(dtype) * 0.41 - 7       # |x| <= 1e4: nothing overflows in float32 that does not in float64


@functools.lru_cache(maxsize=None)
def stack(shape, dtype: str) -> np.ndarray:
    """The small random stack of a table case (read-only: shared between the tests)."""
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
    a = _scaled(rng.integers(0, 256, shape, dtype=np.uint8), dtype)
    a.setflags(write=False)
    return a


# non-finite samples, one mid-size shape for every family: (frame, y, x) of the NaNs -- interior, within R of a corner (the reflection
# doubles it), in the halo rows between two strips (`seam` - 1 in frame 0, `seam` in frame 1), in the halo columns between two
# 64-column tiles -- and of one +Inf and one -Inf whose supports are disjoint from each other's and from the NaNs' up to R = 15
NONFINITE_SHAPE = (2, 130, 140)
SEAM = {"strip": 32, "stripr": 64, "ring": 32}                       # first row of the second strip of a wave


def nonfinite_points(row: str):
    s = SEAM[row]
    nans = [(0, 60, 100), (0, 1, 1), (1, 1, 1), (0, s - 1, 40), (1, s, 40), (0, 100, 63), (1, 100, 64)]
    return nans, [(t, 95, 20) for t in (0, 1)], [(t, 20, 105) for t in (0, 1)]


@functools.lru_cache(maxsize=None)
def nonfinite_stack(row: str, dtype: str) -> np.ndarray:
    a = stack(NONFINITE_SHAPE, dtype).copy()
    nans, pinf, ninf = nonfinite_points(row)
    for pts, v in ((nans, np.nan), (pinf, np.inf), (ninf, -np.inf)):
        for p in pts:
            a[p] = v
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames_stack(dtype: str) -> np.ndarray:
    """T = 3 with a different constant per frame: a wrong frame offset shows."""
    base = np.random.default_rng(77).integers(0, 100, (3, 70, 132), dtype=np.uint8) + np.array([0, 60, 120], np.uint8)[:, None, None]
    a = _scaled(base, dtype)
    a.setflags(write=False)
    return a


STACKS = {"table": stack, "nonfinite": nonfinite_stack, "frames": lambda key, dtype: frames_stack(dtype)}


@functools.lru_cache(maxsize=None)
def reference(kind: str, key, dtype: str, w, lo=None, hi=None) -> np.ndarray:
    """The float64 reference of a case, computed once: kind "table" (key: shape), "nonfinite" (key: table row), "frames" (key: None)."""
    fr = STACKS[kind](key, dtype)
    w1, w2 = split(w)
    ref = smooth(fr, w1) if w2 is None else edge_detect(fr, w1, w2)
    if lo is not None:
        ref = clip(ref, np.float64(np.float32(lo)), np.float64(np.float32(hi)))
    ref.setflags(write=False)
    return ref


def compare(got: np.ndarray, ref: np.ndarray, frames: np.ndarray, w):
    """(the NaN, +Inf and -Inf masks are the reference's, largest |got - ref| / gate over the finite outputs).  Where the gate is 0 the
    ratio is 0 for equal values and inf otherwise."""
    w1, w2 = split(w)
    masks = (got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == np.inf, ref == np.inf)
             and np.array_equal(got == -np.inf, ref == -np.inf))
    if not masks:
        return False, np.inf
    fin = np.isfinite(ref)
    g = np.broadcast_to(gate(w1, w2, max_abs(frames), frames.dtype), ref.shape)[fin]
    err = np.abs(got.astype(np.float64)[fin] - ref[fin])
    if err.size == 0:
        return True, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / g)
    return True, float(ratio.max())
