"""Mirror of ``ffpiv.window`` for the call sites on pyorc's PIV path.

Reference call sites: pyorc/api/frames.py:85-90 (``get_rect_coordinates``), :167
(``round_to_even``); pyorc/velocimetry/ffpiv.py:120-126 (``required_memory``), :129
(``available_memory``).  The grid functions call the C ABI (host-only code in
liblspiv_hip.so, no GPU needed); the memory functions answer for HBM instead of host RAM,
because that is what bounds a chunk on the ``hip`` engine.
"""

from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib


def round_to_even(input_tuple: Sequence[float]) -> Tuple[int, ...]:
    """Round window sizes to even integers (pyorc/api/frames.py:167).  The direction for odd sizes is the
    library option ``round_odd``: 0 round-half-even of x / 2 (25 -> 24, 27 -> 28; default), 1 up, 2 down."""
    mode = _lib.get_option("round_odd")
    if mode == 1:
        return tuple(int(np.ceil(float(x) / 2.0) * 2) for x in input_tuple)
    if mode == 2:
        return tuple(int(np.floor(float(x) / 2.0) * 2) for x in input_tuple)
    return tuple(int(np.round(float(x) / 2.0) * 2) for x in input_tuple)


SEARCH_AREAS = (16, 32, 64)


class SearchWindow(tuple):
    """A window searched inside a larger search area, as ONE window argument of the layers below ``get_ffpiv`` / ``piv_pairs``: the tuple
    itself is the SEARCH AREA ``(say, sax)`` -- which lays out the grid, the correlation planes and the memory plan, so every
    function that takes a window size answers for the search area --, ``.window`` the ``(wy, wx)`` cut from frame t."""

    def __new__(cls, search_area, window):
        self = super().__new__(cls, (int(search_area[0]), int(search_area[1])))
        self.window = (int(window[0]), int(window[1]))
        return self


def search_spec(window_size, search_area_size=None):
    """``window_size`` as the layers below take it: the plain tuple when there is no search area of its own (None, or equal to the
    window: today's path), else a validated :class:`SearchWindow`.  Host-only.  Supported: a square search area of 16, 32 or 64 px
    with a square even window, 4 <= window <= search area - 2; not with the option ``norm_clip`` = 0."""
    if isinstance(window_size, SearchWindow):
        return window_size
    ws = (int(window_size[0]), int(window_size[1]))
    if search_area_size is None or (int(search_area_size[0]), int(search_area_size[1])) == ws:
        return ws
    sa = (int(search_area_size[0]), int(search_area_size[1]))
    if not _lib.load().lspiv_search_supported(sa[0], sa[1], ws[0], ws[1]):
        raise ValueError(f"search_area_size {sa} with window_size {ws} is not supported: the search area must be square and one of "
                         f"{SEARCH_AREAS}, the window square and even with 4 <= window <= search area - 2 (or search_area_size == "
                         "window_size)")
    if _lib.get_option("norm_clip") == 0:
        raise ValueError("option norm_clip = 0 is served by the block-per-window kernels only, not with a search_area_size "
                         "larger than the window")
    return SearchWindow(sa, ws)


SHIFT_WINDOWS = (16, 32, 64)
MAX_PASSES = 8
DEFORM_WINDOWS = (16, 32, 64)
MAX_DEFORM_PASSES = 4


class MultiPassWindow(tuple):
    """A chain of passes as ONE window argument of the layers below ``get_ffpiv`` / ``piv_pairs``: the tuple
    itself is the FINAL pass's window ``(n, n)`` -- which lays out the grid and the result --, ``.passes`` every pass ``(n_k, overlap_k)``,
    coarsest first, the final one last.  The chunk alignment is pass 0's, the memory plan answers for the whole chain.  ``.deform``:
    the window deformation passes that follow the chain on the final grid (0: none)."""

    def __new__(cls, passes, deform: int = 0):
        passes = tuple((int(n), int(o)) for n, o in passes)
        self = super().__new__(cls, (passes[-1][0], passes[-1][0]))
        self.passes = passes
        self.deform = int(deform)
        return self

    @property
    def overlap(self):
        return (self.passes[-1][1], self.passes[-1][1])


def deform_count(deform_passes) -> int:
    """The ``deform_passes`` keyword checked: None or a whole number 0 .. 4 -> the count.  Host-only."""
    if deform_passes is None:
        return 0
    if isinstance(deform_passes, bool) or not isinstance(deform_passes, (int, np.integer)) or not 0 <= int(deform_passes) <= MAX_DEFORM_PASSES:
        raise ValueError(f"deform_passes must be a whole number 0 .. {MAX_DEFORM_PASSES}, got {deform_passes!r}")
    return int(deform_passes)


def deform_supported(window_size) -> bool:
    """Can a window deformation pass run on this final window (``lspiv_deform_supported``: square, 16, 32 or 64)?  Host-only."""
    return bool(_lib.load().lspiv_deform_supported(int(window_size[0]), int(window_size[1])))


def multipass_spec(window_size, overlap, coarse_passes=None, deform_passes=None):
    """``window_size`` as the layers below take it: the plain tuple without coarse passes (None or empty: today's path), else a
    validated :class:`MultiPassWindow`.  ``deform_passes`` = D (0 .. 4; None or 0: none): D window deformation passes follow the chain on
    the final grid -- then a :class:`MultiPassWindow` comes back also without coarse passes (a chain of one
    pass), and the final window must be one of 16, 32, 64 at one overlap for both axes.  ``coarse_passes``: coarsest first, each an int n (window n x n at overlap n / 2) or a pair
    ``(n, overlap)``; the final pass is ``window_size`` / ``overlap``.  Every pass is square and even, the list is non-increasing in n,
    pass 0 takes any even square window the per-timestep path serves, every later pass one of 16, 32, 64.  Host-only."""
    deform = deform_count(deform_passes)
    if isinstance(window_size, MultiPassWindow):
        if coarse_passes:
            raise ValueError("coarse_passes given twice: window_size is a MultiPassWindow already")
        if deform and deform != window_size.deform:
            raise ValueError("deform_passes given twice: window_size is a MultiPassWindow already")
        return window_size
    ws = (int(window_size[0]), int(window_size[1]))
    no_coarse = coarse_passes is None or len(coarse_passes) == 0
    if no_coarse and not deform:
        return ws
    if isinstance(window_size, SearchWindow):
        raise NotImplementedError(("coarse_passes" if not no_coarse else "deform_passes") +
                                  " together with a search_area_size larger than the window is not implemented")
    ov = (int(overlap[0]), int(overlap[1]))
    if deform and (ws[0] != ws[1] or ws[0] not in DEFORM_WINDOWS or ov[0] != ov[1]):
        raise ValueError(f"deform_passes need a square final window, one of {DEFORM_WINDOWS}, at one overlap for both axes, got window_size {ws}, "
                         f"overlap {ov}")
    if ws[0] != ws[1] or ov[0] != ov[1]:
        raise ValueError(f"coarse_passes need a square window and overlap, got window_size {ws}, overlap {ov}")
    passes = []
    for e in ([] if no_coarse else coarse_passes):
        if isinstance(e, (int, np.integer)) and not isinstance(e, bool):
            n, o = int(e), int(e) // 2
        else:
            try:
                n, o = e
            except (TypeError, ValueError):
                raise ValueError(f"coarse_passes: an entry is a window size n or a pair (n, overlap), got {e!r}") from None
            if any(isinstance(q, bool) or not isinstance(q, (int, np.integer)) for q in (n, o)):
                raise ValueError(f"coarse_passes: an entry is a window size n or a pair (n, overlap) of whole numbers, got {e!r}")
            n, o = int(n), int(o)
        passes.append((n, o))
    passes.append((ws[0], ov[0]))
    if len(passes) > MAX_PASSES:
        raise ValueError(f"coarse_passes: at most {MAX_PASSES} passes in a chain, got {len(passes)}")
    for k, (n, o) in enumerate(passes):
        if n < 2 or n % 2:
            raise ValueError(f"pass {k}: window {n} must be even and >= 2")
        if not 0 <= o < n:
            raise ValueError(f"pass {k}: overlap {o} must satisfy 0 <= overlap < window {n}")
        if k and n not in SHIFT_WINDOWS:
            raise ValueError(f"pass {k}: window {n} is not supported: every pass after the first (the final window_size included) must be "
                             f"one of {SHIFT_WINDOWS}")
        if k and n > passes[k - 1][0]:
            raise ValueError(f"pass {k}: window {n} is larger than pass {k - 1}'s {passes[k - 1][0]}: list the passes coarsest first")
    if _lib.load().lspiv_kernel_kind(passes[0][0], passes[0][0]) < 0:
        raise ValueError(f"pass 0: no kernel for window {passes[0][0]}")
    return MultiPassWindow(passes, deform)


SPECTRAL_FILTERS = ("none", "spof")
SPOF_WINDOWS = (16, 32, 64)


class FilteredWindow(tuple):
    """A window whose correlation goes through a spectral filter, as ONE window argument of the layers below
    ``get_ffpiv`` / ``piv_pairs``: the tuple itself is the window ``(wy, wx)`` -- grid, planes and memory plan are the plain per-pair
    launch's --, ``.spectral_filter`` the filter's name.  The filtered kernels are per-pair: the chunk alignment is 1."""

    def __new__(cls, window_size, spectral_filter: str):
        self = super().__new__(cls, (int(window_size[0]), int(window_size[1])))
        self.spectral_filter = str(spectral_filter)
        return self


def spectral_filter_spec(value) -> Optional[str]:
    """The ``spectral_filter`` keyword checked: None and ``"none"`` -> None (today's path), ``"spof"`` -> ``"spof"`` (the symmetric
    phase-only filter R / sqrt(|R|) on the cross spectrum); anything else is a ValueError listing the names.  Host-only."""
    if value is None:
        return None
    if isinstance(value, str) and value in SPECTRAL_FILTERS:
        return None if value == "none" else value
    raise ValueError(f"spectral_filter must be None or one of {SPECTRAL_FILTERS}, got {value!r}")


def spectral_filter_supported(window_size) -> Tuple[int, int]:
    """``window_size`` as a pair of ints when the filtered kernels serve it (``lspiv_spof_supported``: square, 16, 32 or 64), else a
    ValueError naming the sizes.  Host-only."""
    ws = 2 * (window_size,) if isinstance(window_size, (int, np.integer)) else tuple(window_size)
    if len(ws) != 2 or not _lib.load().lspiv_spof_supported(int(ws[0]), int(ws[1])):
        raise ValueError(f"window_size {window_size!r} is not supported with spectral_filter: the window must be square and one of {SPOF_WINDOWS}")
    return int(ws[0]), int(ws[1])


def filtered_spec(window_size, spectral_filter=None):
    """``window_size`` as the layers below take it: unchanged without a filter (None / "none": today's path), else a validated
    :class:`FilteredWindow`.  Not together with a search area, a multi-pass chain or deformation passes (NotImplementedError)."""
    if isinstance(window_size, FilteredWindow):
        if spectral_filter_spec(spectral_filter) not in (None, window_size.spectral_filter):
            raise ValueError("spectral_filter given twice: window_size is a FilteredWindow already")
        return window_size
    flt = spectral_filter_spec(spectral_filter)
    if flt is None:
        return window_size
    if isinstance(window_size, SearchWindow):
        raise NotImplementedError("spectral_filter together with a search_area_size larger than the window is not implemented: the "
                                  "filtered kernels correlate two windows of one size")
    if isinstance(window_size, MultiPassWindow):
        raise NotImplementedError(("spectral_filter together with deform_passes" if window_size.deform and len(window_size.passes) == 1
                                   else "spectral_filter together with coarse_passes") + " is not implemented: the shifted and the "
                                  "deformation kernels have no filtered form")
    return FilteredWindow(spectral_filter_supported(window_size), flt)


MASK_WINDOWS = (16, 32, 64)


class MaskedWindow(tuple):
    """A window correlated under an image mask, as ONE window argument of the layers below ``get_ffpiv`` /
    ``piv_pairs``: the tuple itself is the window ``(wy, wx)`` -- grid and planes are the plain per-pair launch's --, ``.image_mask`` the
    mask as contiguous uint8 ``(H, W)`` (non-zero = valid; converted once), ``.mask_coverage_min`` the smallest share of valid samples a
    window is evaluated at, ``.k_min`` = ``max(2, ceil(mask_coverage_min * wy * wx))`` in float64.  The masked kernels are per-pair: the
    chunk alignment is 1.  :meth:`device_mask` keeps one copy of the mask per device for the lifetime of this object -- one call."""

    def __new__(cls, window_size, image_mask, mask_coverage_min: float = 0.25):
        self = super().__new__(cls, (int(window_size[0]), int(window_size[1])))
        m = np.asarray(image_mask)
        if m.ndim != 2 or m.dtype.kind not in "buif":
            raise ValueError(f"image_mask must be a 2-D array of bool, integer or float type, got shape {m.shape}, dtype {m.dtype}")
        self.image_mask = np.ascontiguousarray(m != 0, dtype=np.uint8)
        self.mask_coverage_min = coverage_spec(mask_coverage_min)
        self.k_min = max(2, int(math.ceil(self.mask_coverage_min * float(self[0] * self[1]))))
        self._device_masks = {}
        self._lock = threading.Lock()
        return self

    def device_mask(self):
        """The mask in HBM of the CURRENT device (a ``DeviceFrames`` of shape ``(1, H, W)``, uint8), uploaded on first use there."""
        from .device import DeviceFrames, _Pool

        dev = _Pool.device()
        with self._lock:
            d = self._device_masks.get(dev)
            if d is None:
                d = self._device_masks[dev] = DeviceFrames.from_host(self.image_mask[None])
            return d


def coverage_spec(value) -> float:
    """``mask_coverage_min`` checked: a number in (0, 1], else a ValueError.  Host-only."""
    try:
        c = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"mask_coverage_min must be a number in (0, 1], got {value!r}") from None
    if not 0.0 < c <= 1.0:
        raise ValueError(f"mask_coverage_min must lie in (0, 1], got {value!r}")
    return c


def mask_supported(window_size) -> Tuple[int, int]:
    """``window_size`` as a pair of ints when the masked kernels serve it (``lspiv_mask_supported``: square, 16, 32 or 64), else a
    ValueError naming the sizes.  Host-only."""
    ws = 2 * (window_size,) if isinstance(window_size, (int, np.integer)) else tuple(window_size)
    if len(ws) != 2 or not _lib.load().lspiv_mask_supported(int(ws[0]), int(ws[1])):
        raise ValueError(f"window_size {window_size!r} is not supported with image_mask: the window must be square and one of {MASK_WINDOWS}")
    return int(ws[0]), int(ws[1])


def masked_spec(window_size, image_mask=None, mask_coverage_min: float = 0.25, dim_size=None):
    """``window_size`` as the layers below take it: unchanged without a mask (None: today's path), else a validated
    :class:`MaskedWindow`.  ``dim_size``: the frames' ``(H, W)``, which the mask must have (ValueError).  Not together with a search area,
    a multi-pass chain, deformation passes or a spectral filter (NotImplementedError naming both keywords)."""
    if isinstance(window_size, MaskedWindow):
        if image_mask is not None:
            raise ValueError("image_mask given twice: window_size is a MaskedWindow already")
        spec = window_size
    elif image_mask is None:
        coverage_spec(mask_coverage_min)
        return window_size
    else:
        if isinstance(window_size, SearchWindow):
            raise NotImplementedError("image_mask together with a search_area_size larger than the window is not implemented: the masked "
                                      "kernels correlate two windows of one size under one mask")
        if isinstance(window_size, MultiPassWindow):
            raise NotImplementedError(("image_mask together with deform_passes" if window_size.deform and len(window_size.passes) == 1
                                       else "image_mask together with coarse_passes") + " is not implemented: the shifted and the "
                                      "deformation kernels have no masked form")
        if isinstance(window_size, FilteredWindow):
            raise NotImplementedError("image_mask together with spectral_filter is not implemented: the filtered kernels have no masked form")
        spec = MaskedWindow(mask_supported(window_size), image_mask, mask_coverage_min)
    if dim_size is not None and spec.image_mask.shape != (int(dim_size[0]), int(dim_size[1])):
        raise ValueError(f"image_mask has shape {spec.image_mask.shape}, the frames are {(int(dim_size[0]), int(dim_size[1]))}")
    return spec


PEAK2_WINDOWS = (16, 32, 64)


class PeakRatioWindow(tuple):
    """A window whose launch also hands out the second correlation peak, as ONE window argument of the layers
    below ``get_ffpiv`` / ``piv_pairs``: the tuple itself is the window ``(wy, wx)`` -- grid and planes are the plain per-pair launch's --,
    ``.peak_exclusion`` the half side r of the box around the primary peak in which no second peak is looked for.  The second-peak
    kernels are per-pair: the chunk alignment is 1."""

    def __new__(cls, window_size, peak_exclusion: int = 2):
        self = super().__new__(cls, (int(window_size[0]), int(window_size[1])))
        self.peak_exclusion = exclusion_spec(peak_exclusion, min(self))
        return self


def exclusion_spec(value, n: int) -> int:
    """``peak_exclusion`` checked for a plane whose shorter side is ``n``: a whole number in 1 .. n // 4, else a ValueError.  Host-only."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= int(n) // 4:
        raise ValueError(f"peak_exclusion must be a whole number in 1 .. {int(n) // 4} (a quarter of the {int(n)} px plane), got {value!r}")
    return int(value)


def peak2_supported(window_size) -> Tuple[int, int]:
    """``window_size`` as a pair of ints when the second-peak kernels serve it (``lspiv_peak2_supported``: square, 16, 32 or 64), else a
    ValueError naming the sizes.  Host-only."""
    ws = 2 * (window_size,) if isinstance(window_size, (int, np.integer)) else tuple(window_size)
    if len(ws) != 2 or not _lib.load().lspiv_peak2_supported(int(ws[0]), int(ws[1])):
        raise ValueError(f"window_size {window_size!r} is not supported with peak_ratio: the window must be square and one of {PEAK2_WINDOWS}")
    return int(ws[0]), int(ws[1])


def peak_ratio_spec(window_size, peak_ratio: bool = False, peak_exclusion: int = 2):
    """``window_size`` as the layers below take it: unchanged without ``peak_ratio`` (today's path), else a validated
    :class:`PeakRatioWindow`.  Not together with a search area, a multi-pass chain, deformation passes, a spectral filter or an image mask
    (NotImplementedError naming both keywords): ``piv.second_peak`` on their planes serves those."""
    if isinstance(window_size, PeakRatioWindow):
        return window_size
    if not peak_ratio:
        return window_size
    hint = "; use piv.second_peak on its planes instead"
    if isinstance(window_size, SearchWindow):
        raise NotImplementedError("peak_ratio together with a search_area_size larger than the window is not implemented: the second-peak "
                                  "kernels correlate two windows of one size" + hint)
    if isinstance(window_size, MultiPassWindow):
        raise NotImplementedError(("peak_ratio together with deform_passes" if window_size.deform and len(window_size.passes) == 1
                                   else "peak_ratio together with coarse_passes") + " is not implemented: the shifted and the "
                                  "deformation kernels have no second-peak form" + hint)
    if isinstance(window_size, FilteredWindow):
        raise NotImplementedError("peak_ratio together with spectral_filter is not implemented: the filtered kernels have no second-peak form" + hint)
    if isinstance(window_size, MaskedWindow):
        raise NotImplementedError("peak_ratio together with image_mask is not implemented: the masked kernels have no second-peak form" + hint)
    return PeakRatioWindow(peak2_supported(window_size), peak_exclusion)


LAG_WINDOWS = (16, 32, 64)
MAX_LAG = 16
# the forms of ``pair_step`` as the C ABI numbers them (include/lspiv.h, LSPIV_LAG_*)
LAG_UNIFORM, LAG_WINDOW, LAG_TABLE, LAG_ADAPTIVE = 0, 1, 2, 3


class LagSpec:
    """``pair_step`` checked: ``.form`` (``LAG_UNIFORM`` / ``LAG_WINDOW`` / ``LAG_ADAPTIVE``), ``.k`` (the
    uniform lag, or ``pair_step_max`` of the adaptive form), ``.array`` (the per-window lags, uint8 ``(rows, cols)``, else None),
    ``.target128`` (``rint(128 * pair_step_target)``, adaptive form) and ``.halo``: the largest lag a pair can get, i.e. how many
    frames behind a chunk's last pair a launch needs (fewer at the end of the stack)."""

    def __init__(self, form, k, array=None, target128=0):
        self.form, self.k, self.array, self.target128 = form, k, array, target128
        self.halo = int(array.max()) if array is not None else k


def lag_supported(window_size) -> Tuple[int, int]:
    """``window_size`` as a pair of ints when the lag kernels serve it (``lspiv_lag_supported``: square, 16, 32 or 64), else a ValueError
    naming the sizes.  Host-only."""
    ws = 2 * (window_size,) if isinstance(window_size, (int, np.integer)) else tuple(window_size)
    if len(ws) != 2 or int(ws[0]) != int(ws[1]) or int(ws[0]) not in LAG_WINDOWS:
        raise ValueError(f"window_size {window_size!r} is not supported with pair_step: the window must be square and one of {LAG_WINDOWS}")
    return int(ws[0]), int(ws[1])


def _whole(value, lo, hi, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{name} must be a whole number in {lo} .. {hi}, got {value!r}")
    return int(value)


def lag_spec(pair_step, window_size, grid=None, pair_step_max: int = 4, pair_step_target=None):
    """``pair_step`` / ``pair_step_max`` / ``pair_step_target`` checked for the square window ``window_size`` and, for an array, the grid
    ``(rows, cols)``: None for ``pair_step`` None or 1 (today's path), else a :class:`LagSpec`.  ValueError for a window other than 16,
    32 or 64 px square, a lag outside 1 .. 16, an array of another shape or type, a target outside (0, window / 2].  Host-only."""
    if isinstance(pair_step, LagSpec):
        return pair_step
    k_max = _whole(pair_step_max, 1, MAX_LAG, "pair_step_max")
    if pair_step is None:
        return None
    what = f"pair_step must be a whole number in 1 .. {MAX_LAG}, an integer array (rows, cols) or 'adaptive', got "
    if isinstance(pair_step, str):
        if pair_step != "adaptive":
            raise ValueError(what + repr(pair_step))
        n = lag_supported(window_size)[0]
        target = n / 4 if pair_step_target is None else pair_step_target   # the quarter rule
        if isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)) or not 0 < float(target) <= n / 2:
            raise ValueError(f"pair_step_target must be a number in (0, {n / 2}] px (half the {n} px window), got {pair_step_target!r}")
        t128 = int(np.rint(128.0 * float(target)))
        if t128 < 1:
            raise ValueError(f"pair_step_target {pair_step_target!r} is below 1 / 256 px")
        return LagSpec(LAG_ADAPTIVE, k_max, None, t128)
    if pair_step_target is not None:
        raise ValueError("pair_step_target belongs to pair_step='adaptive'")
    if isinstance(pair_step, (int, np.integer)) and not isinstance(pair_step, bool):
        k = _whole(pair_step, 1, MAX_LAG, "pair_step")
        if k == 1:
            return None
        lag_supported(window_size)
        return LagSpec(LAG_UNIFORM, k)
    arr = np.asarray(pair_step)
    if arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer) or arr.ndim != 2:
        raise ValueError(what + (f"an array of {arr.dtype} {arr.shape}" if arr.ndim else repr(pair_step)))
    lag_supported(window_size)
    if grid is not None and arr.shape != tuple(grid):
        raise ValueError(f"pair_step must have the grid's shape {tuple(grid)}, got {arr.shape}")
    if arr.size == 0 or arr.min() < 1 or arr.max() > MAX_LAG:
        raise ValueError(f"pair_step: every lag must lie in 1 .. {MAX_LAG}")
    return LagSpec(LAG_WINDOW, 0, np.ascontiguousarray(arr, dtype=np.uint8))


MIN_STEERING_GRID = 3


def ensemble_chain_spec(spec: MultiPassWindow, dim_size) -> MultiPassWindow:
    """``spec`` as a chain of ENSEMBLES on frames of ``dim_size``, or NotImplementedError: every pass that
    steers another one needs a grid of at least 3 x 3 windows.  One field of such a pass moves a window of the next pass for EVERY
    pair of the run, and the predictor's 3 x 3 median is all that keeps a stray ensemble vector out of it: on one or two windows per
    side that median is the vector itself, or the mean of two.  (The per-timestep chain, section 2d, predicts per pair and takes any
    grid.)  Host-only."""
    for k, (n, o) in enumerate(spec.passes[:-1]):
        rows, cols = get_array_shape(dim_size, (n, n), (o, o))
        if min(rows, cols) < MIN_STEERING_GRID:
            raise NotImplementedError(f"coarse_passes with ensemble_corr=True is not implemented for a steering pass of fewer than "
                                      f"{MIN_STEERING_GRID} x {MIN_STEERING_GRID} windows (pass {k}: {n} px at overlap {o} gives {rows} x {cols} "
                                      f"on a {dim_size[0]} x {dim_size[1]} frame): its one field steers every pair of the run, and the "
                                      "predictor's 3 x 3 median has no neighbourhood there to reject a stray vector with")
    return spec


def get_axis_shape(dim_size: int, window_size: int, overlap: int) -> int:
    nr, nc = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_grid_shape(dim_size, dim_size, window_size, window_size, overlap, overlap,
                                            C.byref(nr), C.byref(nc)))
    return nr.value


def get_array_shape(dim_size, window_size, overlap) -> Tuple[int, int]:
    nr, nc = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_grid_shape(dim_size[0], dim_size[1], window_size[0], window_size[1],
                                            overlap[0], overlap[1], C.byref(nr), C.byref(nc)))
    return nr.value, nc.value


def get_rect_coordinates(dim_size, window_size, overlap, search_area_size=None, center_on_field=False):
    """Window-centre pixel indices ``(x_cols, y_rows)``, int64 (usable for fancy indexing)."""
    if center_on_field:
        raise NotImplementedError("pyorc never centres the grid on the field")
    sa = window_size if search_area_size is None else search_area_size
    n_rows, n_cols = get_array_shape(dim_size, sa, overlap)
    rows = np.empty(max(n_rows, 0), dtype=np.int64)
    cols = np.empty(max(n_cols, 0), dtype=np.int64)
    _lib.check(_lib.load().lspiv_grid_coords(dim_size[0], dim_size[1], sa[0], sa[1], overlap[0], overlap[1],
                                             rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                             cols.ctypes.data_as(C.POINTER(C.c_int64))))
    return cols, rows


def required_memory(n_frames: int, dim_size, window_size, overlap, search_area_size=None,
                    dtype=np.uint8, with_planes: bool = False, sliding_blocks: int = 0, coarse_passes=None,
                    ensemble_sums: bool = False, deform_passes=None) -> int:
    """HBM bytes one fused call on ``n_frames`` frames needs (frames + four result planes).

    The reference's figure is the host RAM of the materialised window stack + correlation volume
    (x3.9 .. x14.8 of the frames); the fused kernel materialises neither.

    ``sliding_blocks``: the blocks of a sliding ensemble's WHOLE run (:func:`sliding_outputs`); its block store stays in HBM next
    to every chunk (:func:`sliding_store_bytes`).  ``coarse_passes`` (or a :class:`MultiPassWindow`): a multi-pass chain.
    ``ensemble_sums``: an ensemble's plane sums and counts (:func:`ensemble_sums_bytes`) stay in HBM next to every chunk -- of the pass
    that needs most, in a chain (the multi-pass ensemble, INTEGRATION.md section 2e, runs one pass at a time).
    ``deform_passes`` (or a :class:`MultiPassWindow` that carries them): the warped frames of one batch of pairs and the nodes
    (:func:`deform_bytes`) come on top.  A :class:`FilteredWindow` answers as the plain per-pair launch of its window: the filtered
    kernels have no workspace.  A :class:`MaskedWindow` answers as the plain per-pair launch of its window plus the bytes of the mask, a
    :class:`PeakRatioWindow` plus the four floats of the second peak per window and pair.
    """
    if coarse_passes or deform_count(deform_passes) or isinstance(window_size, MultiPassWindow):
        # a chain: the frames once, the largest pass's launch (results, rescue lists, the planes of the final pass), and the
        # intermediates of two grids -- two result blocks and an offset array of the largest grid (lspiv_piv_multipass_dev_at)
        spec = multipass_spec(window_size, overlap, coarse_passes, deform_passes)
        frames_bytes = int(n_frames) * int(dim_size[0]) * int(dim_size[1]) * np.dtype(dtype).itemsize
        last = len(spec.passes) - 1
        per_pass = [required_memory(n_frames, dim_size, (n, n), (o, o), dtype=dtype, with_planes=with_planes and k == last) - frames_bytes
                    for k, (n, o) in enumerate(spec.passes)]
        tiles = [(int(n_frames) - 1) * int(np.prod(get_array_shape(dim_size, (n, n), (o, o)))) for n, o in spec.passes]
        sums = max(ensemble_sums_bytes(dim_size, (n, n), (o, o)) for n, o in spec.passes) if ensemble_sums else 0
        n, o = spec.passes[-1]
        deform = deform_bytes(n_frames, dim_size, (n, n), (o, o)) if spec.deform else 0
        return frames_bytes + max(per_pass) + 2 * 16 * max(tiles[:-1], default=0) + 4 * max(tiles[1:], default=0) + sums + deform
    sa = window_size if search_area_size is None else search_area_size
    code = _lib.DTYPE_CODES[np.dtype(dtype)]
    r = _lib.load().lspiv_required_bytes(n_frames, dim_size[0], dim_size[1], code, sa[0], sa[1],
                                         overlap[0], overlap[1], int(with_planes))
    need = _lib.check(r)
    if isinstance(window_size, MaskedWindow):
        need += int(window_size.image_mask.nbytes)
    if isinstance(window_size, PeakRatioWindow):
        need += 16 * (int(n_frames) - 1) * int(np.prod(get_array_shape(dim_size, sa, overlap)))
    if sliding_blocks:
        need += sliding_store_bytes(sliding_blocks, dim_size, sa, overlap)
    if ensemble_sums:
        need += ensemble_sums_bytes(dim_size, sa, overlap)
    return need


def lag_required_memory(n_pairs: int, halo: int, dim_size, window_size, overlap, dtype=np.uint8, spec=None) -> int:
    """HBM bytes one lagged launch of ``n_pairs`` pairs with ``halo`` frames behind its last pair's frame t needs (INTEGRATION.md section
    2k): the plain launch on ``n_pairs + halo`` frames (the frames, a result block that large -- never less than the launch's own, and the
    block pass 0 of the adaptive form writes its field into --, the rescue lists) plus the two tables, one lag byte and two int16 per
    window and pair."""
    n_win = int(np.prod(get_array_shape(dim_size, window_size, overlap)))
    return required_memory(int(n_pairs) + max(int(halo), 1), dim_size, tuple(window_size), overlap, dtype=dtype) + 5 * int(n_pairs) * n_win


def deform_bytes(n_frames: int, dim_size, window_size, overlap) -> int:
    """HBM bytes the deformation passes of a call on ``n_frames`` frames take next to the chain: the float32 warped frames of ONE batch
    of pairs (at most 256 MiB, one frame at least) and the int32 nodes of every pair (``lspiv_deform_required_bytes``)."""
    return _lib.check(_lib.load().lspiv_deform_required_bytes(int(n_frames), int(dim_size[0]), int(dim_size[1]), int(window_size[0]),
                                                              int(window_size[1]), int(overlap[0]), int(overlap[1])))


def ensemble_sums_bytes(dim_size, window_size, overlap) -> int:
    """HBM bytes of an ensemble handle's running state: one float32 plane sum and one count per window, and the window offsets of a
    shifted handle (2 x int16)."""
    n_win = int(np.prod(get_array_shape(dim_size, window_size, overlap)))
    return n_win * (int(window_size[0]) * int(window_size[1]) + 2) * 4


def sliding_spec(ensemble_corr: bool, ensemble_window, ensemble_stride):
    """The sliding-ensemble keywords of ``get_ffpiv`` checked -> None (no ``ensemble_window``) or ``(M, s)`` pairs: 1 <= s <= M and
    M % s == 0; ``ensemble_stride`` None means s = M (block ensembles).  Both keywords need ``ensemble_corr=True``.  Host-only."""
    if ensemble_window is None:
        if ensemble_stride is not None:
            raise ValueError("ensemble_stride needs ensemble_window")
        return None
    if not ensemble_corr:
        raise ValueError("ensemble_window / ensemble_stride need ensemble_corr=True")
    for name, val in (("ensemble_window", ensemble_window), ("ensemble_stride", ensemble_stride)):
        if val is not None and (isinstance(val, bool) or not isinstance(val, (int, np.integer))):
            raise ValueError(f"{name} must be a whole number of frame pairs, got {val!r}")
    M = int(ensemble_window)
    s = M if ensemble_stride is None else int(ensemble_stride)
    if not (1 <= s <= M) or M % s != 0:
        raise ValueError(f"need 1 <= ensemble_stride <= ensemble_window and ensemble_window % ensemble_stride == 0, got "
                         f"ensemble_window {M}, ensemble_stride {s}")
    return M, s


def sliding_outputs(n_pairs: int, M: int, s: int) -> Tuple[int, int]:
    """(n_blk, n_out) of a sliding ensemble over ``n_pairs`` pairs: block b = pairs [b s, (b + 1) s), output j = blocks j .. j + M / s - 1.
    Trailing pairs that fill no block enter no output."""
    n_blk = n_pairs // s
    n_out = n_blk - M // s + 1
    if n_out < 1:
        raise ValueError(f"ensemble_window {M} needs at least {M} pairs, got {n_pairs}")
    return n_blk, n_out


def sliding_store_bytes(n_blocks: int, dim_size, window_size, overlap) -> int:
    """HBM bytes of a sliding ensemble's block store: one float32 plane sum and one count per (block, window).  Host-only."""
    n_rows, n_cols = get_array_shape(dim_size, window_size, overlap)
    return int(n_blocks) * n_rows * n_cols * (int(window_size[0]) * int(window_size[1]) + 1) * 4


def available_memory() -> int:
    """Free HBM on the current device in bytes (library workspaces counted as reusable)."""
    free, total = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_available_bytes(C.byref(free), C.byref(total)))
    return free.value


def available_host_memory() -> int:
    """Free host RAM in bytes -- what ``ffpiv.window.available_memory`` answers in the reference (pyorc/velocimetry/ffpiv.py:129), and
    what bounds how much of a LAZY stack ``get_ffpiv`` may materialise at a time (the chunks that ``.load()`` brings in live on the
    host before they cross PCIe).  ``psutil`` when importable, ``/proc/meminfo`` otherwise."""
    try:
        import psutil

        return int(psutil.virtual_memory().available)
    except Exception:
        try:
            with open("/proc/meminfo") as fh:
                for line in fh:
                    if line.startswith("MemAvailable:"):
                        return int(line.split()[1]) * 1024
        except OSError:
            pass
    return 8 << 30   # nothing to ask: a conservative 8 GiB


def chunk_alignment(window_size, dim_size=None, overlap=None) -> int:
    """Frame pairs between two anchors of the time-walking kernels: time chunks that start on a multiple of it reproduce the
    whole-stack result bit for bit.  1 for per-pair kernels.  Host-only.

    The anchor length depends on the window GRID since round 5 (25 pairs; 75 on grids with at least as many windows as the chip has
    lane groups, ``lspiv_chunk_alignment_grid``): pass the frame shape ``dim_size`` and the ``overlap`` whenever chunks of frames of
    that shape are cut.  Without them the alignment that is right on EVERY grid comes back (``lspiv_chunk_alignment``, ABI 5: the
    longest anchor length of the window family, a multiple of every grid's -- 75 where ABI 4 answered 25)."""
    lib = _lib.load()
    if isinstance(window_size, (SearchWindow, FilteredWindow, MaskedWindow, PeakRatioWindow)):
        return 1   # the search-area, the filtered, the masked and the second-peak kernels are per-pair: any chunking gives the same bits
    if isinstance(window_size, MultiPassWindow):
        # pass 0 is the per-timestep path on ITS window and grid; every later pass is pair-local
        n0, o0 = window_size.passes[0]
        return chunk_alignment((n0, n0), dim_size, None if dim_size is None else (o0, o0))
    if dim_size is None:
        return _lib.check(lib.lspiv_chunk_alignment(int(window_size[0]), int(window_size[1])))
    ov = (int(window_size[0]) // 2, int(window_size[1]) // 2) if overlap is None else overlap
    return _lib.check(lib.lspiv_chunk_alignment_grid(int(dim_size[0]), int(dim_size[1]), int(window_size[0]), int(window_size[1]),
                                                     int(ov[0]), int(ov[1])))


def chunk_alignment_any_grid(window_size) -> int:
    """The alignment that is right for EVERY frame shape (= ``chunk_alignment(window_size)`` since ABI 5).  For callers that cut the time
    axis before they know the frames (``shard.sharded_piv`` without ``frame_shape``)."""
    return chunk_alignment(window_size)
