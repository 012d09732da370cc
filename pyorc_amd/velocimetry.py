"""Mirror of ``pyorc/velocimetry/ffpiv.py`` for ``engine="hip"``.

``get_ffpiv`` keeps the reference's signature, time chunking with a 1-frame halo
(pyorc/velocimetry/ffpiv.py:140), result layout (``s2n``, ``corr``, ``v_x``, ``v_y`` on
``(time, y, x)``, time = stamp of the 2nd frame of each pair, float32) and warnings/exceptions,
but each chunk is ONE fused GPU call instead of cross_corr + numpy reductions +
u_v_displacement over a materialised (T-1, n_win, wy, wx) volume.

Differences, all deliberate and documented in DESIGN.md:
  * a LAZY stack (anything with ``load()``: pyorc's dask-backed DataArray) is kept resident in HBM while it runs (``pyorc_amd.resident``,
    round 6): what ``.load()`` materialises at a time is planned against free HOST memory like in the reference (``available_memory() /
    memory_factor``, ffpiv.py:129; same warning text), divided by the number of loads the chunk executor keeps in flight, cut on dask's
    own block boundaries and WITHOUT the reference's halo frame (no block is decoded + projected twice); the kernels are launched on
    their anchors as the frames arrive.  When the stack is the direct product of ``project_hip`` (``pyorc_amd.plugin``), the CAMERA
    frames are loaded and projected on the device: ortho frames never exist on the host -- and when those camera frames are the recipe's
    filters (``normalize`` / ``edge_detect`` / ``minmax`` / ``smooth``) over a uint8 stack, the uint8 frames are loaded and filtered on
    the device too;
  * for a materialised stack (numpy, ``DeviceFrames``) the chunk size is planned against free HBM, not host RAM, and rounded down to a multiple of
    ``window.chunk_alignment`` (>= one multiple): chunks then start on the anchors of the time-walking kernels'
    segments, so the result is the same, bit for bit, whatever chunk size the planner or the user picked -- as in the
    reference, which computes every window independently;
  * quirk Q1 (user ``chunksize`` raises NameError in the reference, ffpiv.py:127-140) is fixed;
  * quirk Q2 (chunks are computed twice, ffpiv.py:402-408) is not reproduced;
  * quirk Q3 (ensemble ``n_frames`` = number of CHUNKS, ffpiv.py:373) IS reproduced, because it
    changes results (the ``count_min`` filter).

Works on ``xarray.DataArray`` frames (returns ``xarray.Dataset``) when xarray is importable, and
on plain ``(T, H, W)`` numpy arrays (returns ``PivResult``, a dict with the same variable names).
"""

from __future__ import annotations

import math
import warnings
from typing import Literal, Optional, Tuple

import numpy as np

from . import executor, piv, resident, window
from .device import is_device

try:  # xarray is optional: the GPU box image does not ship it
    import xarray as xr
except ImportError:  # pragma: no cover - depends on the environment
    xr = None

CHUNK_SIZE_ERROR = (
    "Chunk size with selected nr of chunks ({chunks}) is 2 or less. If you manually "
    "selected `chunks={chunks}` then consider increasing chunk size to at least 2, and preferrably more. If memory "
    "is limited, consider closing memory intensive applications. If pyorc crashes, then this is due to "
    " insufficient memory."
)
CHUNK_SIZE_WARNING = (
    "Memory availability is poor ({avail_mem} GB). Chunk size is automatically set to {chunksize} to avoid "
    "memory issues. If pyorc crashes, then this is due to insufficient memory. Consider to manually set a lower "
    "chunk size e.g using `get_piv(engine={engine}, chunk=2)` or `get_piv(engine={engine}, chunk=3)` or close "
    "memory intensive applications."
)
MAX_WINDOWS_PER_LAUNCH = 2**31 - 1


class PivResult(dict):
    """Stand-in for ``xarray.Dataset`` when xarray is absent: data variables + ``coords`` + ``dims``."""

    dims = ("time", "y", "x")

    def __init__(self, data_vars, coords):
        super().__init__(data_vars)
        self.coords = coords

    def mean_time(self):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            return {k: np.nanmean(v, axis=0) for k, v in self.items()}


def _is_xr(obj) -> bool:
    return xr is not None and isinstance(obj, xr.DataArray)


def load_frame_chunk(da):
    """pyorc/velocimetry/ffpiv.py:13-21: materialise a chunk, retry without its last frame on TypeError."""
    if not hasattr(da, "load"):
        return da
    try:
        return da.load()
    except TypeError:
        return load_frame_chunk(da[:-1])


def _values(da):
    if is_device(da):
        return da   # HBM-resident chunk (a view): handed to the *_dev entry points as it is
    return da.values if hasattr(da, "values") else np.asarray(da)


def plan_chunks(n_frames: int, req_mem: float, avail_mem: float, chunksize: Optional[int], engine: str,
                n_win: int = 1):
    """Chunk planner of pyorc/velocimetry/ffpiv.py:127-142 -> (chunksize, [(start, stop), ...])."""
    if chunksize is None:
        chunks = int((req_mem // avail_mem) + 1)
        chunksize = int(np.ceil(n_frames / chunks))
        if chunksize <= 5:
            warnings.warn(   # at the caller of get_ffpiv (get_ffpiv -> _plan_slices -> here)
                CHUNK_SIZE_WARNING.format(avail_mem=avail_mem / 1e9, chunksize=chunksize, engine=engine), stacklevel=4
            )
            chunksize = 5  # hard override, try to manage with 5
            chunks = int(np.ceil(n_frames / chunksize))
    else:
        chunksize = int(chunksize)
        chunks = int(np.ceil(n_frames / max(chunksize, 1)))  # reference: NameError here (quirk Q1)
    if chunksize < 2:
        raise OverflowError(CHUNK_SIZE_ERROR.format(chunks=chunks))
    # one launch indexes windows with 32 bits
    max_cs = max(2, MAX_WINDOWS_PER_LAUNCH // max(n_win, 1))
    if chunksize > max_cs:
        chunksize = max_cs
        chunks = int(np.ceil(n_frames / chunksize))
    slices = [(max(c * chunksize - 1, 0), min((c + 1) * chunksize, n_frames)) for c in range(chunks)]
    # check if there are chunks that are too small in size, needs to be at least 2 frames per chunk
    return chunksize, [(a, b) for a, b in slices if b - a >= 2]


def aligned_slices(n_frames: int, chunksize: int, align: int, n_win: int = 1, fits=None):
    """Frame slices ``[(a, b), ...]`` of chunks whose first PAIR index ``a`` is a multiple of ``align``.

    ``chunksize`` is the number of FRAMES per chunk planned by :func:`plan_chunks` (a memory bound).  A chunk of C pairs
    reads C + 1 frames -- the halo frame sits at the end of a chunk instead of at its start (ffpiv.py:140), the union of
    pairs is the same --, so C is ``chunksize - 1`` rounded down to a multiple of ``align``.  When the plan is smaller
    than one anchor length (the forced ``chunksize = 5`` of the low-memory branch, or a small user value), one anchor
    length is still used IF ``fits(n_frames_of_chunk)`` says it fits the memory budget (chunk-invariant results are worth
    more than a plan that was conservative for the reference's 4-15x larger window stack); otherwise the plan is
    honoured with chunks of ``chunksize - 1`` pairs that start off the anchors: correct, and equal to an aligned run
    up to the last float32 bit of a chunk's first pairs.
    """
    n_pairs = n_frames - 1
    budget = max(1, int(chunksize) - 1)            # pairs per chunk the plan allows (C + 1 <= chunksize frames)
    if budget >= align:
        C = (budget // align) * align
    elif fits is None or fits(min(align, n_pairs) + 1):
        C = align
    else:
        C = budget
    max_pairs = max(1, MAX_WINDOWS_PER_LAUNCH // max(n_win, 1))
    if C > max_pairs:  # one launch indexes windows with 32 bits: shrink, aligned if possible
        C = max(1, (max_pairs // align) * align) if max_pairs >= align else max_pairs
    return [(p, min(p + C, n_pairs) + 1) for p in range(0, n_pairs, C)]


def _dataset(data_vars, time, y, x, like):
    if _is_xr(like):
        return xr.Dataset({k: (["time", "y", "x"], v) for k, v in data_vars.items()},
                          coords={"time": time, "y": y, "x": x})
    return PivResult(data_vars, {"time": np.asarray(time), "y": np.asarray(y), "x": np.asarray(x)})


def get_ffpiv(
    frames,
    y: np.ndarray,
    x: np.ndarray,
    dt: np.ndarray,
    window_size: Tuple[int, int],
    overlap: Tuple[int, int],
    search_area_size: Tuple[int, int],
    res_y: float,
    res_x: float,
    chunksize: Optional[int] = None,
    memory_factor: float = 4,
    engine: Literal["hip"] = "hip",
    ensemble_corr: bool = False,
    corr_min: float = 0.2,
    s2n_min: float = 3,
    count_min: float = 0.2,
    signal_threshold: Optional[float] = None,
    time: Optional[np.ndarray] = None,
    prefetch: Optional[int] = None,
    devices=None,
    ensemble_window: Optional[int] = None,
    ensemble_stride: Optional[int] = None,
    coarse_passes=None,
    deform_passes=None,
    spectral_filter=None,
    image_mask=None,
    mask_coverage_min: float = 0.25,
    peak_ratio: bool = False,
    peak_exclusion: int = 2,
    validate=None,
    pair_step=None,
    pair_step_max: int = 4,
    pair_step_target: Optional[float] = None,
):
    """Compute time-resolved (or ensemble) PIV on the MI355X; signature of pyorc's ``get_ffpiv`` (ffpiv.py:24-42).

    ``frames``: ``xr.DataArray (time, y, x)``, a ``(T, H, W)`` array, or a ``pyorc_amd.device.DeviceFrames`` stack that
    already lives in HBM (the output of ``pyorc_amd.filters`` / ``Projection.project_frames`` on device stacks: no
    chunk is staged through the host then, each chunk is one launch on a view of the stack); ``dt``: time step per pair (``T-1``,
    seconds; an ``xr.DataArray`` on ``time[1:]`` in pyorc); ``time``: frame time stamps when ``frames`` is a
    plain array (default ``arange(T)``).  Returns Dataset / PivResult with ``s2n, corr, v_x, v_y``.

    ``prefetch``: how many lazy chunks are materialised (``load_frame_chunk``: dask runs decode + projection + filters there)
    AHEAD of the chunk being launched, on a worker thread (``pyorc_amd.executor``; default ``LSPIV_PREFETCH_DEPTH`` or 1; 0 = the
    reference's serial load-then-compute loop, ffpiv.py:399-408).  Same chunks, same order, same results; stacks that are already
    materialised (numpy, ``DeviceFrames``) have nothing to prefetch.

    ``devices``: None (the calling thread's device: one worker, as always), ``"all"`` (every device ``lspiv_device_count`` reports) or
    a sequence of device indices (repeats allowed: ``[0, 0]`` is two workers on device 0).  Each device works on one thread of its
    own over a contiguous block of pairs cut on the kernels' anchors (:func:`device_work`), so per-timestep results are the bits of
    one device; ensemble sums are reduced device to device (``piv.ensemble_allreduce``) and finished with the float64 rescue of
    every device's pairs (``shard.staged_finish``).  A ``DeviceFrames`` stack runs on the device it lives on.

    ``ensemble_window`` = M, ``ensemble_stride`` = s (with ``ensemble_corr=True`` only; the project's own mode, INTEGRATION.md section
    2c): a SLIDING ensemble -- output j is fitted on the mean correlation plane of the M pairs [j s, j s + M), so the result keeps a time
    axis of ``(P // s) - M // s + 1`` steps.  1 <= s <= M, M % s == 0; s None = M (block ensembles).  Chunks are cut on multiples of s
    and every chunking gives the same bits.  One device, materialised stacks (numpy, ``DeviceFrames``).

    ``coarse_passes`` (the project's own mode): multi-pass PIV -- a list of coarse passes, coarsest first, each
    an int n (window n x n at overlap n / 2) or a pair ``(n, overlap)``, run before the final pass ``window_size`` / ``overlap`` (16, 32 or
    64 px), whose grid is the result's.  Every pass after the first cuts its window of frame t+1 at the integer offset the previous pass
    predicts.  None or empty: today's path.  Chunks are cut on the anchors of pass 0; ``devices=`` and ``chunksize=`` give the same bits.
    Without a search area of its own.  With ``ensemble_corr=True`` every pass is a full ensemble over all
    pairs and ONE field steers the next pass's windows: the passes are the outer loop, the chunk loop the inner one; materialised
    stacks (numpy, ``DeviceFrames``), not together with ``ensemble_window``, and every pass that steers another one needs a grid of at
    least 3 x 3 windows (``window.ensemble_chain_spec``).

    ``deform_passes`` = D (the project's own mode; a whole number 0 .. 4, None or 0: today's path bit for bit):
    after the chain (``coarse_passes`` may be empty) D window deformation passes run on the final grid, each between frame t and frame
    t+1 warped at sub-pixel resolution by the field of the pass before it; the final window must be 16, 32 or 64 px.  One pass roughly
    halves the median error on sheared flows, a second one neither helps nor hurts.  Pair-local: ``chunksize=``, ``devices=``, host
    stacks, ``DeviceFrames`` and lazy stacks give the same bits.  Not with ``ensemble_corr=True`` and not with a search area.

    ``spectral_filter`` (the project's own mode; None or ``"none"``: today's path bit for bit): ``"spof"`` runs
    the correlation through the symmetric phase-only filter -- every bin R of the cross spectrum becomes R / sqrt(|R|) --, which keeps
    the tracers' peak where a static or slow background (bed texture, ripples, glare) outweighs them.  Windows of 16, 32 or 64 px,
    per-timestep and ensemble mode; ``corr`` / ``s2n`` are those of the filtered planes, so useful values of ``corr_min`` / ``s2n_min``
    are lower than for the plain ensemble.  Pair-local: ``chunksize=``, ``devices=``, host stacks, ``DeviceFrames`` and lazy stacks give
    the same bits.  No float64 rescue.  Not with ``coarse_passes``, ``deform_passes``, a search area or ``ensemble_window``.

    ``image_mask`` (the project's own mode; None: today's path bit for bit): an ``(H, W)`` array of bool,
    integer or float type, non-zero = valid, one static mask for every frame -- banks, piers, vegetation, the outside of the
    orthoprojected area.  Every window is correlated over its valid samples only (mean, standard deviation, ``signal_threshold`` and the
    divisor of the plane are those of the valid samples; excluded samples are never read into the arithmetic, NaN there is harmless); a
    window with fewer than ``max(2, ceil(mask_coverage_min * n * n))`` valid samples is NaN.  ``mask_coverage_min`` lies in (0, 1].
    Windows of 16, 32 or 64 px, per-timestep mode.  Pair-local: ``chunksize=``, ``devices=``, host stacks, ``DeviceFrames`` and lazy
    stacks give the same bits; the mask goes to each device once per call.  Not with ``ensemble_corr=True``, ``coarse_passes``,
    ``deform_passes``, a search area, ``spectral_filter`` or ``ensemble_window``.

    ``peak_ratio`` (the project's own mode; False: today's path bit for bit): the result gains ``peak_ratio``
    (height of the highest correlation peak over the second highest: what PIV practice validates a vector with), ``corr2`` (that second
    height) and ``v_x2``, ``v_y2`` (the runner-up vector, scaled like ``v_x``, ``v_y``: the usual substitute for a rejected one).  The
    second peak is the largest sample of the plane that is at least 1e-5, lies outside the box of half side ``peak_exclusion`` (1 ..
    n // 4, default 2) around the primary peak and is no smaller than its 4-neighbours; without one ``corr2`` = 0, ``peak_ratio`` = inf
    and the vector NaN.  ``s2n``, ``corr``, ``v_x``, ``v_y`` are those of ``peak_ratio=False`` up to the last float32 bit of the
    one-window-per-job kernels.  Windows of 16, 32 or 64 px, per-timestep mode.  Pair-local: ``chunksize=``, ``devices=``, host stacks,
    ``DeviceFrames`` and lazy stacks give the same bits.  Not with ``image_mask``, ``spectral_filter``, ``coarse_passes``,
    ``deform_passes``, a search area or ``ensemble_corr=True`` (NotImplementedError): ``piv.second_peak`` on their planes serves those.

    ``validate`` (the project's own option; None: today's path bit for bit): True, or a dict of
    ``validate.median_test``'s keywords (``threshold`` 2.0, ``epsilon`` 0.1 px, ``min_neighbours`` 3, ``replace`` "nan" | "median",
    ``iterations`` 1) -- the normalised median test over the 3 x 3 neighbourhood of every vector, on the displacement in PIXELS before the
    px -> m/s scaling: on the result block in HBM for a ``DeviceFrames`` or lazy stack, through the host twin right after the call for a
    host stack; both give the bits of ``median_test`` on the unscaled fields followed by the scaling.  The result gains the uint8
    variable ``flag``: 0 kept or unjudged, 1 rejected (NaN), 2 substituted by the runner-up, 3 replaced by the neighbourhood median.  With
    ``peak_ratio=True`` the runner-up vector is the first substitute for an outlier; ``v_x2``, ``v_y2``, ``corr2``, ``peak_ratio``,
    ``corr`` and ``s2n`` stay as they are.  Pair-local: ``chunksize=``, ``devices=``, host stacks, ``DeviceFrames`` and lazy stacks give the
    same bits.  With the plain path, ``search_area_size``, ``spectral_filter``, ``image_mask`` and ``peak_ratio``; not with
    ``ensemble_corr=True``, ``coarse_passes`` or ``deform_passes`` (NotImplementedError): ``validate.median_test`` on the result serves those.

    ``pair_step`` (the project's own mode; None: today's path bit for bit): multi-frame PIV for slow flow --
    pair t, window w is correlated against frame ``t + k[t, w]`` and the displacement divided by k, so ``v_x``, ``v_y`` keep their
    meaning, the T - 1 outputs and the time axis stay, and the result gains the uint8 variable ``pair_step``, the effective lags.  A
    whole number k in 1 .. 16 (1: today's path and its bits plus the all-ones variable); an integer array ``(rows, cols)`` of lags 1 ..
    16; or ``"adaptive"``: a lag-1 pass, then per window the largest lag ``<= pair_step_max`` (1 .. 16, default 4) that keeps the median
    displacement of its 3 x 3 neighbourhood at or below ``pair_step_target`` px (default window / 4, at most window / 2), with the
    integer window offset that goes with it.  Every lag is clipped to the frames left in the stack.  Windows of 16, 32 or 64 px,
    per-timestep mode, materialised stacks (numpy, ``DeviceFrames``) on one device; every chunk carries a halo of min(largest lag,
    frames to the end of the stack) frames, and every chunking gives the same bits.  A lag multiplies the shear inside a window: where the
    velocity changes by more than about 1 px per frame across a window, long lags hurt -- that is what ``pair_step_target`` is for.  Not
    with ``ensemble_corr=True``, ``ensemble_window``, ``coarse_passes``, ``deform_passes``, ``spectral_filter``, ``image_mask``,
    ``peak_ratio``, ``validate``, a search area larger than the window, lazy stacks or ``devices=`` (NotImplementedError).
    """
    if engine != "hip":
        raise ValueError(f"Selected PIV engine {engine} does not exist.")
    if validate is not None:
        from .validate import validate_spec

        validate = validate_spec(validate)     # ValueError for a value outside its range; False is None
    if validate is not None:
        if ensemble_corr:
            raise NotImplementedError("validate together with ensemble_corr=True is not implemented: the ensemble has one field and no "
                                      "per-pair result block; use validate.median_test on the result instead")
        if (coarse_passes is not None and len(coarse_passes)) or window.deform_count(deform_passes):
            raise NotImplementedError("validate together with coarse_passes / deform_passes is not implemented: no validation runs between "
                                      "or after the passes of a chain; use validate.median_test on the result instead")
    lag = window.lag_spec(pair_step, window_size, (len(y), len(x)), pair_step_max, pair_step_target)     # ValueError: sizes, ranges, shapes
    if lag is not None:
        return _get_ffpiv_lagged(frames, y, x, dt, window_size, overlap, search_area_size, res_y, res_x, chunksize, memory_factor, engine,
                                 signal_threshold, time, devices, lag,
                                 dict(ensemble_window=ensemble_window is not None, ensemble_corr=ensemble_corr,
                                      coarse_passes=coarse_passes is not None and len(coarse_passes) > 0,
                                      deform_passes=window.deform_count(deform_passes) > 0,
                                      spectral_filter=window.spectral_filter_spec(spectral_filter) is not None,
                                      image_mask=image_mask is not None, peak_ratio=peak_ratio, validate=validate is not None))
    if pair_step is not None:     # a lag of one frame: today's path, and the variable that says so
        res = get_ffpiv(frames, y, x, dt, window_size, overlap, search_area_size, res_y, res_x, chunksize, memory_factor, engine, ensemble_corr,
                        corr_min, s2n_min, count_min, signal_threshold, time, prefetch, devices, ensemble_window, ensemble_stride,
                        coarse_passes, deform_passes, spectral_filter, image_mask, mask_coverage_min, peak_ratio, peak_exclusion, validate)
        if np.ndim(res["v_x"]) == 3:
            _add_variable(res, "pair_step", np.ones(np.shape(res["v_x"]), dtype=np.uint8))
        return res
    # a search area of its own: one window argument that answers for the search area wherever a grid, a plan or an alignment is asked for
    window_size = window.search_spec(window_size, search_area_size)
    flt = window.spectral_filter_spec(spectral_filter)     # ValueError for an unknown name
    window.coverage_spec(mask_coverage_min)                # ValueError outside (0, 1]
    if image_mask is not None:
        if ensemble_window is not None:
            raise NotImplementedError("image_mask together with ensemble_window is not implemented: a sliding ensemble has no masked form")
        if ensemble_corr:
            raise NotImplementedError("image_mask together with ensemble_corr=True is not implemented: the ensemble kernels and their "
                                      "float64 rescue have no masked form")
        if coarse_passes is not None and len(coarse_passes):
            raise NotImplementedError("image_mask together with coarse_passes is not implemented: the shifted kernels have no masked form")
        if window.deform_count(deform_passes):
            raise NotImplementedError("image_mask together with deform_passes is not implemented: the deformation kernels have no masked form")
        if flt is not None:
            raise NotImplementedError("image_mask together with spectral_filter is not implemented: the filtered kernels have no masked form")
        # (NotImplementedError with a search area, ValueError for another window, the coverage or the mask's shape)
        window_size = window.masked_spec(window_size, image_mask, mask_coverage_min, tuple(frames[0].shape))
    if flt is not None:
        if coarse_passes is not None and len(coarse_passes):
            raise NotImplementedError("spectral_filter together with coarse_passes is not implemented: the shifted kernels have no filtered form")
        if window.deform_count(deform_passes):
            raise NotImplementedError("spectral_filter together with deform_passes is not implemented: the deformation kernels have no filtered form")
        if isinstance(window_size, window.SearchWindow):
            window.filtered_spec(window_size, flt)     # NotImplementedError naming the two keywords
        if ensemble_window is not None:
            raise NotImplementedError("spectral_filter together with ensemble_window is not implemented: a sliding ensemble has no spectral filter")
    n_deform = window.deform_count(deform_passes)     # ValueError outside 0 .. 4
    if n_deform:
        if ensemble_corr:
            raise NotImplementedError("deform_passes with ensemble_corr=True is not implemented: a deformation pass is per pair")
        if isinstance(window_size, window.SearchWindow):
            raise NotImplementedError("deform_passes together with a search_area_size larger than the window is not implemented")
        if coarse_passes is None or not len(coarse_passes):
            window_size = window.multipass_spec(window_size, overlap, None, n_deform)   # a chain of one pass + D deformation passes
    if coarse_passes is not None and len(coarse_passes):
        if ensemble_corr and ensemble_window is not None:
            raise NotImplementedError("coarse_passes together with ensemble_window is not implemented: a sliding ensemble has no shifted pass")
        if isinstance(window_size, window.SearchWindow):
            raise NotImplementedError("coarse_passes together with a search_area_size larger than the window is not implemented")
        window_size = window.multipass_spec(window_size, overlap, coarse_passes, n_deform)   # ValueError for an unsupported chain
    if ensemble_corr and isinstance(window_size, window.SearchWindow):
        raise NotImplementedError("ensemble_corr=True with search_area_size != window_size is not implemented: the search-area kernels "
                                  "serve per-timestep mode only")
    if flt is not None:
        window_size = window.filtered_spec(window_size, flt)     # NotImplementedError with a search area, ValueError for another window
    if peak_ratio:
        if ensemble_corr:
            raise NotImplementedError("peak_ratio together with ensemble_corr=True is not implemented: the ensemble kernels have no "
                                      "second-peak form; use piv.second_peak on the mean planes instead")
        # (NotImplementedError naming the other keyword for another mode's window, ValueError for another window or radius)
        window_size = window.peak_ratio_spec(window_size, True, peak_exclusion)
    sliding = window.sliding_spec(ensemble_corr, ensemble_window, ensemble_stride)
    n_frames = len(frames)
    dim_size = tuple(frames[0].shape)
    dtype = frames.dtype if np.dtype(frames.dtype) in (np.dtype(np.uint8), np.dtype(np.float32)) else np.float64
    n_rows, n_cols = len(y), len(x)
    n_win = n_rows * n_cols
    if sliding is not None:
        return _get_ffpiv_sliding(frames, y, x, dt, window_size, overlap, res_y, res_x, chunksize, memory_factor, engine, corr_min, s2n_min,
                                  count_min, signal_threshold, time, prefetch, devices, sliding, n_frames, dim_size, dtype)
    chain = ensemble_corr and isinstance(window_size, window.MultiPassWindow)     # multi-pass ensemble
    if chain and _is_lazy(frames):
        raise NotImplementedError("coarse_passes with ensemble_corr=True and a lazy stack is not implemented: load the stack (numpy or "
                                  "DeviceFrames) first -- every pass reads the whole video, a lazy one would be computed once per pass")
    if chain:
        window.ensemble_chain_spec(window_size, dim_size)     # NotImplementedError for a steering pass of fewer than 3 x 3 windows
    _, ref_slices, slices = _plan_slices(n_frames, dim_size, window_size, overlap, dtype, chunksize, memory_factor, engine, n_win,
                                         ensemble_sums=chain)
    if time is None:
        time = frames["time"] if _is_xr(frames) else np.arange(n_frames)
    dt_arr = np.asarray(_values(dt), dtype=np.float64)
    if dt_arr.shape != (n_frames - 1,):
        raise ValueError(f"dt must have one entry per frame pair ({n_frames - 1}), got shape {dt_arr.shape}")
    devs = _resolve_frames_devices(frames, devices)
    align = window.chunk_alignment(window_size, dim_size, overlap)
    stack_mode = _stack_signal_mode(signal_threshold)
    # (a chain's later passes read every frame of a chunk at offsets of their own: a lazy stack takes the chunk-loading path; so do a
    # filtered, a masked and a second-peak run, whose per-pair entry points take chunks)
    resident_run = (_is_lazy(frames) and n_frames >= 2 and not stack_mode and
                    not isinstance(window_size, (window.MultiPassWindow, window.FilteredWindow, window.MaskedWindow, window.PeakRatioWindow)))
    if resident_run:
        # a lazy stack: resident in HBM, loads planned against HOST memory and cut where dask cuts, launches on the anchors
        work = plan_lazy_devices(frames, n_frames, dim_size, window_size, overlap, n_win, chunksize, memory_factor, engine, prefetch, devs)
    else:
        work = device_work(n_frames, slices, devs, align, stack_mode,
                           lambda a, b, d, cnt: _plan_slices(b - a + 1, dim_size, window_size, overlap, dtype, chunksize, memory_factor,
                                                             engine, n_win, d, cnt, ensemble_sums=chain)[2])
    if chain:
        return _run_ensemble_chain(frames, work, devs, time, window_size, dim_size, y, x, dt_arr, res_x, res_y, signal_threshold, corr_min,
                                   s2n_min, count_min, ref_slices)
    args = (n_frames - 1, len(work), y, x, dt_arr, res_x, res_y, window_size, overlap, signal_threshold)
    sink = (_ensemble_sink(*args, corr_min, s2n_min, count_min, ref_slices) if ensemble_corr else
            _timestep_sink(*args, **({} if validate is None else {"validate": validate})))
    if resident_run:
        return _run_resident(frames, work, sink, devs, time, signal_threshold)
    depth = (executor.default_depth() if prefetch is None else int(prefetch)) if hasattr(frames, "load") else 0
    return _run_chunks(frames, work, sink, depth, devs, time, window_size, overlap, (n_rows, n_cols))


def _add_variable(res, name, values):
    """One more (time, y, x) variable on a result of :func:`get_ffpiv`."""
    if isinstance(res, PivResult):
        res[name] = values
    else:
        res[name] = (["time", "y", "x"], values)


def lagged_slices(slices, n_frames: int, halo: int):
    """The frame slices ``[(a, b), ...]`` of :func:`aligned_slices` (pairs a .. b - 2, ONE halo frame) as lagged launches ``[(first pair,
    pairs, end frame), ...]``: the same pairs, frames ``[a, end)`` with a halo of min(``halo``, frames to the end of the stack) frames
    behind the last pair's frame t, so that no chunking changes a lag's clip."""
    return [(a, b - 1 - a, min(b - 1 + int(halo), n_frames)) for a, b in slices]


def _get_ffpiv_lagged(frames, y, x, dt, window_size, overlap, search_area_size, res_y, res_x, chunksize, memory_factor, engine, signal_threshold,
                      time, devices, lag, others):
    """``get_ffpiv`` with ``pair_step``: one ``piv.piv_pairs_lagged`` call per chunk, every chunk with its halo;
    the adaptive form's chunks are cut on the anchors of its lag-1 pass.  ``others``: which of the modes without a lagged form were asked for."""
    why = {"ensemble_corr": "the ensemble kernels have no lagged form", "ensemble_window": "a sliding ensemble has no lagged form",
           "coarse_passes": "a chain's shifted passes pair frame t with frame t+1", "deform_passes": "the deformation kernels have no lagged form",
           "spectral_filter": "the filtered kernels have no lagged form", "image_mask": "the masked kernels have no lagged form",
           "peak_ratio": "the second-peak kernels have no lagged form", "validate": "run validate.median_test on the result instead"}
    for key, asked in others.items():
        if asked:
            raise NotImplementedError(f"pair_step together with {key}{'=True' if key in ('ensemble_corr', 'peak_ratio') else ''} is not "
                                      f"implemented: {why[key]}")
    ws, ov = window.lag_supported(window_size), (int(overlap[0]), int(overlap[1]))
    if search_area_size is not None and tuple(int(q) for q in search_area_size) != ws:
        raise NotImplementedError("pair_step together with a search_area_size larger than the window is not implemented: the lag kernels "
                                  "correlate two windows of one size")
    if devices is not None:
        raise NotImplementedError("pair_step together with devices= is not implemented: the block cuts of several devices assume one halo frame")
    if _is_lazy(frames):
        raise NotImplementedError("pair_step with a lazy stack is not implemented: load the stack (numpy or DeviceFrames) first -- the "
                                  "loaders' block cuts assume one halo frame")
    n_frames, dim_size = len(frames), tuple(frames[0].shape)
    dtype = frames.dtype if np.dtype(frames.dtype) in (np.dtype(np.uint8), np.dtype(np.float32)) else np.float64
    n_pairs, grid = n_frames - 1, (len(y), len(x))
    n_win = grid[0] * grid[1]
    if tuple(window.get_array_shape(dim_size, ws, ov)) != grid:
        raise ValueError(f"grid {tuple(window.get_array_shape(dim_size, ws, ov))} does not match coordinates {grid}")
    dt_arr = np.asarray(_values(dt), dtype=np.float64)
    if dt_arr.shape != (n_pairs,):
        raise ValueError(f"dt must have one entry per frame pair ({n_pairs}), got shape {dt_arr.shape}")
    if time is None:
        time = frames["time"] if _is_xr(frames) else np.arange(n_frames)

    def need(n):   # HBM bytes of a launch of n - 1 pairs with its halo, the tables and -- adaptive -- the lag-1 field (in the result block)
        return window.lag_required_memory(n - 1, min(lag.halo, n_frames - 1), dim_size, ws, ov, dtype, lag)

    avail = window.available_memory() / memory_factor
    cs, _ = plan_chunks(n_frames, need(n_frames), avail, chunksize, engine, n_win=n_win)
    align = window.chunk_alignment(ws, dim_size, ov) if lag.form == window.LAG_ADAPTIVE else 1
    launches = lagged_slices(aligned_slices(n_frames, cs, align, n_win=n_win, fits=lambda n: need(n) <= avail), n_frames, lag.halo)
    full = {k: np.empty((n_pairs, *grid), dtype=np.float32) for k in ("s2n", "corr", "v_x", "v_y")}
    full["pair_step"] = np.empty((n_pairs, *grid), dtype=np.uint8)
    for a, p, end in launches:
        u, v, cm, sn, k = piv.piv_pairs_lagged(_values(load_frame_chunk(frames[a:end])), ws, ov, lag, signal_threshold=signal_threshold, pair_offset=a,
                                               out=(full["v_x"][a:a + p], full["v_y"][a:a + p], full["corr"][a:a + p], full["s2n"][a:a + p]),
                                               pairs=p)
        _to_velocity(u, res_x, dt_arr[a:a + p, None, None], out=u)
        _to_velocity(v, res_y, dt_arr[a:a + p, None, None], out=v)
        full["pair_step"][a:a + p] = k
    t = time[1:]
    return _dataset(full, t, y, x, frames)


def _run_ensemble_chain(frames, work, devices, time, spec, dim_size, y, x, dt, res_x, res_y, signal_threshold, corr_min, s2n_min, count_min,
                        ref_slices):
    """The multi-pass ensemble: the passes of ``spec`` are the outer loop, the chunk loop of the ensemble sink
    over ``work`` -- ONE chunk plan for the whole chain, cut on pass 0's anchors -- the inner one.  Every pass is accumulated per device
    worker, all-reduced and finished as the plain ensemble is; its field, in the kernels' orientation, goes through the predictor and the
    resulting offsets (a few KB, through the host) are set on every worker's handle of the next pass.  The last pass's sink builds the
    result on the coordinates ``y``, ``x``."""
    n_pairs = len(dt)
    prev = out = None
    for k, (n, ov) in enumerate(spec.passes):
        ws, ovk = (n, n), (ov, ov)
        last = k == len(spec.passes) - 1
        grid = (len(y), len(x)) if last else tuple(window.get_array_shape(dim_size, ws, ovk))
        shift = None if k == 0 else piv.predict_shift(prev[0], prev[1], dim_size, spec.passes[k - 1], (n, ov))[0]
        yk, xk = (y, x) if last else (np.arange(grid[0]), np.arange(grid[1]))
        sink = _ensemble_sink(n_pairs, len(work), yk, xk, dt, res_x, res_y, ws, ovk, signal_threshold, corr_min, s2n_min, count_min, ref_slices,
                              shift=shift, field_only=not last)
        out = _run_chunks(frames, work, sink, 0, devices, time, ws, ovk, grid)
        prev = out
    return out


def sliding_labels(time, dt, M: int, s: int, n_out: int):
    """(time label, dt_j) of every output of a sliding ensemble: the mean second-frame time and the mean ``dt`` of its M pairs."""
    t2 = np.asarray(time, dtype=np.float64)[1:]
    dt = np.asarray(dt, dtype=np.float64)
    return (np.array([t2[j * s:j * s + M].mean() for j in range(n_out)]), np.array([dt[j * s:j * s + M].mean() for j in range(n_out)]))


def _get_ffpiv_sliding(frames, y, x, dt, window_size, overlap, res_y, res_x, chunksize, memory_factor, engine, corr_min, s2n_min, count_min,
                       signal_threshold, time, prefetch, devices, sliding, n_frames, dim_size, dtype):
    """``get_ffpiv`` with ``ensemble_window``: the chunk loop of the ensemble mode on chunks cut on multiples of s pairs, one sliding
    ``Ensemble`` handle, a result with one time step per output (:func:`_sliding_sink`)."""
    M, s = sliding
    n_win = len(y) * len(x)
    if _is_lazy(frames):
        raise NotImplementedError("ensemble_window with a lazy stack is not implemented: load the stack (numpy or DeviceFrames) first")
    n_blk, n_out = window.sliding_outputs(n_frames - 1, M, s)
    many = "ensemble_window with devices={} is not implemented: a sliding ensemble runs on one device"
    if devices is not None and not isinstance(devices, str) and len(list(devices)) > 1:
        raise NotImplementedError(many.format(list(devices)))
    devs = _resolve_frames_devices(frames, devices)
    if devs is not None and len(devs) > 1:
        raise NotImplementedError(many.format(list(devs)))
    slices = plan_sliding_slices(n_frames, dim_size, window_size, overlap, dtype, chunksize, memory_factor, engine, n_win, s,
                                 None if devs is None else devs[0])
    if time is None:
        time = frames["time"] if _is_xr(frames) else np.arange(n_frames)
    dt_arr = np.asarray(_values(dt), dtype=np.float64)
    if dt_arr.shape != (n_frames - 1,):
        raise ValueError(f"dt must have one entry per frame pair ({n_frames - 1}), got shape {dt_arr.shape}")
    sink = _sliding_sink(n_frames - 1, y, x, dt_arr, res_x, res_y, window_size, overlap, signal_threshold, corr_min, s2n_min, count_min, M, s,
                         n_out)
    depth = (executor.default_depth() if prefetch is None else int(prefetch)) if hasattr(frames, "load") else 0
    return _run_chunks(frames, [slices], sink, depth, devs, time, window_size, overlap, (len(y), len(x)))


def plan_sliding_slices(n_frames, dim_size, window_size, overlap, dtype, chunksize, memory_factor, engine, n_win, s, device=None):
    """The chunk plan of a sliding ensemble: the planner of :func:`_plan_slices` with the run's block store counted next to every
    chunk, and chunks of a multiple of s pairs (>= one block) -- ``window.chunk_alignment`` keeps its meaning for the other modes."""
    blocks = -(-(n_frames - 1) // s)     # (a trailing partial block has a slot too)

    def need(n):
        return window.required_memory(n_frames=n, dim_size=dim_size, window_size=window_size, overlap=overlap, dtype=dtype,
                                      sliding_blocks=blocks)

    with executor.on_device(device):
        avail = window.available_memory() / memory_factor
    cs, _ = plan_chunks(n_frames, need(n_frames), avail, chunksize, engine, n_win=n_win)
    if cs >= n_frames and (n_frames - 1) * max(n_win, 1) <= MAX_WINDOWS_PER_LAUNCH:
        return [(0, n_frames)]     # the whole stack in one call: the trailing pairs ride along (the last call may end inside a block)
    slices = aligned_slices(n_frames, cs, s, n_win=n_win, fits=lambda n: need(n) <= avail)
    if len(slices) > 1 and (slices[0][1] - 1) % s != 0:
        # aligned_slices fell back to chunks off the blocks: a sliding handle takes whole blocks only (all calls but the last)
        raise ValueError(f"ensemble_stride {s}: a block of {s} pairs ({s + 1} frames, {need(s + 1)} bytes with the block store of {blocks} blocks) does "
                         f"not fit one call -- {int(avail)} bytes are available (memory_factor, chunksize {chunksize}) and one launch takes "
                         f"{MAX_WINDOWS_PER_LAUNCH} windows, this grid has {n_win} per pair; use a smaller ensemble_stride")
    return slices


# ---------------------------------------------------------------------------------------------------------------------------------
# several devices from one process: who computes which pairs
# ---------------------------------------------------------------------------------------------------------------------------------
def _resolve_frames_devices(frames, devices):
    """``devices`` of :func:`get_ffpiv` -> None or a list of device indices, checked before any GPU work.  A ``DeviceFrames`` stack
    lives on one device: ``"all"`` runs it there, a list may only name that device (its workers would share one HBM stack and gain
    nothing: it runs as one worker)."""
    if devices is None:
        return None
    from . import _lib

    devs = executor.resolve_devices(devices, _lib.device_count())
    if is_device(frames):
        home = frames.device
        if not isinstance(devices, str) and any(d != home for d in devs):
            raise ValueError(f"devices={list(devs)}: the DeviceFrames stack lives on device {home}")
        return [home]
    return devs


def device_work(n_frames: int, slices, devices, align: int, whole_chunks: bool, plan_block):
    """Per device worker, the frame slices ``[(a, b), ...]`` it launches (pair ``p`` = frames ``p, p + 1``; consecutive slices share
    one frame, as in :func:`aligned_slices`).

    * ``devices`` None: one worker with ``slices`` (the single-device plan) -- what ``get_ffpiv`` has always run;
    * ``whole_chunks`` (the "stack" reading of ``signal_threshold``, whose statistic depends on the chunk cut): the chunks of the
      single-device plan, dealt out as contiguous runs balanced to within one chunk (``shard.pair_block`` over the chunk list) -- the
      bits cannot move; workers beyond the number of chunks stay idle;
    * otherwise D contiguous pair blocks on the anchors (``shard.pair_block`` with ``align``: balanced to within one anchor); the
      block ``[a, b)`` of worker ``k`` is cut into chunks by ``plan_block(a, b, device, workers on that device)`` (frame slices
      relative to ``a``, planned against that device's memory) -- every chunk still starts on an anchor.  Workers beyond the number
      of anchors stay idle."""
    from . import shard

    if devices is None:
        return [list(slices)]
    D = len(devices)
    if whole_chunks:
        return [list(slices[i0:i1]) for i0, i1 in (shard.pair_block(len(slices), k, D) for k in range(D))]
    n_pairs = n_frames - 1
    out = []
    for k, d in enumerate(devices):
        a, b = shard.pair_block(n_pairs, k, D, align)
        out.append([(a + s0, a + s1) for s0, s1 in plan_block(a, b, d, devices.count(d))] if b > a else [])
    return out


def _plan_slices(n_frames, dim_size, window_size, overlap, dtype, chunksize, memory_factor, engine, n_win, device=None, share=1,
                 ensemble_sums=False):
    """The chunk plan of :func:`get_ffpiv` for ``n_frames`` frames against the HBM of ``device`` (None: the calling thread's) that
    ``share`` workers divide -> (chunksize, the reference planner's slices -- quirk Q3 counts them --, the slices launched: on the
    anchors, :func:`aligned_slices`).  ``ensemble_sums``: the plane sums of an ensemble stay in HBM next to every chunk (the multi-pass
    ensemble counts them, for its largest pass)."""
    def need(n):   # HBM bytes of one launch on n frames
        return window.required_memory(n_frames=n, dim_size=dim_size, window_size=window_size, overlap=overlap, dtype=dtype,
                                      ensemble_sums=ensemble_sums)

    req = need(n_frames)
    with executor.on_device(device):
        avail = window.available_memory() / memory_factor / share
    cs, ref_slices = plan_chunks(n_frames, req, avail, chunksize, engine, n_win=n_win)
    align = window.chunk_alignment(window_size, dim_size, overlap)
    return cs, ref_slices, aligned_slices(n_frames, cs, align, n_win=n_win, fits=lambda n: need(n) <= avail)


def _merge_stats(per_device, devices) -> dict:
    """``executor.LAST_STATS`` of a run: the keys of one worker's statistics (times and chunk counts summed, per-chunk lists in pair
    order, depths maxed), plus ``devices`` and ``per_device`` (each worker's own statistics, in worker order)."""
    active = [st for st in per_device if st]
    if len(per_device) == 1:
        out = dict(per_device[0] or {})
    else:
        out = {}
        for st in active:
            for key, v in st.items():
                if key == "plan" or key == "ensemble":
                    continue
                if isinstance(v, bool):
                    out[key] = out.get(key, False) or v
                elif key in ("depth", "max_depth"):
                    out[key] = max(out.get(key, 0), v)
                elif isinstance(v, (int, float)):
                    out[key] = out.get(key, 0) + v
                elif isinstance(v, list):
                    out[key] = out.get(key, []) + list(v)
        plans = [st["plan"] for st in active if "plan" in st]
        if plans:
            plan = dict(plans[0])
            plan["windows"] = [w for pl in plans for w in pl["windows"]]
            for key in ("peak_host_bytes", "host_budget"):
                plan[key] = sum(pl[key] for pl in plans)
            plan["load_frames"] = max(pl["load_frames"] for pl in plans)
            out["plan"] = plan
            # the halo frame of every block after the first is loaded by both neighbours
            out["boundary_frames"] = max(0, len(plans) - 1)
    out["devices"] = None if devices is None else list(devices)
    out["per_device"] = [dict(st) if st else {} for st in per_device]
    out["idle_devices"] = sum(1 for st in per_device if not st)
    return {k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}


_to_velocity = piv._to_velocity      # (disp * res / dt).astype(float32) with numpy's own arithmetic, into a slice of the run's arrays


# ---------------------------------------------------------------------------------------------------------------------------------
# where the launches write: one sink per mode, a tuple (launch, close, result) --
#   launch(k, frames, p0, p1): pairs [p0, p1) (frames p0 .. p1) on device worker k, called on that worker's thread;
#   close(per_device):         release what the workers hold (and note it in their statistics, per_device[k]);
#   result(time, like):        the Dataset / PivResult of everything launched.
# ---------------------------------------------------------------------------------------------------------------------------------
def _delivered(full, done):
    """``full`` (the run's result arrays, allocated once, every launch writing its time slice) when every pair was delivered, in order;
    else the ``done`` ranges of it concatenated (a chunk lost trailing frames -- load_frame_chunk's TypeError retry -- or was
    skipped).  ``done``: (first pair, one past the last pair) of every launch, sorted."""
    if not done:
        raise ValueError("no chunk with at least one frame pair")
    n = len(next(iter(full.values())))
    if done[0][0] == 0 and done[-1][1] == n and all(a[1] == b[0] for a, b in zip(done, done[1:])):
        return full
    return {k: np.concatenate([v[i:j] for i, j in done], axis=0) for k, v in full.items()}


def _timestep_sink(n_pairs, n_workers, y, x, dt, res_x, res_y, window_size, overlap, signal_threshold, validate=None):
    """Per-timestep PIV (pyorc/velocimetry/ffpiv.py:379-443).  The four result variables of the WHOLE run are allocated once and every
    launch writes its time slice of them (corr, s2n straight from the library, v_x / v_y through the px -> m/s scaling): no per-chunk
    arrays to concatenate at the end (the reference's xr.concat, ffpiv.py:442 -- 125 KB per pair, i.e. as many bytes again as a uint8
    chunk's upload at 32 x 32)."""
    peak2 = isinstance(window_size, window.PeakRatioWindow)     # (four more variables)
    names = ("s2n", "corr", "v_x", "v_y") + (("peak_ratio", "corr2", "v_x2", "v_y2") if peak2 else ())
    full = {k: np.empty((n_pairs, len(y), len(x)), dtype=np.float32) for k in names}
    if validate is not None:      # (the median test's flags)
        full["flag"] = np.empty((n_pairs, len(y), len(x)), dtype=np.uint8)
    done = []
    px = [None] * n_workers            # per worker: scratch for a launch's u, v in pixels
    # (the modes whose entry points have no fused scaling: numpy's arithmetic on the host, the same bits)
    on_device = piv.device_scaling_is_numpys(res_x, res_y) and not isinstance(window_size, piv._HOST_SCALED)

    def launch(k, frames, p0, p1):
        p = p1 - p0
        dt_chunk = dt[p0:p1]  # dt.sel(time=da.time[1:]), ffpiv.py:403-404
        if on_device:
            # u and v to meter per second on the device, before they cross PCIe: the arithmetic of ffpiv.py:418-419 for python-float
            # resolutions (float32 product, float64 division, float32 storage)
            uv, scale = (full["v_x"][p0:p1], full["v_y"][p0:p1]), (res_x, res_y, dt_chunk)
        else:
            # ... in pixels, scaled on the host with numpy's own arithmetic for any other kind of resolution (a numpy float64 scalar
            # makes the product float64)
            if px[k] is None or px[k][0].shape[0] < p:
                px[k] = [np.empty((p, len(y), len(x)), dtype=np.float32) for _ in range(2)]
            uv, scale = (px[k][0][:p], px[k][1][:p]), None
        ret = piv.piv_pairs(frames, window_size, overlap, signal_threshold, pair_offset=p0, scale=scale,
                            out=uv + (full["corr"][p0:p1], full["s2n"][p0:p1]),
                            **({} if validate is None else {"validate": validate}))
        if validate is not None:      # validated in pixels inside the call, before either scaling
            full["flag"][p0:p1] = ret[-1]
        if scale is None:
            _to_velocity(uv[0], res_x, dt_chunk[:, None, None], out=full["v_x"][p0:p1])
            _to_velocity(uv[1], res_y, dt_chunk[:, None, None], out=full["v_y"][p0:p1])
        if peak2:     # (u2, v2, corr2, peak_ratio) per window: the runner-up vector scaled like u, v (host arithmetic: scale is None here)
            second = ret[4]
            _to_velocity(second[..., 0], res_x, dt_chunk[:, None, None], out=full["v_x2"][p0:p1])
            _to_velocity(second[..., 1], res_y, dt_chunk[:, None, None], out=full["v_y2"][p0:p1])
            full["corr2"][p0:p1] = second[..., 2]
            full["peak_ratio"][p0:p1] = second[..., 3]
        done.append((p0, p1))

    def result(time, like):
        done.sort()
        data = _delivered(full, done)
        times = [time[i + 1:j + 1] for i, j in done]
        t = xr.concat(times, dim="time") if _is_xr(like) else np.concatenate([np.asarray(tt) for tt in times])
        return _dataset(data, t, y, x, like)

    return launch, lambda per_device: None, result


def _ensemble_sink(n_pairs, n_workers, y, x, dt, res_x, res_y, window_size, overlap, signal_threshold, corr_min, s2n_min, count_min,
                   ref_slices, shift=None, field_only=False):
    """Ensemble correlation (pyorc/velocimetry/ffpiv.py:182-376): every device worker accumulates its pairs into an ``Ensemble`` handle
    of its own (corr_sum / corr_count stay in HBM); the masked per-pair corr_max / s2n of the whole run are allocated once and every
    launch writes its time slice (the ``out`` of ``Ensemble.accumulate``).  One handle finishes as it always has; several are reduced
    device to device (``piv.ensemble_allreduce``) and finished with every device's float64 rescue (``shard.staged_finish``).
    A pass of a multi-pass ensemble (:func:`_run_ensemble_chain`): ``shift`` (n_rows, n_cols, 2) makes the handles shifted ones
    with these offsets; ``field_only``: the result is the pass's ``(u, v)`` in pixels and in the kernels' orientation, for the predictor."""
    full = {k: np.empty((n_pairs, len(y) * len(x)), dtype=np.float32) for k in ("corr", "s2n")}
    done = []
    handles = [None] * n_workers

    def launch(k, frames, p0, p1):
        if handles[k] is None:   # made on the worker's thread: on the worker's device
            handles[k] = piv.Ensemble(tuple(frames.shape[1:]), window_size, overlap, **({} if shift is None else {"shift": shift}))
        handles[k].accumulate(frames, corr_min, s2n_min, signal_threshold, out=(full["corr"][p0:p1], full["s2n"][p0:p1]))
        done.append((p0, p1))

    def close(per_device):
        for k, h in enumerate(handles):
            if h is None:
                continue
            with executor.on_device(getattr(h, "device", None)):
                if per_device[k] is not None:
                    per_device[k]["ensemble"] = h.stats() if hasattr(h, "stats") else {}
                h.close()

    def result(time, like):
        from . import shard

        done.sort()
        data = _delivered(full, done)
        # quirk Q3: `n_frames` is the number of CHUNKS, not pairs (ffpiv.py:373), and `time[0:1]` of the LAST chunk ends up on the
        # result (ffpiv.py:336) -- both taken from the reference's own chunk plan (same formula, fed with HBM figures), not from the
        # chunks that were launched, so neither depends on the segment anchoring, on the loads or on the number of devices
        assert ref_slices   # plan_chunks' first slice is (0, min(chunksize, n_frames)) with chunksize >= 2; fewer frames raised above
        n_chunks, last = len(ref_slices), ref_slices[-1][0]
        live = [h for h in handles if h is not None]
        if len(live) == 1:
            with executor.on_device(getattr(live[0], "device", None)):
                u, v, corr_count = live[0].finish(count_min, n_chunks)
        else:
            with executor.on_device(getattr(live[0], "device", None)):
                piv.ensemble_allreduce(live)
            u, v, corr_count = shard.staged_finish(live, count_min, n_chunks)
        if field_only:
            from . import _lib

            return u, (-v if _lib.get_option("v_sign") == 1 else v)      # (a negation is exact)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            # very low amounts of found valid correlations are entirely filtered out (ffpiv.py:280-286)
            data["corr"][:, corr_count < count_min * n_chunks] = np.nan
            corr_mean = np.nanmean(data["corr"], axis=0).reshape(-1, len(y), len(x))
            s2n_mean = np.nanmean(data["s2n"], axis=0).reshape(-1, len(y), len(x))
        dt_av = dt.mean()
        data = {"s2n": s2n_mean, "corr": corr_mean, "v_x": (u * res_x / dt_av).astype(np.float32),
                "v_y": (v * res_y / dt_av).astype(np.float32)}
        return _dataset(data, time[last + 1:last + 2], y, x, like)

    return launch, close, result


def _sliding_sink(n_pairs, y, x, dt, res_x, res_y, window_size, overlap, signal_threshold, corr_min, s2n_min, count_min, M, s, n_out):
    """The ensemble sink for a sliding ensemble: one handle with a block store, ``n_out`` time steps.
    ``corr`` / ``s2n`` of output j: nanmean over its M pairs of the masked per-pair values, the windows below ``count_min * M`` set to
    NaN first (as ffpiv.py:284-286 does for the one ensemble); velocities with the mean ``dt`` of those pairs."""
    full = {k: np.empty((n_pairs, len(y) * len(x)), dtype=np.float32) for k in ("corr", "s2n")}
    done = []
    handle = [None]

    def launch(k, frames, p0, p1):
        if handle[0] is None:
            handle[0] = piv.Ensemble(tuple(frames.shape[1:]), window_size, overlap, sliding=(M, s))
            handle[0].reserve_sliding(n_pairs)     # the whole run's block store at once: what plan_sliding_slices counted
        handle[0].accumulate(frames, corr_min, s2n_min, signal_threshold, out=(full["corr"][p0:p1], full["s2n"][p0:p1]))
        done.append((p0, p1))

    def close(per_device):
        h = handle[0]
        if h is not None:
            with executor.on_device(getattr(h, "device", None)):
                if per_device[0] is not None:
                    per_device[0]["ensemble"] = h.stats() if hasattr(h, "stats") else {}
                h.close()

    def result(time, like):
        done.sort()
        if not done or done[0][0] != 0 or done[-1][1] != n_pairs or any(a[1] != b[0] for a, b in zip(done, done[1:])):
            raise ValueError("ensemble_window: a chunk lost frames while it was loaded; the outputs of a sliding ensemble need every pair")
        h = handle[0]
        with executor.on_device(getattr(h, "device", None)):
            u, v, cnt = h.finish_sliding(count_min)
        low = cnt.reshape(n_out, -1) < np.float32(count_min) * np.float32(M)     # the device's threshold, in its arithmetic
        corr = np.empty((n_out, len(y) * len(x)), dtype=np.float32)
        s2n = np.empty_like(corr)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            for j in range(n_out):
                c = full["corr"][j * s:j * s + M].copy()
                c[:, low[j]] = np.nan
                corr[j] = np.nanmean(c, axis=0)
                s2n[j] = np.nanmean(full["s2n"][j * s:j * s + M], axis=0)
        t_out, dt_out = sliding_labels(np.asarray(time), dt, M, s, n_out)
        shape = (n_out, len(y), len(x))
        data = {"s2n": s2n.reshape(shape), "corr": corr.reshape(shape),
                "v_x": (u * res_x / dt_out[:, None, None]).astype(np.float32), "v_y": (v * res_y / dt_out[:, None, None]).astype(np.float32)}
        return _dataset(data, t_out, y, x, like)

    return launch, close, result


# ---------------------------------------------------------------------------------------------------------------------------------
# the drivers: which frames reach the sink, on which device worker
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_workers(sink, devices, run, per_device, time, like):
    """``run(k, stop)`` on every device worker, each on a thread of its own, then the sink's result.  Whatever happens, the sink is
    closed and ``executor.LAST_STATS`` written -- once, by the calling thread: the workers only fill their own ``per_device`` entry."""
    _, close, result = sink
    try:
        executor.run_on_devices(devices, run)
        return result(time, like)
    finally:
        close(per_device)
        executor.LAST_STATS.clear(); executor.LAST_STATS.update(_merge_stats(per_device, devices))


def _run_chunks(frames, work, sink, prefetch, devices, time, window_size, overlap, grid):
    """The chunk loops of pyorc/velocimetry/ffpiv.py:348-370 and :399-440 (one fused GPU call per chunk); chunk n + 1 is loaded on a
    worker thread while chunk n is launched (``pyorc_amd.executor.ChunkPrefetcher``; ``prefetch = 0``: the reference's serial order).
    ``work``: the chunk slices of every device worker (:func:`device_work`), each worker loops over its own on its own device;
    ``grid``: (rows, columns) of the coordinates."""
    launch = sink[0]
    per_device = [None] * len(work)

    def run(k, stop):
        slices = work[k]
        if not slices:
            return
        frames_chunks = [frames[a:b] for a, b in slices]
        loader = executor.ChunkPrefetcher(frames_chunks, load_frame_chunk, depth=prefetch)
        try:
            for n, da in loader:
                executor.stop_point(stop)
                if len(da) >= 2:  # we need at least one image-pair to do PIV
                    vals = _values(da)
                    got = tuple(window.get_array_shape(tuple(vals.shape[1:]), window_size, overlap))
                    if got != grid:
                        raise ValueError(f"grid {got} does not match coordinates {grid}")
                    a = slices[n][0]
                    launch(k, vals, a, a + len(da) - 1)   # load_frame_chunk may have dropped trailing frames
                # remove chunk safely from memory.  (The reference follows this with gc.collect() to get rid of its window stack and
                # correlation volume, ffpiv.py:437-440; neither exists here, and a collection costs ~1 ms per chunk: dropped.)
                frames_chunks[n] = None
                del da
        finally:
            # also when a launch raises in the loop body: the worker threads stop loading the next chunks NOW, not when the traceback is
            # collected, and the statistics of what ran are kept
            loader.close()
            per_device[k] = loader.stats

    return _run_workers(sink, devices, run, per_device, time, frames)


# ---------------------------------------------------------------------------------------------------------------------------------
# lazy stacks (round 6): resident in HBM, loads against the host budget on dask's block boundaries, launches on the anchors
# ---------------------------------------------------------------------------------------------------------------------------------
def _is_lazy(frames) -> bool:
    """Something that materialises on ``load()``: pyorc's dask-backed DataArray.  An ``xr.DataArray`` that is already in memory has a
    ``load()`` too; its ``.data`` (the backing array: looking at it computes nothing) is a numpy array, and it runs as one."""
    if is_device(frames) or not hasattr(frames, "load"):
        return False
    return not isinstance(getattr(frames, "data", None), np.ndarray)


def _stack_signal_mode(signal_threshold) -> bool:
    """The "stack" reading of ``signal_threshold`` scores a window position over all frames of a CHUNK (include/lspiv.h, option
    ``signal_mode`` = 1): its results depend on the chunking by definition, so such a run keeps the chunk loop it was defined on."""
    if signal_threshold is None:
        return False
    from . import _lib

    try:
        return _lib.get_option("signal_mode") == 1
    except Exception:
        return False


def _lazy_source(frames, handoff):
    """The stack a lazy run loads: ``frames`` itself, or for a ``project_hip`` hand-off (``plugin.hip_projection_source``) its camera
    frames -- or, when those are the recipe's filters over a uint8 stack (``ops``), that stack (``root``)."""
    if handoff is None:
        return frames
    return handoff["root"] if handoff.get("ops") else handoff["source"]


class LazyPlan(dict):
    """What :func:`plan_lazy` decided (a dict, for the tests and ``executor.LAST_STATS``): ``windows`` [(w0, w1)] frame ranges resident at
    a time, ``loads`` per window [(f0, f1)], ``load_frames``, ``host_budget`` / ``host_frame_bytes`` / ``peak_host_bytes``, ``depth`` (None =
    adaptive) and ``max_depth``, ``align``, ``blocks`` (dask's), ``source`` ("frames" | "camera": the pre-projection stack of project_hip),
    ``chain`` (a ``filters.Chain`` when the camera frames are the recipe's filters over a uint8 stack: that stack is loaded, the filters run
    on the device) and ``hbm_scratch`` (bytes of HBM next to the resident stack)."""


def plan_lazy(frames, n_frames, dim_size, window_size, overlap, n_win, chunksize, memory_factor, engine, prefetch,
              host_available=None, hbm_available=None, first=0, stop=None, host_share=1) -> LazyPlan:
    """How a lazy stack runs.  The reference's planner (ffpiv.py:119-139) with its own quantities where they still mean something:

    * what a load materialises is bounded by the HOST: ``available_memory() / memory_factor`` (ffpiv.py:129) divided by the loads the
      executor may keep in flight (``max_depth + 1``, or ``prefetch + 1`` when the caller fixed it), in frames of the stack that is
      actually loaded (the camera frames when the stack is ``project_hip``'s product); at 5 frames or fewer the reference's warning is
      raised and 5 it is (ffpiv.py:131-137); a user ``chunksize`` is honoured as the load size;
    * below that bound, loads are the overlap granule of ``pyorc_amd.resident.load_size`` -- at least ``MIN_LOADS`` of them when the
      stack has that many anchors -- in whole dask blocks;
    * what is resident at a time is bounded by HBM (``lspiv_available_bytes / memory_factor``): normally everything, less the scratch of
      the pieces being staged (a filter chain's: ``max_depth + 1`` pieces of its uint8 upload and outputs, and its mean plane).

    ``first`` / ``stop``: the frame range of ONE device's block (:func:`plan_lazy_devices`; ``first`` on an anchor), ``host_share``: how
    many devices' loaders share the host budget -- each gets that fraction of it and of ``max_depth`` (at least one load ahead)."""
    from . import plugin

    align = window.chunk_alignment(window_size, dim_size, overlap)
    handoff = plugin.hip_projection_source(frames)
    chain = None
    if handoff is not None and handoff.get("ops"):
        from .filters import Chain

        chain = Chain(handoff["ops"])
    src = _lazy_source(frames, handoff)
    src_shape = tuple(int(v) for v in (src[0].shape if handoff is not None else dim_size))
    host_frame_bytes = int(np.prod(src_shape)) * np.dtype(src.dtype).itemsize
    blocks = resident.time_blocks(src)
    if prefetch is None and executor.adaptive_by_default():
        depth, deepest = None, executor.max_depth()
        if host_share > 1:
            deepest = max(1, deepest // host_share)
    else:
        depth = executor.default_depth() if prefetch is None else int(prefetch)
        if host_share > 1 and depth > 0:
            depth = max(1, depth // host_share)
        deepest = depth
    stop = n_frames if stop is None else int(stop)
    first = int(first)
    host_avail = window.available_host_memory() if host_available is None else host_available
    host_budget = host_avail / memory_factor / max(1, host_share)
    if chunksize is None:
        host_frames = int(host_budget // ((deepest + 1) * host_frame_bytes))
        if host_frames <= 5:
            warnings.warn(CHUNK_SIZE_WARNING.format(avail_mem=host_budget / 1e9, chunksize=host_frames, engine=engine), stacklevel=4)
            host_frames = 5  # hard override, try to manage with 5
        load_frames = resident.load_size(stop - first, align, host_frames, blocks)
    else:
        load_frames = int(chunksize)
        if load_frames < 2:
            raise OverflowError(CHUNK_SIZE_ERROR.format(chunks=int(np.ceil(n_frames / max(load_frames, 1)))))
    # HBM: the narrowed stack + the result block (+ one load of camera frames next to it when they are projected on the device)
    dev_itemsize = 4 if handoff is not None else resident.DeviceFrames.device_dtype(frames.dtype).itemsize
    hbm_avail = (window.available_memory() if hbm_available is None else hbm_available) / memory_factor
    per_frame = int(np.prod(dim_size)) * dev_itemsize + 16 * n_win
    scratch = load_frames * host_frame_bytes if handoff is not None else 0
    if chain is not None:
        # every loader thread stages a piece at a time: its upload and the chain's outputs, + the mean plane
        cam_pixels = int(np.prod(src_shape))
        scratch = (deepest + 1) * load_frames * chain.scratch_bytes_per_pixel * cam_pixels + (4 * cam_pixels if chain.samples else 0)
    frames_per_window = max(align + 1, int((hbm_avail - scratch) // per_frame))
    frames_per_window = min(frames_per_window, max(2, MAX_WINDOWS_PER_LAUNCH // max(n_win, 1)))
    windows = [(first + w0, first + w1) for w0, w1 in resident.hbm_windows(stop - first, frames_per_window, align, blocks)]
    loads = [resident.plan_loads(w1, load_frames, blocks, first=w0) for w0, w1 in windows]
    biggest = max((b - a for ls in loads for a, b in ls), default=0)
    return LazyPlan(windows=windows, loads=loads, load_frames=load_frames, align=align, blocks=blocks, depth=depth, max_depth=deepest,
                    host_budget=host_budget, host_frame_bytes=host_frame_bytes, peak_host_bytes=(deepest + 1) * biggest * host_frame_bytes,
                    source="frames" if handoff is None else "camera", handoff=handoff, chain=chain, hbm_scratch=scratch)


def lazy_unit(align: int, blocks, n_frames: int, n_devices: int) -> int:
    """The unit the device blocks of a lazy stack are cut in: whole anchors, and whole dask blocks as well (their common multiple)
    when the blocks are regular and the stack still has a unit for every device; else whole anchors."""
    if not blocks or len(blocks) <= 2:
        return align
    lens = np.diff(blocks)[:-1]           # the last block may be short
    typical = int(lens[0]) if len(lens) else 0
    if typical <= 0 or any(int(v) != typical for v in lens):
        return align
    both = align * typical // math.gcd(align, typical)
    return both if -(-(n_frames - 1) // both) >= n_devices else align


def plan_lazy_devices(frames, n_frames, dim_size, window_size, overlap, n_win, chunksize, memory_factor, engine, prefetch, devices,
                      host_available=None, hbm_available=None):
    """One :func:`plan_lazy` per device worker (``[plan]`` for ``devices`` None: the single-device run).  Worker ``k`` gets the frames of
    pair block ``shard.frame_block(n_pairs, k, D, unit)`` (:func:`lazy_unit`: anchors, and dask's blocks where possible; its halo frame
    is the first frame of the next block: loaded by both), a 1/D share of the host budget and of the loads in flight, and a plan of
    its own against the HBM of its device (shared by the workers on that device).  A worker without pairs gets None.
    ``host_available`` / ``hbm_available``: figures for the tests (per device: a callable of the device index, or a number)."""
    from . import plugin, shard

    if devices is None:
        return [plan_lazy(frames, n_frames, dim_size, window_size, overlap, n_win, chunksize, memory_factor, engine, prefetch,
                          host_available=host_available, hbm_available=hbm_available)]
    D = len(devices)
    align = window.chunk_alignment(window_size, dim_size, overlap)
    unit = lazy_unit(align, resident.time_blocks(_lazy_source(frames, plugin.hip_projection_source(frames))), n_frames, D)
    host = window.available_host_memory() if host_available is None else host_available
    plans = []
    for k, d in enumerate(devices):
        f0, f1 = shard.frame_block(n_frames - 1, k, D, unit)
        if f1 - f0 < 2:
            plans.append(None)
            continue
        if hbm_available is None:
            with executor.on_device(d):
                hbm = window.available_memory()
        else:
            hbm = hbm_available(d) if callable(hbm_available) else hbm_available
        plans.append(plan_lazy(frames, n_frames, dim_size, window_size, overlap, n_win, chunksize, memory_factor, engine, prefetch,
                               host_available=host, hbm_available=hbm / devices.count(d), first=f0, stop=f1, host_share=D))
    return plans


def _run_resident(frames, plans, sink, devices, time, signal_threshold):
    """The loops of pyorc/velocimetry/ffpiv.py:348-370 and :399-440 over a lazy stack: pieces are loaded ahead (``ChunkPrefetcher``),
    pushed into an HBM-resident stack (``ResidentStack``) and launched on the anchors.  ``plans``: one :class:`LazyPlan` per device
    worker (:func:`plan_lazy_devices`); every worker runs its own windows on its own device."""
    from . import plugin

    launch = sink[0]
    dim_size = tuple(int(v) for v in frames[0].shape)
    first = next(pl for pl in plans if pl is not None)
    handoff, chain = first["handoff"], first["chain"]
    lazy = _lazy_source(frames, handoff)
    mean, mean_host = None, None
    mean_s = 0.0
    if chain is not None and chain.samples:
        # normalize's mean plane, from the sampled camera frames only (frames.py:296-299), loaded once for the run and computed on the
        # first device; the other devices get a copy of the same plane (the same bits in every device's filters)
        import time as _time

        t0 = _time.perf_counter()
        iv = round(len(lazy) / chain.samples)
        if iv == 0:
            raise AssertionError(f"Amount of frames is too small to provide {chain.samples} samples")
        with executor.on_device(None if devices is None else devices[0]):
            mean = chain.mean_plane(np.ascontiguousarray(_values(load_frame_chunk(lazy[::iv]))))
            if devices is not None and any(d != devices[0] for d in devices):
                mean_host = mean.to_host()
        mean_s = _time.perf_counter() - t0
    per_device = [None] * len(plans)

    def run(k, stop):
        plan = plans[k]
        if plan is None:
            return
        device = None if devices is None else devices[k]
        mean_k = mean if (mean_host is None or device == devices[0]) else resident.DeviceFrames.from_host(mean_host)
        projection = None if handoff is None else plugin.projection_for(handoff) if devices is None else plugin.projection_for(handoff, device)

        def launch_k(view, p0, p1):
            executor.stop_point(stop)
            launch(k, view, p0, p1)

        stats = per_device[k] = {
            "plan": {key: plan[key] for key in ("windows", "load_frames", "align", "depth", "max_depth", "source", "peak_host_bytes", "host_budget")},
            "load_s": 0.0, "waited_s": 0.0, "upload_s": 0.0, "launch_s": 0.0, "chunks": 0, "depth_per_chunk": [], "load_s_per_chunk": [],
            "waited_s_per_chunk": []}
        if plan["chain"] is not None:
            stats["plan"]["chain"] = plan["chain"].names
            stats["mean_s"] = mean_s if k == 0 else 0.0      # sampled frames loaded, uploaded, mean plane computed (once)
        for (w0, w1), loads in zip(plan["windows"], plan["loads"]):
            executor.stop_point(stop)
            stack = resident.ResidentStack(w0, w1 - w0, dim_size, frames.dtype, plan["align"], launch_k, signal_threshold, projection,
                                           plan["chain"], mean_k)
            pieces = [(f0, lazy[f0:f1]) for f0, f1 in loads]

            def load_and_stage(piece, stack=stack):
                # on a loader thread: materialise the piece AND bring it to the device (upload -- or upload + projection -- into its place:
                # PCIe and the host's page handling stay off the thread that launches; the loaded array is released here as well)
                executor.stop_point(stop)
                f0, da = piece
                return stack.stage(f0, _values(load_frame_chunk(da)))

            with executor.ChunkPrefetcher(pieces, load_and_stage, depth=plan["depth"], max_depth_=plan["max_depth"]) as loader:
                try:
                    for n, n_staged in loader:
                        pieces[n] = None
                        stack.commit(loads[n][0], n_staged)
                finally:
                    loader.close()
                    st = loader.stats     # this window's loads: added up; depth / workers / adaptive: the last window's
                    for key in ("load_s", "waited_s", "chunks", "depth_per_chunk", "load_s_per_chunk", "waited_s_per_chunk"):
                        stats[key] += st[key]
                    stats.update(depth=st["depth"], workers=st["workers"], adaptive=st["adaptive"])
            stack.finish()
            stats["upload_s"] += stack.upload_s; stats["launch_s"] += stack.launch_s
            del stack
        for key, v in list(stats.items()):
            if isinstance(v, float):
                stats[key] = round(v, 6)

    return _run_workers(sink, devices, run, per_device, time, frames)
