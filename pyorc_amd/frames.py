"""Mirror of ``Frames.get_piv`` / ``Frames.get_piv_coords`` (pyorc/api/frames.py:47-197) for ``engine="hip"``.

Two ways in:

* ``get_piv(frames, ...)`` -- a function with the accessor's parameters.  ``frames`` is either an
  ``xr.DataArray`` produced by pyorc (then camera configuration, resolution, coordinates and
  attributes are taken from it exactly like the reference does, and an ``xr.Dataset`` comes back), or
  a plain ``(T, H, W)`` array -- or a ``pyorc_amd.device.DeviceFrames`` stack that already lives in HBM, e.g. the
  output of ``filters.normalize`` -> ``Projection.project_frames`` on device stacks: the recipe then never bounces
  through host float64 -- plus ``time`` / ``resolution`` keywords (then a ``PivResult`` dict comes back; this is what
  the tests and the benchmark use, since neither xarray nor pyorc exist on the GPU box).
* the two-line patch of INTEGRATION.md, which makes ``frames.frames.get_piv(engine="hip")`` of an
  unmodified pyorc call :func:`pyorc_amd.velocimetry.get_ffpiv`.

Parameter resolution follows the reference line by line: window -> (wy, wx) rounded to even
(:167), search area = window (:168), default overlap from the UN-rounded size (:171, quirk Q6),
engine check raising the same ValueError (:176-177).
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import velocimetry, window

ENGINES = ["hip"]


def resolve_window(window_size, overlap=None, search_area_size=None) -> Tuple[Tuple[int, int], Tuple[int, int], Tuple[int, int]]:
    """(window_size, search_area_size, overlap) as pyorc/api/frames.py:159-171 derives them.  ``search_area_size``: None = the window
    size (the reference's only choice), else an int or a pair, rounded to even like the window; a default ``overlap`` is then half the
    SEARCH AREA, which is what the grid is laid out by."""
    if window_size is None:
        raise ValueError("window_size is required when frames carry no camera configuration")
    ws = 2 * (window_size,) if isinstance(window_size, (int, np.integer)) else tuple(window_size)
    ws_even = window.round_to_even(ws)
    if search_area_size is not None:
        sa = 2 * (search_area_size,) if isinstance(search_area_size, (int, np.integer)) else tuple(search_area_size)
        sa_even = window.round_to_even(sa)
        if overlap is None:
            overlap = tuple(int(round(s) / 2) for s in sa_even)
        return ws_even, sa_even, tuple(int(o) for o in overlap)
    if overlap is None:
        if isinstance(window_size, (int, np.integer)):
            overlap = 2 * (int(round(window_size) / 2),)
        else:
            overlap = tuple(int(round(w) / 2) for w in window_size)
    return ws_even, ws_even, tuple(int(o) for o in overlap)


def get_piv_coords(dim_size, window_size, search_area_size, overlap, x=None, y=None):
    """Result axes: ``x[cols]``, ``y[rows]`` at the window centres (pyorc/api/frames.py:85-92, helpers.py:166-167)."""
    cols, rows = window.get_rect_coordinates(dim_size=dim_size, window_size=window_size,
                                             search_area_size=search_area_size, overlap=overlap)
    x = np.arange(dim_size[1]) if x is None else np.asarray(x)
    y = np.arange(dim_size[0]) if y is None else np.asarray(y)
    return {"y": y[rows], "x": x[cols]}, {"cols": cols, "rows": rows}


def get_piv(frames, window_size=None, overlap=None, engine: str = "hip", ensemble_corr: bool = False,
            time=None, resolution: Optional[float] = None, search_area_size=None, coarse_passes=None, **kwargs):
    """PIV on projected frames with the MI355X engine; parameters of ``Frames.get_piv`` (frames.py:114-121).

    Extra keywords for plain arrays: ``time`` (T,) seconds (default ``arange(T)``), ``resolution`` metres per
    pixel (default 1.0 => velocities in px/s).  ``**kwargs`` are forwarded to ``get_ffpiv`` (``chunksize``,
    ``memory_factor``, ``corr_min``, ``s2n_min``, ``count_min``, ``signal_threshold``).  ``search_area_size``: None (the window size,
    as in the reference) or a larger square search area of 16, 32 or 64 px ("Extended search area").
    ``ensemble_window`` / ``ensemble_stride`` (in ``**kwargs``, with ``ensemble_corr=True``): a sliding ensemble, INTEGRATION.md 2c.
    ``coarse_passes``: multi-pass PIV -- coarse passes run before ``window_size``, coarsest first, each an int n
    (n x n at overlap n / 2) or a pair ``(n, overlap)``; the result stays on the grid of ``window_size`` / ``overlap``.
    ``deform_passes`` (in ``**kwargs``): 0 .. 4 window deformation passes after the chain, per-timestep mode only.
    ``spectral_filter`` (in ``**kwargs``): ``"spof"`` -- SPOF phase-filtered correlation, windows of 16, 32 or 64 px.
    ``image_mask`` / ``mask_coverage_min`` (in ``**kwargs``): an ``(H, W)`` mask of the valid pixels, non-zero = valid, and the smallest
    share of valid samples a window is evaluated at (default 0.25) -- every window is correlated over its valid samples only
    (INTEGRATION.md 2h), windows of 16, 32 or 64 px, per-timestep mode.
    ``peak_ratio`` / ``peak_exclusion`` (in ``**kwargs``): ``peak_ratio=True`` adds ``peak_ratio``, ``corr2``, ``v_x2``, ``v_y2`` to the
    result -- the ratio of the two highest correlation peaks, the second one's height and the runner-up vector;
    ``peak_exclusion`` (default 2) is the half side of the box around the primary peak that holds no second peak.  Windows of 16, 32 or
    64 px, per-timestep mode.
    ``validate`` (in ``**kwargs``): True or a dict of ``validate.median_test``'s keywords -- the normalised median test on the
    displacement in pixels, on the device, before the scaling; the result gains the uint8 variable ``flag`` and, with
    ``peak_ratio=True``, rejected vectors are replaced by their runner-up where that one passes.  Per-timestep mode, no chain of passes.
    ``pair_step`` / ``pair_step_max`` / ``pair_step_target`` (in ``**kwargs``): multi-frame PIV for slow flow -- a lag
    of k frames for every window, a lag per window ``(rows, cols)``, or ``"adaptive"`` (a lag-1 pass picks each window's lag, at most
    ``pair_step_max``, so that it moves about ``pair_step_target`` px); velocities stay per frame interval and the result gains the
    uint8 variable ``pair_step``.  Windows of 16, 32 or 64 px, per-timestep mode, materialised stacks on one device.
    """
    if engine not in ENGINES:
        raise ValueError(f"Selected PIV engine {engine} does not exist.")
    is_xr = velocimetry._is_xr(frames)
    camera_config = None
    if is_xr and hasattr(frames, "frames") and hasattr(frames.frames, "camera_config"):
        import copy

        camera_config = copy.deepcopy(frames.frames.camera_config)
        if window_size is not None:
            camera_config.window_size = window_size
        window_size = camera_config.window_size
        resolution = camera_config.resolution if resolution is None else resolution
    ws, sa, ov = resolve_window(window_size, overlap, search_area_size)
    if is_xr:
        t = frames["time"]
        dt = t.diff(dim="time")
        xs, ys = frames["x"].values, frames["y"].values
    else:
        # DeviceFrames: HBM-resident stack, used as it is; a lazy stack (anything with ``load()``: time slices materialise on demand,
        # like the dask-backed DataArray of the xarray branch) is left lazy -- get_ffpiv loads it chunk by chunk, ahead of the launches
        if not velocimetry.is_device(frames) and not hasattr(frames, "load"):
            frames = np.asarray(frames)
        t = np.arange(frames.shape[0], dtype=np.float64) if time is None else np.asarray(time, dtype=np.float64)
        dt = np.diff(t)
        xs = ys = None
    res = 1.0 if resolution is None else float(resolution)
    coords, _ = get_piv_coords(tuple(frames[0].shape), ws, sa, ov, xs, ys)
    ds = velocimetry.get_ffpiv(frames, coords["y"], coords["x"], dt, engine=engine, ensemble_corr=ensemble_corr,
                               search_area_size=sa, window_size=ws, overlap=ov, res_x=res, res_y=res,
                               **({"coarse_passes": coarse_passes} if coarse_passes is not None and len(coarse_passes) else {}),
                               **({} if is_xr else {"time": t}), **kwargs)
    if is_xr and camera_config is not None:
        # the tail of the reference accessor (frames.py:190-196): 2-D coordinates, attributes, encoding
        from pyorc import const  # only reachable inside a pyorc installation

        _, mesh_coords = frames.frames.get_piv_coords(ws, sa, ov)
        ds = ds.velocimetry.add_xy_coords(mesh_coords, coords, {**const.PERSPECTIVE_ATTRS, **const.GEOGRAPHICAL_ATTRS})
        ds.attrs = frames.attrs
        ds.attrs.update(camera_config=camera_config.to_json())
        ds.velocimetry.set_encoding()
    return ds


def encode_int16(a: np.ndarray, scale: float = 0.01, fill: int = -9999) -> np.ndarray:
    """netCDF packing of the result variables (pyorc/const.py:80): int16, scale 0.01, fill -9999 -- on the GPU
    (``lspiv_pack_int16``; no host implementation: without a device this raises like every other entry point)."""
    from .project import pack_int16

    return pack_int16(a, scale, fill)
