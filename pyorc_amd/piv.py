"""Mirror of the ``ffpiv`` API that pyorc's PIV wrapper binds, executed on the MI355X.

``cross_corr`` and ``u_v_displacement`` keep the signatures observed at the reference call
sites (pyorc/velocimetry/ffpiv.py:222-231, 324, 450-459, 471) so they can be swapped in for
``from ffpiv import cross_corr, u_v_displacement`` (ffpiv.py:9).  ``piv_pairs`` is the fused
entry the ``hip`` engine actually uses: one kernel produces u, v, corr_max and s2n per
window without ever writing the (T-1, n_win, wy, wx) correlation volume to memory.

No CPU fallback: every function needs liblspiv_hip.so and a gfx950 device.
"""

from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

from . import _lib, device, window
from .device import is_device

ENGINES = ("hip",)


def _sig(signal_threshold: Optional[float]) -> float:
    return -1.0 if signal_threshold is None else float(signal_threshold)


def _check_args(window_size, overlap, search_area_size, normalize, engine):
    if engine not in ENGINES:
        raise ValueError(f"Selected PIV engine {engine} does not exist.")
    if normalize:
        raise NotImplementedError("stack-level `normalize` is never used by pyorc (ffpiv.py:227,455)")
    return window.search_spec(window_size, search_area_size)   # ValueError for an unsupported combination


def _to_velocity(disp: np.ndarray, res, dt: np.ndarray, out: np.ndarray) -> None:
    """``(disp * res / dt).astype(float32)`` of ffpiv.py:418-419 with the same arithmetic (the product in whatever type numpy
    gives it, the division in float64, one rounding to float32) but without the two float64 temporaries of the one-liner, into
    ``out`` (``disp`` itself, or a time slice of a run's result array).  What every mode without a fused scaling entry point does."""
    np.divide(disp * res, dt, out=out, dtype=np.float64, casting="same_kind")


def _check_scale(scale, return_planes, P):
    """``scale = (res_x, res_y, dt)`` checked: ``dt`` as ``(P,)`` float64; None without a scale."""
    if scale is None:
        return None
    if return_planes:
        raise ValueError("scale and return_planes exclude each other")
    dt = np.ascontiguousarray(scale[2], dtype=np.float64).reshape(-1)
    if dt.shape != (P,):
        raise ValueError(f"scale: dt must have one entry per frame pair ({P}), got shape {dt.shape}")
    return dt


def _check_out(out, shape):
    out = list(out)
    if len(out) != 4 or any(not isinstance(o, np.ndarray) or o.dtype != np.float32 or o.shape != shape or
                            not o.flags.c_contiguous or not o.flags.writeable for o in out):
        raise ValueError(f"out must be four writable C-contiguous float32 arrays of shape {shape}")
    return out


def _results_to_host(d_out, P, n_rows, n_cols, out=None):
    """The [u | v | corr | s2n] block of a launch, four consecutive (P, n_win) blocks in HBM, as four host arrays: straight into the
    caller's ``out`` arrays, or new ones."""
    lib = _lib.load()
    n_win = n_rows * n_cols
    if out is not None:
        for k in range(4):
            _lib.check(lib.lspiv_memcpy_d2h(_lib.ptr(out[k]), C.c_void_p(d_out.ptr + k * P * n_win * 4), out[k].nbytes))
        return tuple(out)
    res = d_out.to_host().reshape(4, P, n_rows, n_cols)     # lspiv_memcpy_d2h runs on, and waits for, the library's stream
    return tuple(np.ascontiguousarray(res[k]) for k in range(4))


def _device_stack(imgs, signal_threshold):
    """``imgs`` as a stack in HBM: a ``DeviceFrames`` as it is, a host stack the way the PIV host entry points bring it in (float64
    narrowed to float32 while it is staged)."""
    from .device import DeviceFrames

    if is_device(imgs):
        return imgs
    a = _lib.as_frames(imgs)
    d = DeviceFrames.empty(a.shape, DeviceFrames.device_dtype(a.dtype))
    d.upload(0, a, signal_threshold)
    return d


def _per_window_input(name, value, grid, dtype):
    """``shift`` / ``nodes`` of a pass: ``(P, n_rows, n_cols, 2)`` of ``dtype``, checked against ``grid`` and brought into HBM."""
    arr = np.ascontiguousarray(value, dtype=dtype)
    if arr.shape != (*grid, 2):
        raise ValueError(f"{name} must have shape {(*grid, 2)}, got {arr.shape}")
    return device.buffer(arr)


def _run_pairs(imgs, ws, ov, signal_threshold, return_planes, pair_offset, out, scale, entry, args, fused=False, extra=None, aux=None,
               validate=None, aux2=None, pairs=None):
    """The body every per-pair entry point shares: stack -> grid -> ``out`` and ``scale`` checked -> results (and planes) allocated on the
    stack's side, host or HBM -> ONE library call -> results on the host -> scaling.  A mode supplies only what differs:

    ``entry``: the names of its host-pointer and its device-pointer entry point (a ``DeviceFrames`` takes the second; None: no such side);
    ``args(c)``: the call's arguments from ``c.frames`` (pointer, dtype code, T, H, W), ``c.at`` (signal threshold, pair offset), ``c.res``
    (four host pointers, or the one of the [u | v | corr | s2n] block in HBM), ``c.planes``, ``c.extra``, ``c.aux`` -- pointers on the
    stack's side, None where there is nothing -- and ``c.dt`` (host); the device side's trailing stream is added here;
    ``fused``: ``scale`` is applied by the call itself (host) or by ``lspiv_scale_velocity_dev`` on the block in HBM (device: the same kernel
    as the host entry point's) -- else by numpy's own arithmetic on the host (:func:`_to_velocity`);
    ``extra(grid)``: the mode's extra input (mask, shift, nodes) for ``grid = (P, n_rows, n_cols)`` on the stack's side, an ndarray or a
    ``DeviceFrames``, or None;
    ``aux``: the dtype of a per-window output ``(P, n_rows, n_cols, 2)`` the call fills besides the results (the chain's offsets), or
    ``(dtype, width)`` for another trailing width (the second peak's four floats); ``aux2``: a second such output (``c.aux2``; the lagged
    pass hands out its lags and its clamped offsets), returned right after ``aux``;
    ``pairs``: the call computes the first ``pairs`` pairs of the stack only (``c.pairs``; the frames behind them are a lagged pass's halo);
    ``validate``: a ``validate.ValidateSpec`` -- the median test on the displacement in pixels, between the
    library call and the scaling: ``lspiv_validate_dev`` on the block in HBM, ``lspiv_validate`` on the host arrays; with ``aux`` (only the
    second-peak mode passes both) the runner-up is offered for substitution.  A mode whose host entry point scales by itself must not be
    given one together with ``fused``.

    Returns ``(u, v, corr_max, s2n[, planes][, aux][, aux2][, flag])``."""
    from .device import DeviceFrames

    lib = _lib.load()
    _lib.require_device()
    a = imgs if is_device(imgs) else _lib.as_frames(imgs)
    T, H, W = a.shape
    n_rows, n_cols = window.get_array_shape((H, W), ws, ov)
    if T < 2 or n_rows < 1 or n_cols < 1:
        raise ValueError(f"need >= 2 frames at least one window large, got {a.shape} for window {ws}")
    P, n_win = T - 1 if pairs is None else int(pairs), n_rows * n_cols
    if not 1 <= P <= T - 1:
        raise ValueError(f"pairs must lie in 1 .. {T - 1} for a stack of {T} frames, got {pairs!r}")
    if out is not None:
        out = _check_out(out, (P, n_rows, n_cols))
    dt = _check_scale(scale, return_planes, P)
    dev = is_device(a)
    x = extra((P, n_rows, n_cols)) if extra is not None else None
    if aux is not None:
        aux_dtype, aux_width = aux if isinstance(aux, tuple) else (aux, 2)
        aux = np.empty((P, n_rows, n_cols, aux_width), dtype=aux_dtype)
    if aux2 is not None:
        aux2 = np.empty((P, n_rows, n_cols, aux2[1]), dtype=aux2[0])
    if dev:   # HBM-resident stack: no staging, one call, only the result block crosses PCIe
        res = DeviceFrames.empty((4, P, n_win), np.float32)
        planes = DeviceFrames.empty((P * n_win, ws[0], ws[1]), np.float32) if return_planes else None
        d_aux = device.buffer(nbytes=aux.nbytes) if aux is not None else None
        d_aux2 = device.buffer(nbytes=aux2.nbytes) if aux2 is not None else None
        frames, res_ptrs, ptr = (a.c_ptr, a.dtype_code), (res.c_ptr,), lambda q: None if q is None else q.c_ptr
    else:
        res = out if out is not None else [np.empty((P, n_rows, n_cols), dtype=np.float32) for _ in range(4)]
        planes = np.empty((P, n_win, ws[0], ws[1]), dtype=np.float32) if return_planes else None
        d_aux, d_aux2 = aux, aux2
        frames, res_ptrs, ptr = (_lib.ptr(a), _lib.DTYPE_CODES[a.dtype]), tuple(_lib.ptr(r) for r in res), lambda q: None if q is None else _lib.ptr(q)
    c = SimpleNamespace(frames=(*frames, T, H, W), pairs=P, at=(_sig(signal_threshold), int(pair_offset)), res=res_ptrs, planes=ptr(planes),
                        extra=ptr(x), aux=ptr(d_aux), aux2=ptr(d_aux2), dt=None if dt is None else _lib.ptr(dt))
    _lib.check(getattr(lib, entry[dev])(*args(c), *((None,) if dev else ())))
    flag = None
    if validate is not None:
        from . import validate as validate_mod

        flag = np.empty((P, n_rows, n_cols), dtype=np.uint8)
        if dev:      # on the result block while it is still in HBM
            d_flag = device.buffer(nbytes=flag.nbytes)
            validate_mod.run_dev(validate, res.c_ptr, C.c_void_p(res.ptr + P * n_win * 4), c.aux, (P, n_rows, n_cols), d_flag.c_ptr)
            device.download_into(d_flag, flag)
        else:        # the host twin, right after the call
            validate_mod.run_host(validate, res[0], res[1], aux, flag)
    if dev:
        if dt is not None and fused:  # px / frame -> m / s in place on the [u | v] blocks
            _lib.check(lib.lspiv_scale_velocity_dev(res.c_ptr, P, n_win, float(scale[0]), float(scale[1]), c.dt, None))
        res = _results_to_host(res, P, n_rows, n_cols, out)
        if return_planes:
            planes = planes.to_host().reshape(P, n_win, ws[0], ws[1])
        if aux is not None:
            device.download_into(d_aux, aux)
        if aux2 is not None:
            device.download_into(d_aux2, aux2)
    if dt is not None and not fused:
        for k in range(2):
            _to_velocity(res[k], scale[k], dt[:, None, None], out=res[k])
    return (*res, *((planes,) if return_planes else ()), *((aux,) if aux is not None else ()), *((aux2,) if aux2 is not None else ()),
            *((flag,) if flag is not None else ()))


# the window specs that carry a mode of their own through ``piv_pairs``: spec class -> (the keyword the messages name, that mode's call)
_SPEC_MODES = {
    window.MultiPassWindow: ("coarse_passes", lambda imgs, spec, overlap, *a, **kw: piv_multipass(imgs, spec, *a, **kw)),
    window.FilteredWindow: ("spectral_filter", lambda imgs, spec, overlap, *a, **kw: piv_pairs_filtered(imgs, spec, overlap, spec.spectral_filter, *a, **kw)),
    window.MaskedWindow: ("image_mask", lambda imgs, spec, overlap, *a, **kw: piv_pairs_masked(imgs, spec, overlap, None, spec.mask_coverage_min, *a, **kw)),
    window.PeakRatioWindow: ("peak_ratio", lambda imgs, spec, overlap, *a, **kw: piv_pairs_peak2(imgs, spec, overlap, spec.peak_exclusion, *a, **kw)),
}
# ... and the specs whose ``scale`` is numpy's arithmetic on the host for a host stack: no fused scaling entry point
_HOST_SCALED = (window.SearchWindow, *_SPEC_MODES)


def piv_pairs(imgs, window_size=(32, 32), overlap=(16, 16), signal_threshold: Optional[float] = None,
              return_planes: bool = False, pair_offset: int = 0, out=None, scale=None, search_area_size=None, validate=None):
    """Fused PIV of every consecutive frame pair of ``imgs`` (T, H, W).

    Returns ``(u, v, corr_max, s2n[, planes])``: float32 arrays (T-1, n_rows, n_cols); u, v in
    pixels (u = column shift, v = row shift).  Replaces pyorc/velocimetry/ffpiv.py:446-474.
    ``pair_offset``: index of the chunk's first pair in the whole stack (``lspiv_piv_pairs_at``); chunks that start on
    multiples of ``window.chunk_alignment`` reproduce the whole-stack result bit for bit.
    ``out``: four C-contiguous float32 arrays (T-1, n_rows, n_cols) that receive u, v, corr_max, s2n (e.g. time slices of the
    arrays of a whole run: the caller's chunk loop then needs no concatenation); they are what is returned.
    ``scale = (res_x, res_y, dt)``: u, v come back in metres per second, ``(u * res_x / dt[:, None, None]).astype(float32)`` (ffpiv.py:
    418-419) computed on the device before the results cross PCIe -- float32 product, float64 division, one rounding: numpy's own
    arithmetic for PYTHON-FLOAT resolutions (the caller checks that, :func:`device_scaling_is_numpys`); ``dt``: (T-1,) float64 seconds.
    ``search_area_size``: None / the window size (today's path), or a larger square search area of 16, 32 or 64 px in which the even
    square window of frame t is searched in frame t+1 ("Extended search area"): the grid, ``overlap`` and the planes
    (``say x sax`` each) are then those of the search area.  ``window_size`` may also be a ``window.SearchWindow``.
    ``validate``: None (today's path bit for bit), True, a dict of ``validate.median_test``'s keywords or a ``validate.ValidateSpec`` --
    the median test on u, v in pixels, before any ``scale``; the returned tuple then ends with ``flag``,
    uint8 (T-1, n_rows, n_cols).  Not with a chain of passes (NotImplementedError).
    """
    if validate is not None:
        from .validate import validate_spec

        validate = validate_spec(validate)      # ValueError for a value outside its range
    mode = _SPEC_MODES.get(type(window_size))
    if mode is not None:   # a chain of passes, a spectral filter, an image mask, the second peak (INTEGRATION.md sections 2d, 2g, 2h, 2i): the final grid is this call's
        if search_area_size is not None and tuple(int(q) for q in search_area_size) != tuple(window_size):
            raise NotImplementedError(f"{mode[0]} together with a search_area_size larger than the window is not implemented")
        if validate is not None and isinstance(window_size, window.MultiPassWindow):
            raise NotImplementedError("validate together with coarse_passes / deform_passes is not implemented: run validate.median_test "
                                      "on the result instead")
        return mode[1](imgs, window_size, overlap, signal_threshold, return_planes, pair_offset, out=out, scale=scale,
                       **({} if validate is None else {"validate": validate}))
    ws = window.search_spec(window_size, search_area_size)
    search, dev = isinstance(ws, window.SearchWindow), is_device(imgs)
    if search:
        entry = ("lspiv_piv_search_pairs_at", "lspiv_piv_search_pairs_dev_at")
        args = lambda c: (*c.frames, *ws, *ws.window, *overlap, *c.at, *c.res, c.planes)  # noqa: E731
    elif scale is not None and not dev and validate is None:      # (the fused host call scales before a validation could run)
        entry = ("lspiv_piv_velocity_at",)
        args = lambda c: (*c.frames, *ws, *overlap, *c.at, float(scale[0]), float(scale[1]), c.dt, *c.res)  # noqa: E731
    else:
        entry = ("lspiv_piv_pairs_at", "lspiv_piv_pairs_dev_at")
        args = lambda c: (*c.frames, *ws, *overlap, *c.at, *c.res, c.planes)  # noqa: E731
    return _run_pairs(imgs, ws, overlap, signal_threshold, return_planes, pair_offset, out, scale, entry, args,
                      fused=dev or (not search and validate is None), validate=validate)


def device_scaling_is_numpys(res_x, res_y) -> bool:
    """Is ``(u * res / dt).astype(float32)`` with THESE resolutions what the device computes (float32 product)?  numpy multiplies a
    float32 array by a Python float in float32; by a numpy float64 scalar in float64 (numpy >= 2) -- then the host keeps numpy's own
    arithmetic.  (``np.float64`` is a subclass of ``float``: the test is on the exact type.)"""
    return type(res_x) in (float, int, np.float32) and type(res_y) in (float, int, np.float32)


def piv_pairs_filtered(imgs, window_size=(32, 32), overlap=(16, 16), spectral_filter="spof", signal_threshold: Optional[float] = None,
                       return_planes: bool = False, pair_offset: int = 0, out=None, scale=None, validate=None):
    """SPOF phase-filtered PIV of every consecutive frame pair of ``imgs``: :func:`piv_pairs` with every bin R
    of the cross spectrum replaced by R / sqrt(|R|) before the inverse transform ("robust phase correlation"), for imagery whose static
    or slow background outweighs the tracers.  Returns ``(u, v, corr_max, s2n[, planes])`` like :func:`piv_pairs`; ``corr_max`` is the
    maximum of the filtered plane (lower than an NCC peak), ``s2n`` its ratio to the mean of the clipped plane.  ``window_size``: square,
    16, 32 or 64 px.  ``spectral_filter``: ``"spof"``; None / ``"none"`` is :func:`piv_pairs`.  Pair-local, one window per job: every
    chunking gives the same bits (``pair_offset`` is accepted for symmetry); no float64 rescue pass.  ``out`` / ``scale`` as in
    :func:`piv_pairs` (the scaling is numpy's own arithmetic on the host).  Host stacks and ``DeviceFrames``."""
    flt = window.spectral_filter_spec(spectral_filter)
    if isinstance(window_size, window.FilteredWindow):
        flt = flt or window_size.spectral_filter
    if validate is not None:
        from .validate import validate_spec

        validate = validate_spec(validate)
    if flt is None:
        return piv_pairs(imgs, tuple(window_size), overlap, signal_threshold, return_planes, pair_offset, out=out, scale=scale,
                         **({} if validate is None else {"validate": validate}))
    ws = window.spectral_filter_supported(window_size)          # ValueError naming the sizes
    ov = (int(overlap[0]), int(overlap[1]))
    return _run_pairs(imgs, ws, ov, signal_threshold, return_planes, pair_offset, out, scale,
                      ("lspiv_piv_spof_pairs_at", "lspiv_piv_spof_pairs_dev_at"), lambda c: (*c.frames, *ws, *ov, *c.at, *c.res, c.planes),
                      validate=validate)


def piv_pairs_masked(imgs, window_size=(32, 32), overlap=(16, 16), image_mask=None, mask_coverage_min: float = 0.25,
                     signal_threshold: Optional[float] = None, return_planes: bool = False, pair_offset: int = 0, out=None, scale=None,
                     validate=None):
    """PIV of every consecutive frame pair of ``imgs`` under an image mask: :func:`piv_pairs` with every
    window correlated over its VALID samples only -- mean, standard deviation, the signal score and the divisor of the plane are those of
    the ``k`` samples where ``image_mask`` (``(H, W)``, bool / integer / float, non-zero = valid, one mask for every frame) is set;
    excluded samples count as exactly zero and are never read into the arithmetic (NaN there is harmless).  A window with fewer than
    ``max(2, ceil(mask_coverage_min * n * n))`` valid samples is NaN throughout.  Returns ``(u, v, corr_max, s2n[, planes])`` like
    :func:`piv_pairs`.  ``window_size``: square, 16, 32 or 64 px, or a ``window.MaskedWindow`` (then ``image_mask`` stays None).
    ``image_mask=None`` without one is :func:`piv_pairs`.  Pair-local, one window per job: every chunking gives the same bits
    (``pair_offset`` is accepted for symmetry); the float64 rescue pass follows as on the other per-pair paths.  ``out`` / ``scale`` as in
    :func:`piv_pairs` (the scaling is numpy's own arithmetic on the host).  Host stacks and ``DeviceFrames``."""
    if validate is not None:
        from .validate import validate_spec

        validate = validate_spec(validate)
    if image_mask is None and not isinstance(window_size, window.MaskedWindow):
        window.coverage_spec(mask_coverage_min)
        return piv_pairs(imgs, tuple(window_size), overlap, signal_threshold, return_planes, pair_offset, out=out, scale=scale,
                         **({} if validate is None else {"validate": validate}))
    a = imgs if is_device(imgs) else _lib.as_frames(imgs)
    spec = window.masked_spec(window_size, image_mask, mask_coverage_min, a.shape[1:])   # ValueError: sizes, coverage, the mask's shape
    ws = (int(spec[0]), int(spec[1]))
    ov = (int(overlap[0]), int(overlap[1]))
    # (the mask in HBM: one upload per device for all chunks of the call that made `spec`)
    return _run_pairs(a, ws, ov, signal_threshold, return_planes, pair_offset, out, scale,
                      ("lspiv_piv_masked_pairs_at", "lspiv_piv_masked_pairs_dev_at"),
                      lambda c: (*c.frames, *ws, *ov, c.extra, spec.k_min, *c.at, *c.res, c.planes),
                      extra=lambda grid: spec.device_mask() if is_device(a) else spec.image_mask, validate=validate)


def piv_pairs_peak2(imgs, window_size=(32, 32), overlap=(16, 16), peak_exclusion: int = 2, signal_threshold: Optional[float] = None,
                    return_planes: bool = False, pair_offset: int = 0, out=None, scale=None, validate=None):
    """PIV of every consecutive frame pair of ``imgs`` with the SECOND correlation peak of every window.
    Returns ``(u, v, corr_max, s2n, peak2[, planes])``: the first four (and the planes) are the bits of :func:`piv_pairs_shifted` without
    offsets; ``peak2`` is float32 ``(T-1, n_rows, n_cols, 4)`` = ``(u2, v2, corr2, peak_ratio)`` -- the runner-up vector in pixels, the
    height of the second highest peak and ``corr_max / corr2``.  On the fft-shifted plane a sample is a candidate when it is at least
    1e-5, lies outside the box of half side ``peak_exclusion`` (1 .. n // 4) around the primary peak (clipped at the edge, no wrap) and
    is no smaller than any of its existing 4-neighbours; the second peak is the largest candidate, the first in row-major order.  No
    candidate: ``corr2 = 0``, ``peak_ratio = inf``, ``u2 = v2 = NaN``; a skipped window is NaN in all four.  ``(u2, v2)`` follow the
    primary's rule (log-Gaussian fit inside, "border_peak" on the border, "v_sign").  The float64 rescue pass corrects u, v and leaves
    ``peak2`` alone.  ``window_size``: square, 16, 32 or 64 px, or a ``window.PeakRatioWindow`` (which carries its own radius).
    Pair-local, one window per job: every chunking gives the same bits (``pair_offset`` is accepted for symmetry).  ``out`` / ``scale``
    as in :func:`piv_pairs` (the scaling is numpy's own arithmetic on the host, on u, v and on u2, v2).  Host stacks and ``DeviceFrames``.
    ``validate`` as in :func:`piv_pairs`: the median test on u, v with the runner-up ``(u2, v2)`` offered for substitution; ``peak2`` stays
    as it is and ``flag`` ends the returned tuple."""
    if validate is not None:
        from .validate import validate_spec

        validate = validate_spec(validate)
    if isinstance(window_size, window.PeakRatioWindow):
        spec = window_size
    else:
        spec = window.peak_ratio_spec(window_size, True, peak_exclusion)   # ValueError: sizes, radius; NotImplementedError: another mode's spec
    ws, r = (int(spec[0]), int(spec[1])), int(spec.peak_exclusion)
    ov = (int(overlap[0]), int(overlap[1]))
    ret = _run_pairs(imgs, ws, ov, signal_threshold, return_planes, pair_offset, out, scale,
                     ("lspiv_piv_peak2_pairs_at", "lspiv_piv_peak2_pairs_dev_at"),
                     lambda c: (*c.frames, *ws, *ov, *c.at, r, *c.res, c.aux, c.planes), aux=(np.float32, 4), validate=validate)
    tail = () if validate is None else (ret[-1],)      # the flags of the median test
    ret = ret if validate is None else ret[:-1]
    peak2 = ret[-1]
    if scale is not None:
        dt = np.ascontiguousarray(scale[2], dtype=np.float64).reshape(-1)[:, None, None]
        for k in range(2):
            _to_velocity(peak2[..., k], scale[k], dt, out=peak2[..., k])
    return (*ret[:4], peak2, *ret[4:-1], *tail)


def second_peak(planes, peak_exclusion: int = 2) -> np.ndarray:
    """The second correlation peak of planes that already exist (mirrors :func:`u_v_displacement`): ``planes``
    ``(P, n_win, wy, wx)`` (or ``(n_win, wy, wx)``) float32, fft-shifted -- :func:`cross_corr` output, ``return_planes``, an ensemble's mean
    planes -- -> float32 ``(P, n_win, 4)`` = ``(u2, v2, corr2, peak_ratio)`` by the rule and the fit of :func:`piv_pairs_peak2`, on the
    device.  Any plane shape of 4 .. 4096 px per side; ``peak_exclusion`` in 1 .. min(wy, wx) // 4.  A NaN plane is NaN in all four."""
    c = np.ascontiguousarray(planes, dtype=np.float32)
    if c.ndim == 3:
        c = c[None]
    if c.ndim != 4:
        raise ValueError(f"planes must have shape (P, n_win, wy, wx), got {c.shape}")
    P, n_win, wy, wx = c.shape
    if min(wy, wx) < 4 or max(wy, wx) > 4096:
        raise ValueError(f"planes of {wy} x {wx}: a side outside 4 .. 4096")
    r = window.exclusion_spec(peak_exclusion, min(wy, wx))
    lib = _lib.load()
    _lib.require_device()
    out = np.empty((P, n_win, 4), dtype=np.float32)
    _lib.check(lib.lspiv_second_peak(_lib.ptr(c), P, n_win, wy, wx, r, _lib.ptr(out)))
    return out


def piv_pairs_shifted(imgs, window_size=(32, 32), overlap=(16, 16), shift=None, signal_threshold: Optional[float] = None,
                      return_planes: bool = False, pair_offset: int = 0):
    """One SHIFTED pass: per window and pair the ``n x n`` window of frame t against the ``n x n`` window of frame t+1 at the integer
    offset ``shift[pair, row, col] = (dy, dx)`` (int16, ``(T-1, n_rows, n_cols, 2)``; None: zeros), clamped by the kernel so that the
    window stays inside the frame.  Returns ``(u, v, corr_max, s2n[, planes])`` like :func:`piv_pairs`; u, v include the clamped offset.
    ``n`` in 16, 32, 64.  Host stacks and ``DeviceFrames``."""
    lib = _lib.load()
    _lib.require_device()
    ws, ov = (int(window_size[0]), int(window_size[1])), (int(overlap[0]), int(overlap[1]))
    if not lib.lspiv_shift_supported(ws[0], ws[1]):
        raise ValueError(f"window_size {ws} is not supported by the shifted pass: the window must be square and one of {window.SHIFT_WINDOWS}")
    return _run_pairs(_device_stack(imgs, signal_threshold), ws, ov, signal_threshold, return_planes, pair_offset, None, None,
                      (None, "lspiv_piv_shift_pairs_dev_at"), lambda c: (*c.frames, *ws, *ov, *c.at, c.extra, *c.res, c.planes),
                      extra=lambda grid: None if shift is None else _per_window_input("shift", shift, grid, np.int16))


def piv_pairs_lagged(imgs, window_size=(32, 32), overlap=(16, 16), pair_step=2, pair_step_max: int = 4, pair_step_target=None,
                     signal_threshold: Optional[float] = None, return_planes: bool = False, pair_offset: int = 0, out=None, scale=None,
                     pairs=None, return_shift: bool = False):
    """Multi-frame PIV: per pair t and window the ``n x n`` window of frame t against the window of frame
    ``t + k`` at an integer offset, the displacement divided by ``k`` -- for flow of a fraction of a pixel per frame interval, whose
    relative error a lag of one frame leaves at tens of per cent.  ``pair_step``: a whole number ``k`` in 1 .. 16 (every window, zero
    offsets); an integer array ``(rows, cols)`` of lags 1 .. 16 (zero offsets); or ``"adaptive"``: pass 0 is :func:`piv_pairs` at lag 1 on
    the same grid, then an integer predictor picks per window the largest lag ``<= pair_step_max`` (1 .. 16) that keeps the median
    displacement of the 3 x 3 neighbourhood at or below ``pair_step_target`` px (default ``n / 4``; ``0 < target <= n / 2``) and the
    integer offset that goes with it.  Every lag is clipped to the frames left: ``k[t] <= T - 1 - t``.  Returns ``(u, v, corr_max, s2n,
    lag[, planes][, shift])``: u, v in px per frame interval, ``lag`` uint8 ``(P, rows, cols)`` the effective lags, ``shift`` int16 ``(P,
    rows, cols, 2)`` the clamped offsets ``(dy, dx)`` with ``return_shift``.  A whole number 1 is :func:`piv_pairs` bit for bit plus the
    all-ones ``lag``; an all-ones ARRAY runs the lag kernel and gives :func:`piv_pairs_shifted`'s bits without offsets.  ``n`` in 16, 32,
    64.  ``pairs``: compute only the first ``pairs`` pairs of ``imgs``; the frames behind them serve the lags (a chunk of a longer stack
    with its halo of ``min(largest lag, frames to the end of the stack)`` frames then gives the bits of the whole stack's call; the
    adaptive form's pass 0 needs chunks cut on ``window.chunk_alignment`` as :func:`piv_pairs` does).  ``out`` / ``scale`` as in
    :func:`piv_pairs` (numpy's arithmetic on the host).  Host stacks and ``DeviceFrames``."""
    a = imgs if is_device(imgs) else _lib.as_frames(imgs)
    ov = (int(overlap[0]), int(overlap[1]))
    ws0 = (int(window_size[0]), int(window_size[1]))
    grid = window.get_array_shape(a.shape[1:], ws0, ov)
    spec = window.lag_spec(pair_step, ws0, grid, pair_step_max, pair_step_target)   # ValueError: sizes, ranges, the array's shape
    if spec is None:   # a lag of one frame: today's path
        if pairs is None:
            ret = piv_pairs(a, ws0, ov, signal_threshold, return_planes, pair_offset, out=out, scale=scale)
        else:          # the plain entry points on the first pairs + 1 frames
            ret = _run_pairs(a, ws0, ov, signal_threshold, return_planes, pair_offset, out, scale, ("lspiv_piv_pairs_at", "lspiv_piv_pairs_dev_at"),
                             lambda c: (*c.frames[:2], c.pairs + 1, *c.frames[3:], *ws0, *ov, *c.at, *c.res, c.planes), fused=is_device(a),
                             pairs=pairs)
        lag = np.ones(ret[0].shape, dtype=np.uint8)
        return (*ret[:4], lag, *ret[4:], *((np.zeros((*lag.shape, 2), dtype=np.int16),) if return_shift else ()))
    ws = window.lag_supported(ws0)

    def lags(grid3):
        if spec.array is None:
            return None
        return device.buffer(spec.array) if is_device(a) else spec.array

    ret = _run_pairs(a, ws, ov, signal_threshold, return_planes, pair_offset, out, scale,
                     ("lspiv_piv_lag_pairs_at", "lspiv_piv_lag_pairs_dev_at"),
                     lambda c: (*c.frames[:3], c.pairs, *c.frames[3:], *ws, *ov, *c.at, spec.form, spec.k, spec.target128, c.extra, None, *c.res,
                                c.planes, c.aux, c.aux2),
                     extra=lags, aux=(np.uint8, 1), aux2=(np.int16, 2), pairs=pairs)
    lag, shift = ret[-2][..., 0], ret[-1]
    return (*ret[:4], np.ascontiguousarray(lag), *ret[4:-2], *((shift,) if return_shift else ()))


def predict_lag(u, v, dim_size, window_size, overlap, n_frames: int, pair_step_max: int = 4, pair_step_target=None):
    """The lag predictor of ``pair_step="adaptive"`` alone, on the device: ``(u, v)`` ``(P, rows, cols)`` of a
    lag-1 pass (kernel orientation: before any ``v_sign``) of a stack of ``n_frames`` frames -> ``(lag, shift)``, uint8 ``(P, rows,
    cols)`` and int16 ``(P, rows, cols, 2)`` = (dy, dx) clamped to the frame: rint(64 x), twice the 3 x 3 median, the largest lag that
    keeps it at or below the target, the offset at that lag -- exact integer arithmetic after the rint."""
    lib = _lib.load()
    _lib.require_device()
    ov = (int(overlap[0]), int(overlap[1]))
    ws = window.lag_supported(window_size)
    spec = window.lag_spec("adaptive", ws, None, pair_step_max, pair_step_target)
    H, W = int(dim_size[0]), int(dim_size[1])
    rows, cols = window.get_array_shape((H, W), ws, ov)
    uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, rows, cols)
    vv = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, rows, cols)
    if uu.shape != vv.shape:
        raise ValueError(f"u {uu.shape} and v {vv.shape} differ")
    P = uu.shape[0]
    if P > int(n_frames) - 1:
        raise ValueError(f"{P} pairs need at least {P + 1} frames, got n_frames = {n_frames}")
    lag = np.empty((P, rows, cols), dtype=np.uint8)
    shift = np.empty((P, rows, cols, 2), dtype=np.int16)
    _lib.check(lib.lspiv_lag_predict(_lib.ptr(uu), _lib.ptr(vv), P, int(n_frames), H, W, *ws, *ov, spec.k, spec.target128, _lib.ptr(lag),
                                     _lib.ptr(shift)))
    return lag, shift


def predict_shift(u, v, dim_size, coarse, fine):
    """The predictor between two passes on the device: ``(u, v)`` ``(P, rows_c, cols_c)`` of a pass on its grid ``coarse = (n, overlap)``
    (kernel orientation: before any ``v_sign``) -> int16 offsets ``(P, rows_f, cols_f, 2)`` = (dy, dx) on the grid ``fine``, clamped to
    the frame: rint, 3 x 3 median, bilinear interpolation between the window centres, all in exact integer arithmetic."""
    from .device import DeviceFrames

    lib = _lib.load()
    _lib.require_device()
    (nc, oc), (nf, of) = (int(coarse[0]), int(coarse[1])), (int(fine[0]), int(fine[1]))
    H, W = int(dim_size[0]), int(dim_size[1])
    rc, cc = window.get_array_shape((H, W), (nc, nc), (oc, oc))
    rf, cf = window.get_array_shape((H, W), (nf, nf), (of, of))
    uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, rc, cc)
    vv = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, rc, cc)
    if uu.shape != vv.shape:
        raise ValueError(f"u {uu.shape} and v {vv.shape} differ")
    P = uu.shape[0]
    d_uv = DeviceFrames.empty((2, P, rc * cc), np.float32)
    _lib.check(lib.lspiv_memcpy_h2d(d_uv.c_ptr, _lib.ptr(uu), uu.nbytes))
    _lib.check(lib.lspiv_memcpy_h2d(C.c_void_p(d_uv.ptr + uu.nbytes), _lib.ptr(vv), vv.nbytes))
    out = np.empty((P, rf, cf, 2), dtype=np.int16)
    d_shift = device.buffer(nbytes=out.nbytes)
    _lib.check(lib.lspiv_piv_predict_shift_dev(d_uv.c_ptr, C.c_void_p(d_uv.ptr + uu.nbytes), P, H, W, nc, nc, oc, oc, nf, nf, of, of,
                                               d_shift.c_ptr, None))
    return device.download_into(d_shift, out)


def predict_deform(u, v):
    """The node predictor of the window deformation passes on the device: ``(u, v)`` ``(P, rows, cols)`` of a
    pass (kernel orientation: before any ``v_sign``) -> int32 nodes ``(P, rows, cols, 2)`` = (v, u) in 1 / 128 px on the same grid:
    rint(64 x), then twice the 3 x 3 median over the valid neighbours."""
    from .device import DeviceFrames

    lib = _lib.load()
    _lib.require_device()
    uu = np.ascontiguousarray(u, dtype=np.float32)
    vv = np.ascontiguousarray(v, dtype=np.float32)
    if uu.ndim == 2:
        uu, vv = uu[None], vv[None]
    if uu.ndim != 3 or uu.shape != vv.shape or uu.shape[1] < 1 or uu.shape[2] < 1:
        raise ValueError(f"u and v must have one shape (P, rows, cols), got {uu.shape} and {vv.shape}")
    P, rows, cols = uu.shape
    out = np.empty((P, rows, cols, 2), dtype=np.int32)
    d_uv = DeviceFrames.empty((2, max(P, 1), rows * cols), np.float32)
    d_nodes = device.buffer(nbytes=out.nbytes)
    if out.size:
        _lib.check(lib.lspiv_memcpy_h2d(d_uv.c_ptr, _lib.ptr(uu), uu.nbytes))
        _lib.check(lib.lspiv_memcpy_h2d(C.c_void_p(d_uv.ptr + uu.nbytes), _lib.ptr(vv), vv.nbytes))
    _lib.check(lib.lspiv_piv_predict_deform_dev(d_uv.c_ptr, C.c_void_p(d_uv.ptr + uu.nbytes), P, rows, cols, d_nodes.c_ptr, None))
    return device.download_into(d_nodes, out)


def piv_pairs_deformed(imgs, window_size=(32, 32), overlap=(16, 16), nodes=None, signal_threshold: Optional[float] = None,
                       return_planes: bool = False, pair_offset: int = 0):
    """One window DEFORMATION pass: per pair, frame t+1 is warped by the dense field interpolated from
    ``nodes[pair, row, col] = (v, u)`` (int32, 1 / 128 px, ``(T-1, n_rows, n_cols, 2)``: the predicted displacement at every window
    centre, :func:`predict_deform`; None: zeros) at 1 / 64 px, bilinearly, the edge replicated; then every ``n x n`` window of frame t
    meets the window at the SAME position of the warped frame.  Returns ``(u, v, corr_max, s2n[, planes])`` like :func:`piv_pairs`;
    u, v include the window's own node.  ``n`` in 16, 32, 64, one overlap for both axes.  Host stacks and ``DeviceFrames``."""
    lib = _lib.load()
    _lib.require_device()
    ws, ov = (int(window_size[0]), int(window_size[1])), (int(overlap[0]), int(overlap[1]))
    if not lib.lspiv_deform_supported(ws[0], ws[1]) or ov[0] != ov[1]:
        raise ValueError(f"window_size {ws}, overlap {ov} is not supported by the deformation pass: the window must be square and one of "
                         f"{window.DEFORM_WINDOWS}, at one overlap for both axes")
    return _run_pairs(_device_stack(imgs, signal_threshold), ws, ov, signal_threshold, return_planes, pair_offset, None, None,
                      (None, "lspiv_piv_deform_pairs_dev_at"), lambda c: (*c.frames, *ws, *ov, *c.at, c.extra, *c.res, c.planes),
                      extra=lambda grid: _per_window_input("nodes", np.zeros((*grid, 2), np.int32) if nodes is None else nodes, grid, np.int32))


def piv_multipass(imgs, passes, signal_threshold: Optional[float] = None, return_planes: bool = False, pair_offset: int = 0,
                  return_shift: bool = False, return_passes: bool = False, out=None, scale=None, deform_passes=None):
    """Multi-pass PIV: ``passes`` = ``[(n_0, overlap_0), ..., (n_K, overlap_K)]`` coarsest first (or a ``window.MultiPassWindow``); pass
    0 is :func:`piv_pairs` of its window, each later pass (16, 32 or 64 px) cuts its window of frame t+1 at the integer offset the
    previous pass predicts and measures the residual.  Returns ``(u, v, corr_max, s2n[, planes][, shift][, per_pass])`` on the LAST
    pass's grid; ``shift`` int16 ``(T-1, n_rows, n_cols, 2)`` = the last pass's clamped offsets (dy, dx); ``per_pass`` a list with every
    pass's ``(u, v, corr_max, s2n, shift)`` in the kernels' orientation (shift None for pass 0) -- the chain is then composed call by
    call from :func:`piv_pairs`, :func:`predict_shift` and :func:`piv_pairs_shifted` IN ADDITION to the one call (a diagnostic: the work
    is done twice; the C ABI hands out no intermediates), which gives the bits of the one call.
    ``out`` / ``scale`` as in :func:`piv_pairs` (the scaling is numpy's own arithmetic on the host).
    ``deform_passes`` = D (0 .. 4; None or 0: today's path, bit for bit; a ``MultiPassWindow`` carries its own): D window deformation
    passes follow the chain on the final grid, each fed with the (u, v) of the pass before it; corr_max, s2n
    and planes are the last one's, ``shift`` stays the last CHAIN pass's.  ``per_pass`` then also lists every deformation pass's
    ``(u, v, corr_max, s2n, nodes)`` (nodes int32 ``(T-1, n_rows, n_cols, 2)`` = (v, u) in 1 / 128 px), composed from
    :func:`predict_deform` and :func:`piv_pairs_deformed`.  One pass roughly halves the median error of the final field on sheared
    flows; a second one neither helps nor hurts on the stacks tried."""
    spec = passes if isinstance(passes, window.MultiPassWindow) else None
    if spec is None:
        passes = [(int(n), int(o)) for n, o in passes]
        if not passes:
            raise ValueError("passes is empty")
        spec = window.multipass_spec((passes[-1][0],) * 2, (passes[-1][1],) * 2, passes[:-1], deform_passes)
        if not isinstance(spec, window.MultiPassWindow):
            spec = window.MultiPassWindow(passes)          # one pass: today's path through the chain's entry point
    elif window.deform_count(deform_passes) not in (0, spec.deform):
        raise ValueError("deform_passes given twice: passes is a MultiPassWindow already")
    passes = list(spec.passes)
    n_deform = spec.deform
    n, ov = passes[-1]
    arr = (C.c_int * (4 * len(passes)))(*[q for m, o in passes for q in (m, m, o, o)])
    d = _device_stack(imgs, signal_threshold) if return_passes else imgs      # (the diagnostic chain below runs on the stack in HBM)
    ret = list(_run_pairs(d, (n, n), (ov, ov), signal_threshold, return_planes, pair_offset, out, scale,
                          ("lspiv_piv_multipass_deform_at", "lspiv_piv_multipass_deform_dev_at"),
                          lambda c: (*c.frames, len(passes), arr, n_deform, *c.at, *c.res, c.planes, c.aux),
                          aux=np.int16 if (return_shift or return_passes) else None))
    if return_passes and not return_shift:      # (the one call of the diagnostic writes its offsets all the same)
        ret.pop()
    if return_passes:
        # the chain again, call by call on the stack in HBM, in the kernels' orientation (a v_sign of the per-call entry points is undone:
        # a negation is exact)
        flip = _lib.get_option("v_sign") == 1
        per, prev = [], None
        for k, (m, o) in enumerate(passes):
            if k == 0:
                u, v, cm, sn = piv_pairs(d, (m, m), (o, o), signal_threshold, pair_offset=pair_offset)
                sh = None
            else:
                sh = predict_shift(prev[0], prev[1], d.shape[1:], passes[k - 1], (m, o))
                u, v, cm, sn = piv_pairs_shifted(d, (m, m), (o, o), sh, signal_threshold, pair_offset=pair_offset)
            if flip:
                v = -v
            prev = (u, v)
            per.append((u, v, cm, sn, sh))
        for _ in range(n_deform):
            nodes = predict_deform(prev[0], prev[1])
            u, v, cm, sn = piv_pairs_deformed(d, (n, n), (ov, ov), nodes, signal_threshold, pair_offset=pair_offset)
            if flip:
                v = -v
            prev = (u, v)
            per.append((u, v, cm, sn, nodes))
        ret.append(per)
    return tuple(ret)


def cross_corr(imgs, window_size=(64, 64), overlap=(32, 32), search_area_size=None, normalize=False,
               engine="hip", signal_threshold=None, verbose=False):
    """``ffpiv.cross_corr`` drop-in: returns ``(x, y, corr)``, corr (T-1, n_win, wy, wx) float32 -- with a ``search_area_size`` larger
    than the window ("Extended search area") planes, grid and coordinates are those of the search area.

    Planes of window pairs below ``signal_threshold`` are NaN (pyorc/velocimetry/ffpiv.py:93-97).
    """
    spec = _check_args(window_size, overlap, search_area_size, normalize, engine)
    a = _lib.as_frames(imgs)
    x, y = window.get_rect_coordinates(a.shape[-2:], tuple(spec), overlap)
    *_, planes = piv_pairs(a, spec, overlap, signal_threshold, return_planes=True)
    return x, y, planes


def u_v_displacement(corr, n_rows: int, n_cols: int, engine: str = "hip") -> Tuple[np.ndarray, np.ndarray]:
    """``ffpiv.u_v_displacement`` drop-in: corr (P, n_win, wy, wx) -> u, v (P, n_rows, n_cols) in pixels."""
    if engine not in ENGINES:
        raise ValueError(f"Selected PIV engine {engine} does not exist.")
    lib = _lib.load()
    _lib.require_device()
    c = np.ascontiguousarray(corr, dtype=np.float32)
    if c.ndim == 3:
        c = c[None]
    P, n_win, wy, wx = c.shape
    if n_win != n_rows * n_cols:
        raise ValueError(f"corr has {n_win} windows, expected {n_rows}*{n_cols}")
    u = np.empty((P, n_rows, n_cols), dtype=np.float32)
    v = np.empty((P, n_rows, n_cols), dtype=np.float32)
    _lib.check(lib.lspiv_u_v_displacement(_lib.ptr(c), P, n_win, wy, wx, _lib.ptr(u), _lib.ptr(v)))
    return u, v


class Ensemble:
    """Device-resident ensemble-correlation accumulator (pyorc/velocimetry/ffpiv.py:182-376)."""

    def __init__(self, dim_size, window_size, overlap, sliding=None, shift=None, spectral_filter=None):
        """``sliding=(M, s)``: a sliding ensemble -- outputs over windows of M pairs that advance by s
        pairs, read with :meth:`finish_sliding`; every ``accumulate`` but the last must then hold a multiple of s pairs.
        ``shift``: int16 ``(n_rows, n_cols, 2)`` = (dy, dx) per window, or a ``DeviceFrames`` holding those bytes -- a SHIFTED ensemble pass
        (INTEGRATION.md section 2e): frame t+1's window of every pair is cut at that offset (clamped to the frame: :attr:`shift`), and
        ``finish`` returns the total displacement.  Windows of 16, 32 or 64 px; not together with ``sliding``.
        ``spectral_filter``: None / ``"none"`` (today's path) or ``"spof"`` (a ``window.FilteredWindow`` as
        ``window_size`` carries its own) -- the planes summed are the SPOF phase-filtered ones of :func:`piv_pairs_filtered`; ``corr_min`` /
        ``s2n_min`` keep their meaning, their useful values are lower.  Windows of 16, 32 or 64 px; every chunking gives the same bits;
        no float64 rescue of the final fit.  Not together with ``sliding`` or ``shift``."""
        if isinstance(window_size, window.MaskedWindow):
            raise NotImplementedError("image_mask together with ensemble_corr=True is not implemented: the ensemble kernels and their "
                                      "float64 rescue have no masked form")
        if isinstance(window_size, window.PeakRatioWindow):
            raise NotImplementedError("peak_ratio together with ensemble_corr=True is not implemented: the ensemble kernels have no "
                                      "second-peak form; use piv.second_peak on the mean planes of finish(return_mean=True) instead")
        flt = window.spectral_filter_spec(spectral_filter)
        if isinstance(window_size, window.FilteredWindow):
            flt = flt or window_size.spectral_filter
        if flt is not None:
            if sliding is not None:
                raise NotImplementedError("spectral_filter together with ensemble_window is not implemented: a sliding ensemble has no spectral filter")
            if shift is not None:
                raise NotImplementedError("spectral_filter together with coarse_passes is not implemented: a shifted ensemble pass has no spectral filter")
            window.spectral_filter_supported(window_size)      # ValueError naming the sizes
        if sliding is not None:
            sliding = window.sliding_spec(True, *sliding)
            if shift is not None:
                raise NotImplementedError("a sliding ensemble has no shifted pass: sliding= and shift= exclude each other")
        lib = _lib.load()
        _lib.require_device()
        self._h = C.c_void_p()
        self.window_size = tuple(window_size)
        self.overlap = tuple(overlap)
        self.dim_size = tuple(dim_size)
        self.n_rows, self.n_cols = window.get_array_shape(dim_size, window_size, overlap)
        _lib.check(lib.lspiv_ensemble_begin(dim_size[0], dim_size[1], window_size[0], window_size[1],
                                            overlap[0], overlap[1], C.byref(self._h)))
        d = C.c_int(0)
        _lib.check(lib.lspiv_get_device(C.byref(d)))
        self.device = int(d.value)   # the handle's sums live here; every call on it is made with this device current
        self._held = []   # DeviceFrames chunks the handle borrows until finish (float64 rescue of the final fit)
        self._retain_mode = None   # set_retain not called yet: accumulate() of a DeviceFrames chunk picks RETAIN_BORROW
        self.sliding = sliding
        self.pairs_done = 0        # pairs accumulated so far (a sliding handle's outputs are counted from it)
        if sliding is not None:
            _lib.check(lib.lspiv_ensemble_set_sliding(self._h, sliding[0], sliding[1]))
        self.shifted = shift is not None
        self.spectral_filter = flt
        try:
            if shift is not None:
                self._set_shift(shift)
            if flt is not None:
                _lib.check(lib.lspiv_ensemble_set_spectral_filter(self._h, window.SPECTRAL_FILTERS.index(flt)))
        except Exception:
            self.close()
            raise

    def _set_shift(self, shift):
        lib = _lib.load()
        n_bytes = self.n_rows * self.n_cols * 4
        if is_device(shift):
            if shift.nbytes != n_bytes:
                raise ValueError(f"shift on the device must hold {(self.n_rows, self.n_cols, 2)} int16 ({n_bytes} bytes), got {shift.nbytes}")
            _lib.check(lib.lspiv_ensemble_set_shift_dev(self._h, shift.c_ptr, None))
            return
        sh = np.ascontiguousarray(shift, dtype=np.int16)
        if sh.shape != (self.n_rows, self.n_cols, 2):
            raise ValueError(f"shift must have shape {(self.n_rows, self.n_cols, 2)}, got {sh.shape}")
        _lib.check(lib.lspiv_ensemble_set_shift(self._h, _lib.ptr(sh)))

    @property
    def shift(self):
        """The clamped offsets the handle uses, int16 ``(n_rows, n_cols, 2)`` = (dy, dx); None on a handle without offsets."""
        if not self.shifted:
            return None
        out = np.empty((self.n_rows, self.n_cols, 2), dtype=np.int16)
        _lib.check(_lib.load().lspiv_ensemble_get_shift(self._h, _lib.ptr(out)))
        return out

    RETAIN_NONE, RETAIN_COPY, RETAIN_BORROW = 0, 1, 2

    def set_retain(self, mode: int) -> None:
        """How ``accumulate_dev`` keeps the chunks for the float64 rescue of the final fit (include/lspiv.h,
        ``lspiv_ensemble_set_retain``): 0 nothing (float32 fits), 1 the handle copies them, 2 it borrows the caller's pointers."""
        _lib.check(_lib.load().lspiv_ensemble_set_retain(self._h, int(mode)))
        self._retain_mode = int(mode)
        # what was borrowed so far STAYS pinned by this object until close(): lspiv_ensemble_set_retain only stores the mode, the handle
        # keeps the earlier borrowed pointers (in COPY mode for good, in NONE mode until the next accumulate), and a finish without
        # another accumulate reads them -- dropping them here let the caller free HBM the final fit's float64 rescue still read

    def stats(self) -> dict:
        """Counters of the last ``finish``: windows flagged / re-evaluated in float64 / left with their float32 fit, chunks and
        bytes kept, and whether every chunk could be kept."""
        st = (C.c_int64 * 6)()
        _lib.check(_lib.load().lspiv_ensemble_stats(self._h, st))
        return {"flagged": int(st[0]), "rescued": int(st[1]), "float32_kept": int(st[2]), "chunks_kept": int(st[3]),
                "bytes_kept": int(st[4]), "retain_complete": bool(st[5])}

    def accumulate(self, imgs, corr_min: float, s2n_min: float, signal_threshold: Optional[float] = None, out=None):
        """Add one frame chunk; returns masked per-pair (corr_max, s2n), each (T-1, n_win) float32.  ``out``: two C-contiguous float32
        arrays of that shape to receive them (time slices of a whole run's arrays: no concatenation afterwards)."""
        a = imgs if is_device(imgs) else _lib.as_frames(imgs)
        if tuple(a.shape[1:]) != self.dim_size:
            raise ValueError(f"chunk shape {a.shape[1:]} != ensemble shape {self.dim_size}")
        P = a.shape[0] - 1
        n_win = self.n_rows * self.n_cols
        if out is not None:
            out = tuple(out)
            if len(out) != 2 or any(not isinstance(o, np.ndarray) or o.dtype != np.float32 or o.shape != (P, n_win) or
                                    not o.flags.c_contiguous or not o.flags.writeable for o in out):
                raise ValueError(f"out must be two writable C-contiguous float32 arrays of shape {(P, n_win)}")
        if is_device(a):
            from .device import DeviceFrames

            d = DeviceFrames.empty((2, P, n_win), np.float32)
            # an HBM-resident stack stays alive as long as this object holds it: unless the caller chose a mode (set_retain: it is respected),
            # the handle borrows the pointer (no copy) and the final fit can go back to the frames.  The borrowed bytes count
            # against the handle's budget (LSPIV_ENSEMBLE_RETAIN_BYTES, a quarter of the HBM by default): beyond it the handle
            # gives the rescue up (stats()["retain_complete"] False, float32 fits) and this object lets go of every chunk --
            # a caller streaming more chunks through one ensemble than the budget holds is not pinned into an out-of-memory
            if self._retain_mode is None:      # no choice made: borrow
                _lib.check(_lib.load().lspiv_ensemble_set_retain(self._h, self.RETAIN_BORROW))
                self._retain_mode = self.RETAIN_BORROW
            if self._retain_mode == self.RETAIN_BORROW:
                self._held.append(a)
            self.accumulate_dev(a.ptr, a.dtype, a.shape[0], corr_min, s2n_min, d.ptr, signal_threshold)
            if self._held and not self.stats()["retain_complete"]:
                self._held = []
            if out is not None:
                for k in range(2):
                    _lib.check(_lib.load().lspiv_memcpy_d2h(_lib.ptr(out[k]), C.c_void_p(d.ptr + k * P * n_win * 4), out[k].nbytes))
                return out
            res = d.to_host()
            return np.ascontiguousarray(res[0]), np.ascontiguousarray(res[1])
        cm, sn = out if out is not None else (np.empty((P, n_win), dtype=np.float32), np.empty((P, n_win), dtype=np.float32))
        _lib.check(_lib.load().lspiv_ensemble_accumulate(self._h, _lib.ptr(a), _lib.DTYPE_CODES[a.dtype], a.shape[0],
                                                         float(corr_min), float(s2n_min), _sig(signal_threshold),
                                                         _lib.ptr(cm), _lib.ptr(sn)))
        self.pairs_done += P
        return cm, sn

    def accumulate_dev(self, d_frames: int, dtype, n_frames: int, corr_min: float, s2n_min: float,
                       d_corr_s2n: int, signal_threshold: Optional[float] = None, stream: Optional[int] = None) -> None:
        """Same on a chunk that already sits in HBM; d_corr_s2n receives [corr_max | s2n], 2*(T-1)*n_win float32."""
        _lib.check(_lib.load().lspiv_ensemble_accumulate_dev(
            self._h, C.c_void_p(d_frames), _lib.DTYPE_CODES[np.dtype(dtype)], n_frames, float(corr_min), float(s2n_min),
            _sig(signal_threshold), C.c_void_p(d_corr_s2n), C.c_void_p(stream) if stream else None))
        self.pairs_done += int(n_frames) - 1

    def finish(self, count_min: float, n_frames: float, return_mean: bool = False):
        """Count filter + mean plane + sub-pixel peak: u, v (1, n_rows, n_cols) px, corr_count (n_win,)."""
        n_win = self.n_rows * self.n_cols
        u = np.empty((1, self.n_rows, self.n_cols), dtype=np.float32)
        v = np.empty((1, self.n_rows, self.n_cols), dtype=np.float32)
        cnt = np.empty(n_win, dtype=np.float32)
        mean = np.empty((1, n_win) + self.window_size, dtype=np.float32) if return_mean else None
        _lib.check(_lib.load().lspiv_ensemble_finish(self._h, float(count_min), float(n_frames), _lib.ptr(u),
                                                     _lib.ptr(v), _lib.ptr(cnt),
                                                     _lib.ptr(mean) if mean is not None else None))
        return (u, v, cnt, mean) if return_mean else (u, v, cnt)

    def reserve_sliding(self, n_pairs: int):
        """Room in the block store for a run of ``n_pairs`` pairs in all, allocated once (before the first ``accumulate``): the store
        then never grows, which would double it and copy the blocks written so far."""
        if self.sliding is None:
            raise ValueError("reserve_sliding needs an Ensemble made with sliding=(M, s)")
        _lib.check(_lib.load().lspiv_ensemble_sliding_reserve(self._h, int(n_pairs)))

    def finish_sliding(self, count_min: float, first: int = 0, n: Optional[int] = None, return_planes: bool = False):
        """Outputs ``first .. first + n - 1`` of a sliding ensemble (``n`` None: all from ``first``): u, v (n, n_rows, n_cols) px and
        count (n, n_rows, n_cols) -- NaN where fewer than ``count_min * M`` pairs of the window were kept --, and with
        ``return_planes`` the mean planes (n, n_win, wy, wx)."""
        if self.sliding is None:
            raise ValueError("finish_sliding needs an Ensemble made with sliding=(M, s)")
        M, s = self.sliding
        total = max(0, self.pairs_done // s - M // s + 1)
        first = int(first)
        n = total - first if n is None else int(n)
        if first < 0 or n < 1 or first + n > total:
            raise ValueError(f"outputs [{first}, {first + n}) asked for, the {self.pairs_done} pairs accumulated give {total}")
        n_win = self.n_rows * self.n_cols
        u, v, cnt = (np.empty((n, self.n_rows, self.n_cols), dtype=np.float32) for _ in range(3))
        mean = np.empty((n, n_win) + self.window_size, dtype=np.float32) if return_planes else None
        _lib.check(_lib.load().lspiv_ensemble_sliding_finish(self._h, float(count_min), first, n, _lib.ptr(u), _lib.ptr(v), _lib.ptr(cnt),
                                                             _lib.ptr(mean) if mean is not None else None))
        return (u, v, cnt, mean) if return_planes else (u, v, cnt)

    # ---- the finish in three stages, for a sum spread over several handles (include/lspiv.h; pyorc_amd.shard.sharded_ensemble) ----
    PARTIAL_DOUBLES = 20

    def flag(self, count_min: float, n_frames: float) -> int:
        """Mean planes + float32 fits + the windows whose fit needs float64: how many (the same on every rank holding the same state)."""
        n = C.c_int64(0)
        _lib.check(_lib.load().lspiv_ensemble_flag(self._h, float(count_min), float(n_frames), C.byref(n)))
        self._n_rec = int(n.value)
        return self._n_rec

    def flag_digest(self) -> int:
        """64-bit digest of the last ``flag``'s sorted records (window, candidates): equal on ranks that flagged the same list."""
        d = C.c_uint64(0)
        _lib.check(_lib.load().lspiv_ensemble_flag_digest(self._h, C.byref(d)))
        return int(d.value)

    def partials(self):
        """(partials (n_records, 20) float64 over THIS handle's retained chunks, complete: bool)."""
        part = np.zeros((getattr(self, "_n_rec", 0), self.PARTIAL_DOUBLES), dtype=np.float64)
        ok = C.c_int(0)
        _lib.check(_lib.load().lspiv_ensemble_partials(self._h, _lib.ptr(part) if part.size else None, C.byref(ok)))
        return part, bool(ok.value)

    def finish_partials(self, partials, return_mean: bool = False):
        """``finish`` with the flagged windows fitted from ``partials`` summed over all handles that share the state."""
        n_win = self.n_rows * self.n_cols
        part = np.ascontiguousarray(partials, dtype=np.float64)
        if part.shape != (getattr(self, "_n_rec", 0), self.PARTIAL_DOUBLES):
            raise ValueError(f"partials shape {part.shape} != ({getattr(self, '_n_rec', 0)}, {self.PARTIAL_DOUBLES})")
        u = np.empty((1, self.n_rows, self.n_cols), dtype=np.float32)
        v = np.empty((1, self.n_rows, self.n_cols), dtype=np.float32)
        cnt = np.empty(n_win, dtype=np.float32)
        mean = np.empty((1, n_win) + self.window_size, dtype=np.float32) if return_mean else None
        _lib.check(_lib.load().lspiv_ensemble_finish_partials(self._h, _lib.ptr(part) if part.size else None, _lib.ptr(u), _lib.ptr(v),
                                                              _lib.ptr(cnt), _lib.ptr(mean) if mean is not None else None))
        return (u, v, cnt, mean) if return_mean else (u, v, cnt)

    def export_state(self):
        """(corr_sum (n_win, wy, wx) float32 in fft-shifted layout, corr_count (n_win,) float32) from HBM.  The handle's
        ``spectral_filter`` is not part of the state: a state goes back into a handle made with the same filter (``import_state``
        leaves the handle's own as it is)."""
        n_win = self.n_rows * self.n_cols
        s = np.empty((n_win,) + self.window_size, dtype=np.float32)
        k = np.empty(n_win, dtype=np.float32)
        _lib.check(_lib.load().lspiv_ensemble_export(self._h, _lib.ptr(s), _lib.ptr(k)))
        return s, k

    def import_state(self, corr_sum, corr_count, add: bool = False):
        """Replace (or add to) the running state, e.g. with the all-reduced sums of every rank's time block."""
        s = np.ascontiguousarray(corr_sum, dtype=np.float32)
        k = np.ascontiguousarray(corr_count, dtype=np.float32)
        n_win = self.n_rows * self.n_cols
        if s.size != n_win * self.window_size[0] * self.window_size[1] or k.size != n_win:
            raise ValueError("state shape does not match this ensemble")
        _lib.check(_lib.load().lspiv_ensemble_import(self._h, _lib.ptr(s), _lib.ptr(k), int(bool(add))))

    def close(self):
        if self._h:
            _lib.load().lspiv_ensemble_destroy(self._h)
            self._h = C.c_void_p()
            self._held = []   # borrowed stacks are released with the handle, not before (finish may be called again)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ensemble_means(corr_max, s2n, corr_count, count_min: float, n_frames: float):
    """``corr`` / ``s2n`` of an ensemble as the reference forms them (ffpiv.py:280-286): the nanmean over the pairs of the masked per-pair
    values ``(P, n_win)``, the windows below the count filter set to NaN in ``corr_max`` first (in place).  Returns two ``(n_win,)`` arrays."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        corr_max[:, np.asarray(corr_count).reshape(-1) < count_min * n_frames] = np.nan
        return np.nanmean(corr_max, axis=0), np.nanmean(s2n, axis=0)


def ensemble_multipass(imgs, passes, corr_min: float, s2n_min: float, count_min: float, signal_threshold: Optional[float] = None,
                       chunks=None, return_passes: bool = False):
    """Multi-pass ensemble correlation on one device: ``passes`` = ``[(n_0, overlap_0), ..., (n_K, overlap_K)]``
    coarsest first (or a ``window.MultiPassWindow``).  Every pass is a full ensemble over all pairs of ``imgs`` (a host stack or a
    ``DeviceFrames``); pass 0 is today's ensemble of its window, each later pass (16, 32 or 64 px) cuts frame t+1's windows at the integer
    offsets the previous pass's field predicts (:func:`predict_shift`, one field for every pair) and adds them to the residual it fits.
    ``chunks``: the frame slices ``[(f0, f1), ...]`` every pass is accumulated in (consecutive ones share a frame; None: one call); their
    number is the ``n_frames`` of the count filter, as in the reference's chunk loop (quirk Q3).
    Every pass but the last needs a grid of at least 3 x 3 windows (``window.ensemble_chain_spec``: NotImplementedError).
    Returns ``(u, v, corr_count, corr, s2n)`` of the LAST pass -- ``(1, n_rows, n_cols)``, count ``(n_win,)``; "v_sign" applied to v --
    and with ``return_passes`` a list with every pass's ``(u, v, corr_count, shift, mean planes)`` in the kernels' orientation (shift None
    for pass 0)."""
    spec = passes if isinstance(passes, window.MultiPassWindow) else None
    if spec is None:
        passes = [(int(n), int(o)) for n, o in passes]
        if not passes:
            raise ValueError("passes is empty")
        spec = window.multipass_spec((passes[-1][0],) * 2, (passes[-1][1],) * 2, passes[:-1])
        if not isinstance(spec, window.MultiPassWindow):
            spec = window.MultiPassWindow(passes)
    passes = list(spec.passes)
    a = imgs if is_device(imgs) else _lib.as_frames(imgs)
    T, H, W = a.shape
    if T < 2:
        raise ValueError(f"need >= 2 frames, got {a.shape}")
    window.ensemble_chain_spec(spec, (H, W))     # NotImplementedError for a steering pass of fewer than 3 x 3 windows
    _lib.load()
    _lib.require_device()
    chunks = [(0, T)] if chunks is None else [(int(f0), int(f1)) for f0, f1 in chunks]
    if chunks[0][0] != 0 or chunks[-1][1] != T or any(f1 - f0 < 2 for f0, f1 in chunks) or any(x[1] - 1 != y[0] for x, y in zip(chunks, chunks[1:])):
        raise ValueError(f"chunks must cover the frames 0 .. {T} in order, each at least two frames, consecutive ones sharing a frame; got {chunks}")
    flip = _lib.get_option("v_sign") == 1
    per, prev = [], None
    for k, (n, ov) in enumerate(passes):
        shift = None if k == 0 else predict_shift(prev[0], prev[1], (H, W), passes[k - 1], (n, ov))[0]
        e = Ensemble((H, W), (n, n), (ov, ov), shift=shift)
        try:
            cm, sn = (np.empty((T - 1, e.n_rows * e.n_cols), dtype=np.float32) for _ in range(2))
            for f0, f1 in chunks:
                e.accumulate(a[f0:f1], corr_min, s2n_min, signal_threshold, out=(cm[f0:f1 - 1], sn[f0:f1 - 1]))
            u, v, cnt, mean = e.finish(count_min, len(chunks), return_mean=True)
            used = e.shift
        finally:
            e.close()
        if flip:           # the kernels' orientation between the passes (a negation is exact)
            v = -v
        prev = (u, v)
        per.append((u, v, cnt, used, mean))
    corr, s2n = ensemble_means(cm, sn, cnt, count_min, len(chunks))
    shape = (1, e.n_rows, e.n_cols)
    ret = (u, -v if flip else v, cnt, corr.reshape(shape), s2n.reshape(shape))
    return ret + (per,) if return_passes else ret


def ensemble_allreduce(ensembles) -> None:
    """Sum the states of several :class:`Ensemble` handles (same geometry, any devices) in list order on the first one's device and
    leave the total in every handle, marked as a foreign state (``lspiv_ensemble_allreduce``): bit for bit what ``export_state`` of
    each, a float32 sum in list order and ``import_state`` of the total on each would leave, without the host round trip."""
    hs = [e._h for e in ensembles]
    if not hs or any(not h for h in hs):
        raise ValueError("ensemble_allreduce needs open Ensemble handles")
    arr = (C.c_void_p * len(hs))(*[h.value for h in hs])
    _lib.check(_lib.load().lspiv_ensemble_allreduce(arr, len(hs)))
