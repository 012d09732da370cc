"""Vector validation on the MI355X: the normalised median test (Westerweel & Scarano 2005) over the 3 x 3 neighbourhood of every vector,
with the runner-up vector of the second correlation peak as the first substitute for a rejected one (INTEGRATION.md section 2j;
``lspiv_validate`` / ``lspiv_validate_dev`` in include/lspiv.h state the rule).

No CPU fallback: every function needs liblspiv_hip.so and a gfx950 device.
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _lib

REPLACE = ("nan", "median")      # LSPIV_VALIDATE_NAN, LSPIV_VALIDATE_MEDIAN
FLAG_KEPT, FLAG_REJECTED, FLAG_SUBSTITUTED, FLAG_MEDIAN = 0, 1, 2, 3


class ValidateSpec(NamedTuple):
    """The checked parameters of the median test, in the order of the C ABI."""
    threshold: float = 2.0
    epsilon: float = 0.1
    min_neighbours: int = 3
    replace: int = 0
    iterations: int = 1


def validate_spec(validate=True, **params) -> Optional[ValidateSpec]:
    """``validate`` of ``get_ffpiv`` -- None / False (no validation: None), True (the defaults), a dict of :func:`median_test`'s
    keywords or a ``ValidateSpec`` -- checked; ``params``: the keywords themselves.  ValueError for a value outside its range."""
    if validate is None or validate is False:
        return None
    if isinstance(validate, ValidateSpec):
        return validate
    if validate is not True:
        if not isinstance(validate, dict):
            raise ValueError(f"validate must be None, True or a dict of median_test's keywords, got {validate!r}")
        params = {**validate, **params}
    unknown = set(params) - {"threshold", "epsilon", "min_neighbours", "replace", "iterations"}
    if unknown:
        raise ValueError(f"validate: unknown keyword(s) {sorted(unknown)}")
    threshold, epsilon = float(params.get("threshold", 2.0)), float(params.get("epsilon", 0.1))
    m, it, replace = params.get("min_neighbours", 3), params.get("iterations", 1), params.get("replace", "nan")
    if not (threshold > 0.0) or not np.isfinite(np.float32(threshold)):
        raise ValueError(f"threshold must be a positive number, got {threshold}")
    if not (epsilon >= 0.0) or not np.isfinite(np.float32(epsilon)):
        raise ValueError(f"epsilon must be a number >= 0, got {epsilon}")
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= 8:
        raise ValueError(f"min_neighbours must be a whole number 1 .. 8, got {m}")
    if isinstance(it, bool) or int(it) != it or not 1 <= int(it) <= 8:
        raise ValueError(f"iterations must be a whole number 1 .. 8, got {it}")
    if replace not in REPLACE:
        raise ValueError(f"replace must be one of {REPLACE}, got {replace!r}")
    return ValidateSpec(threshold, epsilon, int(m), REPLACE.index(replace), int(it))


def run_host(spec: ValidateSpec, u, v, second, flag) -> None:
    """``lspiv_validate`` in place on the C-contiguous float32 host arrays ``u``, ``v`` (T, R, C); ``second`` (T, R, C, 4) or None;
    ``flag`` uint8 (T, R, C) or None."""
    T, R, Cc = u.shape
    _lib.check(_lib.load().lspiv_validate(_lib.ptr(u), _lib.ptr(v), None if second is None else _lib.ptr(second), T, R, Cc,
                                          spec.threshold, spec.epsilon, spec.min_neighbours, spec.replace, spec.iterations,
                                          None if flag is None else _lib.ptr(flag)))


def run_dev(spec: ValidateSpec, d_u, d_v, d_second, grid, d_flag, stream=None) -> None:
    """``lspiv_validate_dev`` in place on device pointers (``ctypes.c_void_p`` or None) of a ``grid`` = (T, R, C) block."""
    T, R, Cc = grid
    _lib.check(_lib.load().lspiv_validate_dev(d_u, d_v, d_second, T, R, Cc, spec.threshold, spec.epsilon, spec.min_neighbours,
                                              spec.replace, spec.iterations, d_flag, C.c_void_p(stream) if stream else None))


def median_test(u, v, second=None, threshold: float = 2.0, epsilon: float = 0.1, min_neighbours: int = 3, replace: str = "nan",
                iterations: int = 1):
    """The normalised median test on the fields ``u``, ``v`` -- float32 ``(T, R, C)`` or ``(R, C)`` -- on the device; returns NEW arrays
    ``(u, v, flag)`` of the input's shape.

    Per vector, against its up to eight neighbours of the same time step that are finite in both components (n of them, no wrap): with
    ``um``, ``vm`` their medians and ``ru``, ``rv`` the medians of ``|u_k - um|``, ``|v_k - vm|``, a vector that is finite and has
    ``n >= min_neighbours`` is an OUTLIER when ``|u - um| > threshold * (ru + epsilon)`` or the same holds for v (``epsilon`` in the units
    of the fields: 0.1 is meant for pixels).  An outlier becomes, in this order: the runner-up ``(second[..., 0], second[..., 1])`` when
    ``second`` (``(..., 4)``, the ``peak2`` of ``piv.piv_pairs_peak2``) is given, the vector is still the primary one and the runner-up
    is finite and no outlier against the same limits (flag 2); NaN with ``replace="nan"`` (flag 1); the neighbourhood median with
    ``replace="median"`` (flag 3).  Anything else -- NaN, too few neighbours -- is left as it is, flag 0: NaN is never filled.
    ``iterations`` (1 .. 8): every iteration reads the field of the one before it; a substituted or median vector is judged again like
    any other, the flag is the last action taken.  ValueError for a value outside its range or for shapes that do not match."""
    spec = validate_spec(True, threshold=threshold, epsilon=epsilon, min_neighbours=min_neighbours, replace=replace, iterations=iterations)
    uu, vv = np.array(u, dtype=np.float32, order="C"), np.array(v, dtype=np.float32, order="C")     # new arrays: worked on in place
    if uu.ndim not in (2, 3) or uu.shape != vv.shape or 0 in uu.shape:
        raise ValueError(f"u and v must have one shape (T, R, C) or (R, C) without an empty axis, got {uu.shape} and {vv.shape}")
    shape = uu.shape
    uu, vv = uu.reshape((-1,) + shape[-2:]), vv.reshape((-1,) + shape[-2:])
    if second is not None:
        second = np.ascontiguousarray(second, dtype=np.float32)
        if second.shape != shape + (4,):
            raise ValueError(f"second must have shape {shape + (4,)}, got {second.shape}")
    flag = np.empty(uu.shape, dtype=np.uint8)
    _lib.load()
    _lib.require_device()
    run_host(spec, uu, vv, second, flag)
    return uu.reshape(shape), vv.reshape(shape), flag.reshape(shape)
