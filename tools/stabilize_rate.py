#!/usr/bin/env python
"""Rate of the stabilisation warp next to its siblings, in one session on one box.

1080p frames resident in HBM (lspiv_synth_particles_dev; float32: the same stack through filters.smooth), FRAMES frames, a pose per
frame that is a random walk of 1.5 px and 0.002 rad per frame (what a handheld camera does).  Every step puts two events on the
library's stream around ONE lspiv_warp_affine_dev call (one kernel launch, nothing else) and, for comparison, around
project_cv's fused undistort + warp remap and around time_diff on the same stack.  Bytes: the warp reads a frame and writes a frame
(2 x H x W x itemsize per frame, the figure of the "algorithmic" rate; the four neighbour loads of a pixel are cache hits).  Also one
estimate() call on a stack of the same size: masked PIV + fit + chain + the copies, by the wall clock.  No figure is fixed in advance.
Usage: stabilize_rate.py [FRAMES [STEPS]] (default 201 frames, 8 timed steps after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyorc_amd import _lib, filters, stabilize  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402
from pyorc_amd.project import ProjectionCV  # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 201
STEPS = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 8
H, W, WARMUP = 1080, 1920, 3


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def poses(T, seed=1):
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th = np.cumsum(rng.normal(size=T) * 0.002)
    d = np.cumsum(rng.normal(size=(T, 2)) * 1.5 / np.sqrt(2.0), axis=0)
    c, s = np.cos(th), np.sin(th)
    A = np.stack([np.stack([c, -s, cx - c * cx + s * cy + d[:, 0]], axis=1), np.stack([s, c, cy - s * cx - c * cy + d[:, 1]], axis=1)], axis=1)
    A[0] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    return np.ascontiguousarray(A)


def main():
    lib = _lib.load()
    _lib.require_device()
    T = FRAMES
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))

    def timed(call):
        spans = []
        for step in range(WARMUP + STEPS):
            _lib.check(lib.lspiv_event_record(e0))
            keep = call()     # noqa: F841  (the result stays alive until the span is read)
            _lib.check(lib.lspiv_event_record(e1))
            _lib.check(lib.lspiv_synchronize())
            span = C.c_float(0)
            _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(span)))
            if step >= WARMUP:
                spans.append(span.value)
        return np.asarray(spans)

    A = poses(T)
    d_A = DeviceFrames.empty((1, 1, A.nbytes), np.uint8)
    _lib.check(lib.lspiv_memcpy_h2d(d_A.c_ptr, _lib.ptr(A), A.nbytes))
    K = np.array([[1500.0, 0, 960], [0, 1500.0, 540], [0, 0, 1]])
    dist = [-0.12, 0.03, 0.0005, -0.0003, 0.0]
    M = np.array([[0.95, 0.04, 20.0], [0.01, 0.9, 30.0], [1e-5, 2e-5, 1.0]])
    res = {"frames": T, "steps": STEPS, "frame": [H, W]}
    try:
        for dtype in (np.uint8, np.float32):
            d = DeviceFrames.empty((T, H, W), np.uint8)
            _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261021, 0.02))
            if dtype == np.float32:
                d = filters.smooth(d, 1)
            out = DeviceFrames.empty(d.shape, d.dtype)
            code, item = d.dtype_code, d.dtype.itemsize
            ms = timed(lambda: _lib.check(lib.lspiv_warp_affine_dev(d.c_ptr, code, T, H, W, d_A.c_ptr, out.c_ptr, None)))
            r = {"warp_ms": stats(ms), "warp_frames_per_s": T / (np.median(ms) * 1e-3),
                 "warp_algorithmic_TB_per_s": 2.0 * T * H * W * item / (np.median(ms) * 1e-3) / 1e12}
            p = ProjectionCV((H, W), (H, W), K, dist, M)
            cv = timed(lambda: p.project_frames(d))
            p.close()
            r["project_cv_fused_ms"] = stats(cv)
            td = timed(lambda: filters.time_diff(d))
            r["time_diff_ms"] = stats(td)
            r["warp_over_project_cv"] = float(np.median(ms) / np.median(cv))
            r["warp_over_time_diff"] = float(np.median(ms) / np.median(td))
            if dtype == np.uint8:    # the estimator on the same stack: masked PIV on a bank strip + fit + chain + copies, wall clock
                mask = np.zeros((H, W), dtype=bool)
                mask[:, :480] = True
                with warnings.catch_warnings():      # (random particles: pairs without consistent vectors are expected here)
                    warnings.simplefilter("ignore", RuntimeWarning)
                    stabilize.estimate(d, mask)
                    t0 = time.perf_counter()
                    tr = stabilize.estimate(d, mask)
                    r["estimate_wall_ms"] = (time.perf_counter() - t0) * 1e3
                r["estimate_n_used_median"] = int(np.median(tr.n_used))
            res[np.dtype(dtype).name] = r
            del d, out
    finally:
        _lib.check(lib.lspiv_synchronize())
        lib.lspiv_event_destroy(e0)
        lib.lspiv_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
