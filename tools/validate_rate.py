#!/usr/bin/env python
"""Time of the vector validation kernel next to the second-peak PIV kernel, in one session on one box.

1080p uint8 resident in HBM (lspiv_synth_particles_dev), 32 x 32 windows at 16 px overlap, exclusion radius 2, PAIRS pairs.  Every step
runs the second-peak PIV call (its kernel time from the library's "time_kernel" ring: no rescue pass, no copies) and then
lspiv_validate_dev on that call's fresh result block, between two events on the library's stream, with the runner-up offered:
ITERATIONS = 2 and 8 are that many kernel launches and nothing else (the fields ping-pong between the block and the workspace), so the
time per iteration is the span over the count; ITERATIONS = 1 is one launch plus the two device-to-device copies an odd count starts
with -- what get_ffpiv(validate=True) pays.  Not isolated: the gaps between back-to-back launches on the stream and the events' own
cost, both inside every span.  No figure is fixed in advance.  Usage: validate_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed steps
after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, validate, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
STEPS = max(8, int(sys.argv[2])) if len(sys.argv) > 2 else 8
H, W, WARMUP = 1080, 1920, 3
N, OV, RADIUS = 32, 16, 2
ITERATIONS = (1, 2, 8)


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def main():
    lib = _lib.load()
    _lib.require_device()
    T = PAIRS + 1
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261020, 0.02))
    rows, cols = window.get_array_shape((H, W), (N, N), (OV, OV))
    n_win = rows * cols
    out = DeviceFrames.empty((4, PAIRS, n_win), np.float32)
    second = DeviceFrames.empty((PAIRS, n_win, 4), np.float32)
    flag = DeviceFrames.empty((1, 1, PAIRS * n_win), np.uint8)
    d_v = C.c_void_p(out.ptr + 4 * PAIRS * n_win)
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))
    ms, n = (C.c_float * 16)(), C.c_int(0)
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "window": [N, OV], "windows_per_pair": n_win, "vectors": PAIRS * n_win}
    piv_ms = []
    _lib.set_option("time_kernel", 1)
    try:
        for it in ITERATIONS:
            spec = validate.validate_spec(True, iterations=it)
            spans, flags = [], None
            for step in range(WARMUP + STEPS):
                _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))   # empties the ring
                _lib.check(lib.lspiv_piv_peak2_pairs_dev_at(d.c_ptr, 0, T, H, W, N, N, OV, OV, -1.0, 0, RADIUS, out.c_ptr, second.c_ptr, None, None))
                _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))
                k_ms = sum(ms[k] for k in range(n.value))
                _lib.check(lib.lspiv_event_record(e0))
                validate.run_dev(spec, out.c_ptr, d_v, second.c_ptr, (PAIRS, rows, cols), flag.c_ptr)
                _lib.check(lib.lspiv_event_record(e1))
                _lib.check(lib.lspiv_synchronize())
                span = C.c_float(0)
                _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(span)))
                if step >= WARMUP:
                    spans.append(span.value)
                    piv_ms.append(k_ms)
                flags = np.bincount(flag.to_host().ravel(), minlength=4).tolist() if step == WARMUP + STEPS - 1 else flags
            r = {"call_ms": stats(spans), "flags": flags}
            if it % 2 == 0:
                r["per_iteration_ms"] = stats(np.asarray(spans) / it)
            res[f"iterations_{it}"] = r
    finally:
        _lib.set_option("time_kernel", 0)
        _lib.check(lib.lspiv_synchronize())
        lib.lspiv_event_destroy(e0)
        lib.lspiv_event_destroy(e1)
    res["peak2_kernel_ms"] = stats(piv_ms)
    per = res["iterations_8"]["per_iteration_ms"]
    res["iteration_over_peak2_kernel"] = {"median": per["median"] / res["peak2_kernel_ms"]["median"], "min": per["min"] / res["peak2_kernel_ms"]["max"],
                                          "max": per["max"] / res["peak2_kernel_ms"]["min"]}
    res["one_call_over_peak2_kernel"] = res["iterations_1"]["call_ms"]["median"] / res["peak2_kernel_ms"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
