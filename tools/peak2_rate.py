#!/usr/bin/env python
"""Rate of the second-peak per-pair kernels in one session on one box.

1080p uint8 resident in HBM (lspiv_synth_particles_dev), overlap 50 %, windows 16 / 32 / 64, exclusion radius 2.  Per size, the PIV
kernel alone (the library's events around it, "time_kernel": no rescue pass, no copies): the second-peak kernel over PAIRS pairs and, in
the same session, the shifted kernel at zero offsets -- the very job the second-peak kernel starts from, so what is left between the two
is the epilogue: N compares per lane against the floor, the box and four neighbours, N / 2 LDS reads per lane, two group reductions, the
fit, one 16-byte store per window.  No ratio is fixed in advance.  Usage: peak2_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed
launches after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
H, W, WARMUP = 1080, 1920, 3
SIZES = ((16, 8), (32, 16), (64, 32))
RADIUS = 2


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def kernel_ms(lib, call):
    """PIV-kernel time of ONE `call` (the "time_kernel" ring; every call here is one launch)."""
    for _ in range(WARMUP):
        call()
    _lib.check(lib.lspiv_synchronize())
    ms, n = (C.c_float * 16)(), C.c_int(0)
    _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))   # empties the ring
    out = []
    for _ in range(STEPS):
        call()
        _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))
        out.append(sum(ms[k] for k in range(n.value)))
    return stats(out)


def ratio(a, b):
    """median / median, and the range the two min - max spans allow"""
    return {"median": a["median"] / b["median"], "min": a["min"] / b["max"], "max": a["max"] / b["min"]}


def main():
    lib = _lib.load()
    _lib.require_device()
    T = PAIRS + 1
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261019, 0.02))
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "peak_exclusion": RADIUS}
    _lib.set_option("time_kernel", 1)
    try:
        for n, o in SIZES:
            rows, cols = window.get_array_shape((H, W), (n, n), (o, o))
            n_win = rows * cols
            out = DeviceFrames.empty((4, PAIRS, n_win), np.float32)
            second = DeviceFrames.empty((PAIRS, n_win, 4), np.float32)
            peak2 = lambda: _lib.check(lib.lspiv_piv_peak2_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, RADIUS, out.c_ptr,
                                                                        second.c_ptr, None, None))
            shifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, None, out.c_ptr, None, None))
            r = {"windows_per_pair": n_win, "peak2_kernel_ms": kernel_ms(lib, peak2), "shifted_kernel_ms": kernel_ms(lib, shifted)}
            r["peak2_again_ms"] = kernel_ms(lib, peak2)          # the order of the two is no part of the ratio
            r["peak2_over_shifted"] = ratio(r["peak2_kernel_ms"], r["shifted_kernel_ms"])
            r["peak2_pairs_per_s"] = 1e3 * PAIRS / r["peak2_kernel_ms"]["median"]
            del out, second
            res[f"{n}@{o}"] = r
    finally:
        _lib.set_option("time_kernel", 0)
        _lib.check(lib.lspiv_synchronize())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
