#!/usr/bin/env python
"""Rate of the masked per-pair kernels in one session on one box.

1080p uint8 resident in HBM (lspiv_synth_particles_dev), overlap 50 %, windows 16 / 32 / 64, a mask that excludes roughly a third of the
frame (everything left of a wavy line: windows of every class -- fully covered, partially covered, below k_min -- and windows below
k_min still occupy a job).  Per size, the PIV kernel alone (the library's events around it, "time_kernel": no rescue pass, no copies):
the masked kernel over PAIRS pairs and, in the same session, the shifted kernel at zero offsets (one window per job, as the masked one:
what is left between the two is the mask's row load, the selects and the integer reduction of the count).  No ratio is fixed in
advance.  Usage: masked_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed launches after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import math
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
H, W, WARMUP = 1080, 1920, 3
SIZES = ((16, 8), (32, 16), (64, 32))


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


def bank_mask():
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return (x >= W / 3.0 + 0.08 * W * np.sin(2 * np.pi * y / (0.61 * H)) + 0.02 * W * np.sin(2 * np.pi * y / (0.14 * H))).astype(np.uint8)


def main():
    lib = _lib.load()
    _lib.require_device()
    T = PAIRS + 1
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261019, 0.02))
    m = bank_mask()
    d_mask = DeviceFrames.from_host(m[None])
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "excluded_share": float(1.0 - m.mean())}
    _lib.set_option("time_kernel", 1)
    try:
        for n, o in SIZES:
            rows, cols = window.get_array_shape((H, W), (n, n), (o, o))
            n_win = rows * cols
            k_min = max(2, int(math.ceil(0.25 * n * n)))
            out = DeviceFrames.empty((4, PAIRS, n_win), np.float32)
            masked = lambda: _lib.check(lib.lspiv_piv_masked_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, d_mask.c_ptr, k_min, -1.0, 0,
                                                                          out.c_ptr, None, None))
            shifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, None, out.c_ptr, None, None))
            r = {"windows_per_pair": n_win, "masked_kernel_ms": kernel_ms(lib, masked), "shifted_kernel_ms": kernel_ms(lib, shifted)}
            r["masked_again_ms"] = kernel_ms(lib, masked)          # the order of the two is no part of the ratio
            r["masked_over_shifted"] = ratio(r["masked_kernel_ms"], r["shifted_kernel_ms"])
            r["masked_pairs_per_s"] = 1e3 * PAIRS / r["masked_kernel_ms"]["median"]
            del out
            res[f"{n}@{o}"] = r
    finally:
        _lib.set_option("time_kernel", 0)
        _lib.check(lib.lspiv_synchronize())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
