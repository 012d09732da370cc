#!/usr/bin/env python
"""Rate of the SPOF phase-filtered kernels in one session on one box.

1080p uint8 resident in HBM (lspiv_synth_particles_dev), overlap 50 %, windows 16 / 32 / 64.  Per size, the PIV kernel alone (the
library's events around it, "time_kernel": no rescue pass, no copies): the filtered per-pair kernel over PAIRS pairs against the
per-pair kernel of the plain path ("walk" = 0: two windows per job, the mean from the DC bin) and against the shifted kernel at zero
offsets (one window per job, as the filtered one: what is left between the two is the filter and the reduction of the clipped plane's
mean); and the filtered ensemble kernel over ENS_PAIRS pairs against the one-owner shifted ensemble kernel at zero offsets.  No ratio is
fixed in advance.  Usage: spof_rate.py [PAIRS [ENS_PAIRS [STEPS]]] (default 200 pairs, 1000 ensemble pairs, 8 timed launches after 3
warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ENS_PAIRS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 8
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


def main():
    lib = _lib.load()
    _lib.require_device()
    T = max(PAIRS, ENS_PAIRS) + 1
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261019, 0.02))
    res = {"pairs": PAIRS, "ensemble_pairs": ENS_PAIRS, "steps": STEPS, "frame": [H, W]}
    _lib.set_option("time_kernel", 1)
    try:
        for n, o in SIZES:
            rows, cols = window.get_array_shape((H, W), (n, n), (o, o))
            n_win = rows * cols
            out = DeviceFrames.empty((4, PAIRS, n_win), np.float32)
            filtered = lambda: _lib.check(lib.lspiv_piv_spof_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, out.c_ptr, None, None))
            plain = lambda: _lib.check(lib.lspiv_piv_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, out.c_ptr, None, None))
            shifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, None, out.c_ptr, None, None))
            r = {"windows_per_pair": n_win, "filtered_kernel_ms": kernel_ms(lib, filtered), "shifted_kernel_ms": kernel_ms(lib, shifted)}
            _lib.set_option("walk", 0)
            try:
                r["per_pair_kernel_ms"] = kernel_ms(lib, plain)
            finally:
                _lib.set_option("walk", -1)
            r["filtered_over_shifted"] = ratio(r["filtered_kernel_ms"], r["shifted_kernel_ms"])
            r["filtered_over_per_pair"] = ratio(r["filtered_kernel_ms"], r["per_pair_kernel_ms"])
            r["filtered_windows_per_s"] = 1e3 * PAIRS * n_win / r["filtered_kernel_ms"]["median"]
            del out
            # the ensembles: one handle each, accumulated into over and over (the sums grow, the work per launch does not change)
            cs = DeviceFrames.empty((2, ENS_PAIRS, n_win), np.float32)
            hs = []
            try:
                for kind in ("filtered", "shifted"):
                    h = C.c_void_p()
                    _lib.check(lib.lspiv_ensemble_begin(H, W, n, n, o, o, C.byref(h)))
                    hs.append(h)
                    if kind == "filtered":
                        _lib.check(lib.lspiv_ensemble_set_spectral_filter(h, 1))
                    else:
                        zero = np.zeros((n_win, 2), np.int16)
                        _lib.check(lib.lspiv_ensemble_set_shift(h, _lib.ptr(zero)))
                    acc = lambda h=h: _lib.check(lib.lspiv_ensemble_accumulate_dev(h, d.c_ptr, 0, ENS_PAIRS + 1, 0.0, 0.5, -1.0, cs.c_ptr, None))
                    r[f"{kind}_ensemble_kernel_ms"] = kernel_ms(lib, acc)
            finally:
                _lib.check(lib.lspiv_synchronize())
                for h in hs:
                    lib.lspiv_ensemble_destroy(h)
            r["filtered_over_shifted_ensemble"] = ratio(r["filtered_ensemble_kernel_ms"], r["shifted_ensemble_kernel_ms"])
            r["filtered_ensemble_pairs_per_s"] = 1e3 * ENS_PAIRS / r["filtered_ensemble_kernel_ms"]["median"]
            del cs
            res[f"{n}@{o}"] = r
    finally:
        _lib.set_option("time_kernel", 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
