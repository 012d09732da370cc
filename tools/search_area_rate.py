#!/usr/bin/env python
"""Rate of the search-area kernels against the per-pair kernels of the same transform size, in one session on one box.

1080p uint8, 1000 pairs resident in HBM (lspiv_synth_particles_dev); per configuration a warm-up, then the kernel time of 20 launches
from the library's own events around the PIV kernel ("time_kernel" option: what rocprofv3 --kernel-trace reports for it).
  16 in 32 @ 16  vs  32 x 32 @ 16 with walk = 0        32 in 64 @ 48  vs  64 x 64 @ 48 with walk = 0
(the same three transforms per pair; the walking kernels carry a spectrum this mode cannot).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

T, H, W, STEPS, WARMUP = 1001, 1080, 1920, 20, 3


def kernel_ms(lib, call):
    for _ in range(WARMUP):
        call()
    _lib.check(lib.lspiv_synchronize())
    ms, n = (C.c_float * 16)(), C.c_int(0)
    _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))   # empties the ring
    out = []
    for _ in range(STEPS):
        call()
        _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(n)))
        out.extend(ms[k] for k in range(n.value))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    lib = _lib.load()
    _lib.require_device()
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20260927, 0.02))
    _lib.set_option("time_kernel", 1)
    res = {}
    for n, S, ov in ((16, 32, 16), (32, 64, 48)):
        nr, nc = window.get_array_shape((H, W), (S, S), (ov, ov))
        out = DeviceFrames.empty((4, T - 1, nr * nc), np.float32)
        search = lambda: _lib.check(lib.lspiv_piv_search_pairs_dev_at(d.c_ptr, 0, T, H, W, S, S, n, n, ov, ov, -1.0, 0, out.c_ptr, None, None))
        plain = lambda: _lib.check(lib.lspiv_piv_pairs_dev_at(d.c_ptr, 0, T, H, W, S, S, ov, ov, -1.0, 0, out.c_ptr, None, None))
        s = kernel_ms(lib, search)
        _lib.set_option("walk", 0)
        p = kernel_ms(lib, plain)
        _lib.set_option("walk", -1)
        res[f"{n}in{S}@{ov}"] = {"search_kernel_ms": s, "per_pair_walk0_kernel_ms": p, "search_pairs_per_s": 1e3 * (T - 1) / s[0],
                                 "per_pair_pairs_per_s": 1e3 * (T - 1) / p[0], "ratio": s[0] / p[0]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
