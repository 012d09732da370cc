#!/usr/bin/env python
"""Rate of multi-pass PIV in one session on one box.

1080p uint8, PAIRS pairs resident in HBM (lspiv_synth_particles_dev), overlap 50 % in every pass, the chains 64 -> 32 -> 16 and 64 -> 32.
Per pass size: the kernel time of the shifted kernel (offsets: the chain's own prediction for that pass) against the per-pair kernel
(walk = 0) and the walking kernel of the same window -- from the library's events around the PIV kernel ("time_kernel" option: what
rocprofv3 --kernel-trace reports for it).  The predictor, the whole shifted call (kernel + rescue pass + add step) with and without an
offset array -- their difference is the add step --, and the whole chain between two events on the library's stream.
Usage: multipass_rate.py [PAIRS [STEPS]] (default 200 pairs, 10 timed launches after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
T, H, W, WARMUP = PAIRS + 1, 1080, 1920, 3
CHAINS = ([(64, 32), (32, 16), (16, 8)], [(64, 32), (32, 16)])


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def kernel_ms(lib, call):
    """PIV-kernel time of `call`'s launches (the "time_kernel" ring)."""
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
    return stats(out)


def span_ms(lib, call):
    """Time of everything `call` puts on the library's stream, between two events."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))
    out = []
    for k in range(WARMUP + STEPS):
        _lib.check(lib.lspiv_event_record(e0))
        call()
        _lib.check(lib.lspiv_event_record(e1))
        _lib.check(lib.lspiv_synchronize())
        ms = C.c_float(0)
        _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(ms)))
        if k >= WARMUP:
            out.append(ms.value)
    lib.lspiv_event_destroy(e0)
    lib.lspiv_event_destroy(e1)
    return stats(out)


def main():
    lib = _lib.load()
    _lib.require_device()
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20260927, 0.02))
    grid = {n: window.get_array_shape((H, W), (n, n), (o, o)) for n, o in CHAINS[0]}
    tiles = {n: PAIRS * g[0] * g[1] for n, g in grid.items()}
    out = DeviceFrames.empty((4, 1, max(tiles.values())), np.float32)
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "windows_per_pair": {str(n): g[0] * g[1] for n, g in grid.items()}}
    # the chains first: they leave the last pass's predicted offsets behind, which the per-pass measurements reuse
    shifts = {}
    for chain in CHAINS:
        n, o = chain[-1]
        arr = (C.c_int * (4 * len(chain)))(*[q for m, ov in chain for q in (m, m, ov, ov)])
        sh = DeviceFrames.empty((1, 1, tiles[n] * 4), np.uint8)
        run = lambda: _lib.check(lib.lspiv_piv_multipass_dev_at(d.c_ptr, 0, T, H, W, len(chain), arr, -1.0, 0, out.c_ptr, None, sh.c_ptr, None))
        t = span_ms(lib, run)
        res["chain " + "->".join(str(m) for m, _ in chain)] = {"ms": t, "pairs_per_s": 1e3 * PAIRS / t["median"]}
        shifts[n] = sh
    _lib.set_option("time_kernel", 1)
    for k, (n, o) in enumerate(CHAINS[0]):
        plain = lambda: _lib.check(lib.lspiv_piv_pairs_dev_at(d.c_ptr, 0, T, H, W, n, n, o, o, -1.0, 0, out.c_ptr, None, None))
        r = {"walking_kernel_ms": kernel_ms(lib, plain)}
        _lib.set_option("walk", 0)
        r["per_pair_walk0_kernel_ms"] = kernel_ms(lib, plain)
        _lib.set_option("walk", -1)
        if k:
            sh = shifts[n]
            shifted = lambda s=sh: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, T, H, W, n, n, o, o, -1.0, 0, s.c_ptr, out.c_ptr, None, None))
            unshifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, T, H, W, n, n, o, o, -1.0, 0, None, out.c_ptr, None, None))
            r["shifted_kernel_ms"] = kernel_ms(lib, shifted)
            r["shifted_zero_offsets_kernel_ms"] = kernel_ms(lib, unshifted)
            r["shifted_over_per_pair"] = r["shifted_kernel_ms"]["median"] / r["per_pair_walk0_kernel_ms"]["median"]
            r["shifted_over_walking"] = r["shifted_kernel_ms"]["median"] / r["walking_kernel_ms"]["median"]
            _lib.set_option("time_kernel", 0)
            r["shifted_call_ms"] = span_ms(lib, shifted)               # kernel + rescue pass + add step
            r["shifted_call_no_offsets_ms"] = span_ms(lib, unshifted)  # kernel + rescue pass
            r["add_step_ms"] = r["shifted_call_ms"]["median"] - r["shifted_call_no_offsets_ms"]["median"]
            nc, oc = CHAINS[0][k - 1]
            _lib.check(lib.lspiv_piv_pairs_dev_at(d.c_ptr, 0, T, H, W, nc, nc, oc, oc, -1.0, 0, out.c_ptr, None, None))
            _lib.check(lib.lspiv_synchronize())
            pred = lambda: _lib.check(lib.lspiv_piv_predict_shift_dev(out.c_ptr, C.c_void_p(out.ptr + 4 * tiles[nc]), PAIRS, H, W, nc, nc, oc, oc,
                                                                      n, n, o, o, sh.c_ptr, None))
            r["predictor_ms"] = span_ms(lib, pred)
            _lib.set_option("time_kernel", 1)
        res[f"{n}@{o}"] = r
    _lib.set_option("time_kernel", 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
