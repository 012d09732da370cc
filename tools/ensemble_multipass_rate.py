#!/usr/bin/env python
"""Times of the multi-pass ensemble in one session on one box.

1080p uint8, PAIRS pairs resident in HBM (lspiv_synth_particles_dev), overlap 50 % in every pass, the chains 64 -> 32 and 64 -> 32 -> 16.
Per pass of a chain: the accumulate call of the whole stack (kernel time from the library's events around the PIV kernel, "time_kernel"
option, and the whole call between two events on the library's stream) and the finish (mean planes, fit, float64 rescue with the stack
borrowed, add step, copy to the host: wall time) -- the shifted passes with the chain's own predicted offsets.  Next to them, the
yardstick: the plain ensemble of the same window in the same session -- the walking ensemble kernel (the default) and the one-owner
ensemble kernel (walk = 0), the kernel the shifted ensemble kernel is built from.
Usage: ensemble_multipass_rate.py [PAIRS [STEPS]] (default 1000 pairs, 5 timed launches after 2 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, piv  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, H, W, WARMUP = PAIRS + 1, 1080, 1920, 2
CHAINS = ([(64, 32), (32, 16)], [(64, 32), (32, 16), (16, 8)])
MASKS = (0.2, 3.0, 0.2)     # corr_min, s2n_min, count_min: the ensemble's defaults


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def run_pass(lib, d, n, o, shift, out):
    """One pass on fresh handles, WARMUP + STEPS times: kernel ms, accumulate-call ms, finish ms, and the field of the last run."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))
    ms, cnt = (C.c_float * 16)(), C.c_int(0)
    kern, call, fin, field = [], [], [], None
    for k in range(WARMUP + STEPS):
        e = piv.Ensemble((H, W), (n, n), (o, o), shift=shift)
        try:
            e.set_retain(e.RETAIN_BORROW)
            _lib.check(lib.lspiv_synchronize())
            _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(cnt)))   # empties the ring
            _lib.check(lib.lspiv_event_record(e0))
            e.accumulate_dev(d.ptr, d.dtype, T, MASKS[0], MASKS[1], out.ptr)
            _lib.check(lib.lspiv_event_record(e1))
            _lib.check(lib.lspiv_synchronize())
            el = C.c_float(0)
            _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(el)))
            _lib.check(lib.lspiv_kernel_times(ms, 16, C.byref(cnt)))
            t0 = time.perf_counter()
            u, v, _ = e.finish(MASKS[2], 1)
            t1 = time.perf_counter()
            if k >= WARMUP:
                kern.append(sum(ms[i] for i in range(cnt.value)))
                call.append(el.value)
                fin.append(1e3 * (t1 - t0))
            field, st = (u, v), e.stats()
        finally:
            e.close()
    lib.lspiv_event_destroy(e0)
    lib.lspiv_event_destroy(e1)
    return {"kernel_ms": stats(kern), "accumulate_call_ms": stats(call), "finish_ms": stats(fin), "flagged": st["flagged"],
            "rescued": st["rescued"]}, field


def main():
    lib = _lib.load()
    _lib.require_device()
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20260927, 0.02))
    n_win = {n: int(np.prod(piv.window.get_array_shape((H, W), (n, n), (o, o)))) for n, o in CHAINS[1]}
    out = DeviceFrames.empty((2, PAIRS, max(n_win.values())), np.float32)
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "windows": {str(n): w for n, w in n_win.items()}}
    _lib.set_option("time_kernel", 1)
    flip = _lib.get_option("v_sign") == 1
    for chain in CHAINS:
        r, prev, total = {}, None, 0.0
        for k, (n, o) in enumerate(chain):
            shift = None if k == 0 else piv.predict_shift(prev[0], -prev[1] if flip else prev[1], (H, W), chain[k - 1], (n, o))[0]
            r[f"pass {k}: {n}@{o}" + (" shifted" if k else "")], prev = run_pass(lib, d, n, o, shift, out)
            p = r[f"pass {k}: {n}@{o}" + (" shifted" if k else "")]
            total += p["accumulate_call_ms"]["median"] + p["finish_ms"]["median"]
        r["accumulate_and_finish_ms"] = total
        res["chain " + "->".join(str(m) for m, _ in chain)] = r
    # the yardstick: the plain ensemble of every window of the chains, both of its kernels, and the shifted kernel with zero offsets
    for n, o in CHAINS[1]:
        y = {"walking_ensemble": run_pass(lib, d, n, o, None, out)[0]}
        _lib.set_option("walk", 0)
        y["one_owner_ensemble_walk0"] = run_pass(lib, d, n, o, None, out)[0]
        _lib.set_option("walk", -1)
        rows, cols = piv.window.get_array_shape((H, W), (n, n), (o, o))
        y["shifted_zero_offsets"] = run_pass(lib, d, n, o, np.zeros((rows, cols, 2), np.int16), out)[0]
        for key in ("walking_ensemble", "one_owner_ensemble_walk0"):
            y["shifted_over_" + key] = y["shifted_zero_offsets"]["kernel_ms"]["median"] / y[key]["kernel_ms"]["median"]
        res[f"plain {n}@{o}"] = y
    _lib.set_option("time_kernel", 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
