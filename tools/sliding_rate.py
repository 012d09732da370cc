#!/usr/bin/env python
"""Rate of the sliding ensemble next to the plain ensemble, same stack, same session.

A 1080p uint8 stack resident in HBM (synthetic particles), 32 x 32 @ 50 %, 1000 pairs: wall time of accumulate + sliding finish for
(M, s) = (30, 10), (30, 30), (8, 1), and of the plain ensemble's accumulate + finish.  Prints one JSON line.

    python tools/sliding_rate.py [--pairs 1000] [--repeats 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pyorc_amd import _lib, piv  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=32)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    H, W, T, n = 1080, 1920, a.pairs + 1, a.window
    stack = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(C.c_void_p(stack.ptr), T, H, W, 20261018, C.c_float(0.02)))

    def run(sliding):
        e = piv.Ensemble((H, W), (n, n), (n // 2, n // 2), sliding=sliding)
        try:
            e.set_retain(e.RETAIN_BORROW)
            if sliding:
                e.reserve_sliding(a.pairs)       # the whole block store (32 MB per block), allocated outside the timed region
            _lib.check(lib.lspiv_synchronize())
            t0 = time.perf_counter()
            e.accumulate(stack, 0.1, 1.5)
            t1 = time.perf_counter()
            out = e.finish_sliding(0.2) if sliding else e.finish(0.2, 1)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, len(out[0]), e.stats()
        finally:
            e.close()

    res = {"pairs": a.pairs, "frame": [H, W], "window": n, "dtype": "uint8", "repeats": a.repeats, "cases": {}}
    for name, sliding in (("plain", None), ("30/10", (30, 10)), ("30/30", (30, 30)), ("8/1", (8, 1))):
        run(sliding)    # warm-up: the workspaces of the context (every run makes a handle, and a block store, of its own)
        acc, fin, st, n_out = [], [], None, 0
        for _ in range(a.repeats):
            ta, tf, n_out, st = run(sliding)
            acc.append(ta); fin.append(tf)
        tot = np.array(acc) + np.array(fin)
        res["cases"][name] = {"outputs": n_out, "accumulate_ms": [round(1e3 * v, 2) for v in acc], "finish_ms": [round(1e3 * v, 2) for v in fin],
                              "total_ms_median": round(1e3 * float(np.median(tot)), 2), "total_ms_min_max": [round(1e3 * float(tot.min()), 2), round(1e3 * float(tot.max()), 2)],
                              "pairs_per_s_median": round(a.pairs / float(np.median(tot))), "flagged": st["flagged"], "rescued": st["rescued"]}
        print(name, json.dumps(res["cases"][name]), file=sys.stderr, flush=True)
    plain = res["cases"]["plain"]["total_ms_median"]
    for name, (M, s) in (("30/10", (30, 10)), ("30/30", (30, 30)), ("8/1", (8, 1))):
        c = res["cases"][name]
        c["times_plain"] = round(c["total_ms_median"] / plain, 2)
        c["q"] = M // s              # the Python loop it replaces correlates every pair q times
    print(json.dumps(res))


if __name__ == "__main__":
    main()
