"""get_ffpiv(devices=...) from one process: pairs/s of devices=None, [0, 0] and "all" on a 1080p uint8 host stack (32 x 32 @ 16) and on
the lazy project_hip hand-off (tests/lazy_doubles.py style), and the time of lspiv_ensemble_allreduce against export + numpy sum +
import for two 1080p 64 x 64 @ 75 % handles.  Prints one JSON line.

    python tools/multi_device_bench.py [n_pairs] [repeats]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from pyorc_amd import _lib, executor, frames as F, piv, plugin  # noqa: E402
from pyorc_amd.synth import particle_stack, projection_maps  # noqa: E402


def best_rate(fn, n_pairs, repeats):
    fn()                                     # warm-up: plans, pools, code objects
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return n_pairs / best, {k: executor.LAST_STATS.get(k) for k in ("devices", "chunks", "waited_s", "load_s", "idle_devices")}


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    _lib.require_device()
    out = {"n_pairs": n_pairs, "devices_visible": _lib.device_count()}
    modes = {"none": None, "0,0": [0, 0], "all": "all"}

    # 1. host uint8 stack, 1080p, 32 x 32 @ 16
    fr = particle_stack(n_pairs + 1, 1080, 1920, seed=3)
    t = np.arange(n_pairs + 1) / 25.0
    for name, dev in modes.items():
        rate, st = best_rate(lambda: F.get_piv(fr, 32, overlap=(16, 16), time=t, resolution=0.02, devices=dev), n_pairs, repeats)
        out[f"host_pairs_per_s[{name}]"] = round(rate, 1)
        out[f"host_stats[{name}]"] = st
    out["host_ratio_00_vs_none"] = round(out["host_pairs_per_s[0,0]"] / out["host_pairs_per_s[none]"], 3)

    # 2. the lazy project_hip hand-off: uint8 camera blocks of 20 frames loaded, projected on the device
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import lazy_doubles

    sys.modules["xarray"] = lazy_doubles
    src, dst = (1080, 1920), (1080, 1920)
    maps = projection_maps(src, dst, tilt=0.1, seed=2)
    cam = particle_stack(n_pairs + 1, src[0], src[1], seed=8)

    def lazy_run(dev):
        stack = lazy_doubles.frames_project(lazy_doubles.from_frames(cam, block=20), maps, dst, plugin.project_hip)
        return F.get_piv(stack, 32, overlap=(16, 16), time=t, resolution=0.02, devices=dev)

    for name, dev in modes.items():
        rate, st = best_rate(lambda: lazy_run(dev), n_pairs, repeats)
        out[f"lazy_pairs_per_s[{name}]"] = round(rate, 1)
        out[f"lazy_stats[{name}]"] = st
    out["lazy_ratio_00_vs_none"] = round(out["lazy_pairs_per_s[0,0]"] / out["lazy_pairs_per_s[none]"], 3)

    # 3. the reduction of two 1080p 64 x 64 @ 75 % ensemble states
    hs = [piv.Ensemble((1080, 1920), (64, 64), (48, 48)) for _ in range(2)]
    try:
        for k, h in enumerate(hs):
            h.accumulate(fr[4 * k:4 * k + 5], 0.2, 3.0)
        out["allreduce_state_mb"] = round(hs[0].n_rows * hs[0].n_cols * (64 * 64 + 1) * 4 / 1e6, 1)
        dev_ms, host_ms = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            piv.ensemble_allreduce(hs)
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            states = [h.export_state() for h in hs]
            s = states[0][0] + states[1][0]
            c = states[0][1] + states[1][1]
            for h in hs:
                h.import_state(s, c)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        out["allreduce_ms"] = round(min(dev_ms), 3)
        out["export_numpy_import_ms"] = round(min(host_ms), 3)
    finally:
        for h in hs:
            h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
