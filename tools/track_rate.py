#!/usr/bin/env python
"""Rate of the point tracker's kernels, in one session on one box.

1080p uint8 frames resident in HBM (lspiv_synth_particles_dev), PAIRS pairs, the points on the centres of the 32 @ 16 PIV grid (7 854 per
pair), levels = 3, eps = 0.01, max_iter = 20, for w = 21, 9 and 31.  Every step puts two events on the library's stream around ONE entry
point: lspiv_pyr_down_dev for each of the two pyramid steps (one launch of pyr_down_kernel each: uint8 -> level 1, level 1 -> level 2),
and lspiv_lk_track_dev, which is those two launches and ONE launch of lk_track_kernel when the pyramid of all pairs fits the workspace
(it does here: 0.52 GB of 1 GiB); "lk_kernel_ms" is that span less the two pyramid launches timed in the same session, step by step.
Beside them the per-pair PIV kernel (option walk = 0) at 32 @ 16 on the same stack.  No figure is fixed in advance.

Usage: track_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed steps after 3 warm-ups); track_rate.py --resources compiles
csrc/track.hip only (no GPU needed) and prints VGPRs / scratch / occupancy of every variant.  Prints one JSON line."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyorc_amd import _lib, track, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

H, W, WARMUP, LEVELS, WINDOWS = 1080, 1920, 3, 3, (21, 9, 31)


def resources():
    """{(dtype, w): {vgpr, scratch, occupancy}} of lk_track_kernel and pyr_down_kernel from the compiler's resource-usage remarks."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize", "-c",
               os.path.join(ROOT, "pyorc_amd", "csrc", "track.hip"), "-o", os.path.join(tmp, "track.o"), "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True).stderr
    res = {}
    for block in out.split("Function Name: ")[1:]:
        name = block.split()[0]
        m = re.search(r"lk_track_kernelI([hf])Li(\d+)E", name)
        key = f"lk_track_kernel<{'uint8' if m.group(1) == 'h' else 'float32'}, {m.group(2)}>" if m else \
            f"pyr_down_kernel<{'uint8' if 'kernelIh' in name else 'float32'}>"
        get = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))  # noqa: E731
        res[key] = {"vgpr": get(r" VGPRs"), "agpr": get(r"AGPRs"), "scratch_bytes_per_lane": get(r"ScratchSize \[bytes/lane\]"),
                    "occupancy_waves_per_simd": get(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": get(r"LDS Size \[bytes/block\]")}
    return res


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def main():
    if "--resources" in sys.argv:
        print(json.dumps(resources()))
        return
    args = [int(a) for a in sys.argv[1:]]
    pairs, steps = (args + [200, 8][len(args):])[:2]
    lib = _lib.load()
    _lib.require_device()
    T = pairs + 1
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))

    def timed(call):
        spans = []
        for step in range(WARMUP + steps):
            _lib.check(lib.lspiv_event_record(e0))
            call()
            _lib.check(lib.lspiv_event_record(e1))
            _lib.check(lib.lspiv_synchronize())
            span = C.c_float(0)
            _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(span)))
            if step >= WARMUP:
                spans.append(span.value)
        return np.asarray(spans)

    x, y = window.get_rect_coordinates((H, W), (32, 32), (16, 16))
    xx, yy = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    pts = np.ascontiguousarray(np.stack([xx.ravel(), yy.ravel()], axis=1))
    N = len(pts)
    res = {"pairs": pairs, "steps": steps, "frame": [H, W], "points_per_pair": N, "levels": LEVELS, "eps": 0.01, "max_iter": 20}
    try:
        d = DeviceFrames.empty((T, H, W), np.uint8)
        _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261021, 0.02))
        shapes = track.level_shapes(H, W, LEVELS)
        l1, l2 = (DeviceFrames.empty((T,) + s, np.float32) for s in shapes[1:])
        p1 = timed(lambda: _lib.check(lib.lspiv_pyr_down_dev(d.c_ptr, 0, T, H, W, l1.c_ptr, None)))
        p2 = timed(lambda: _lib.check(lib.lspiv_pyr_down_dev(l1.c_ptr, 1, T, *shapes[1], l2.c_ptr, None)))
        res["pyr_down_u8_ms"], res["pyr_down_f32_ms"] = stats(p1), stats(p2)
        res["pyr_down_G_samples_out_per_s"] = T * (shapes[1][0] * shapes[1][1]) / (np.median(p1) * 1e-3) / 1e9
        del l1, l2
        d_pts = DeviceFrames.empty((1, 1, pts.nbytes), np.uint8)
        _lib.check(lib.lspiv_memcpy_h2d(d_pts.c_ptr, _lib.ptr(pts), pts.nbytes))
        out = [DeviceFrames.empty((1, 1, pairs * N * b), np.uint8) for b in (8, 8, 8, 8, 4, 1)]
        for w in WINDOWS:
            ms = timed(lambda: _lib.check(lib.lspiv_lk_track_dev(d.c_ptr, 0, T, H, W, d_pts.c_ptr, N, 0, None, 0, w, LEVELS, 20, 0.01, 0.0, 0,
                                                                 *(q.c_ptr for q in out), None, None)))
            n_iter = np.empty(pairs * N, dtype=np.int32)
            status = np.empty(pairs * N, dtype=np.uint8)
            _lib.check(lib.lspiv_memcpy_d2h(_lib.ptr(n_iter), out[4].c_ptr, n_iter.nbytes))
            _lib.check(lib.lspiv_memcpy_d2h(_lib.ptr(status), out[5].c_ptr, status.nbytes))
            kernel = ms - np.median(p1) - np.median(p2)
            res[f"w{w}"] = {"track_ms": stats(ms), "lk_kernel_ms": stats(kernel), "point_pairs_per_s": pairs * N / (np.median(kernel) * 1e-3),
                            "mean_n_iter": float(n_iter.mean()), "status_counts": np.bincount(status, minlength=6).tolist()}
        # the yardstick: the per-pair PIV kernel at 32 @ 16 on the same stack
        _lib.set_option("walk", 0)
        n_rows, n_cols = window.get_array_shape((H, W), (32, 32), (16, 16))
        piv_out = DeviceFrames.empty((1, 1, 4 * pairs * n_rows * n_cols * 4), np.uint8)
        pm = timed(lambda: _lib.check(lib.lspiv_piv_pairs_dev(d.c_ptr, 0, T, H, W, 32, 32, 16, 16, -1.0, piv_out.c_ptr, None, None)))
        _lib.set_option("walk", -1)
        res["piv_walk0_32at16_ms"] = stats(pm)
        res["piv_windows_per_s"] = pairs * n_rows * n_cols / (np.median(pm) * 1e-3)
    finally:
        _lib.check(lib.lspiv_synchronize())
        lib.lspiv_event_destroy(e0)
        lib.lspiv_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
