#!/usr/bin/env python
"""Rate of the lag kernels in one session on one box.

1080p uint8 resident in HBM (lspiv_synth_particles_dev), PAIRS pairs plus a halo of 8 frames, overlap 50 %, windows 16 / 32 / 64.  Per
size, the PIV kernel alone (the library's events around it, "time_kernel": no rescue pass, no copies) for three tables -- all ones, all
4, and the table and offsets the predictor makes of a river profile (u(y) = 0.15 + 2.4 smoothstep px/frame over the frame's height, K = 8,
the quarter rule: lags 1 .. 8 in bands, offsets up to a quarter window) -- and, in the same session, the shifted kernel at zero offsets
(one window per job, the same job but for the address of window B: its instructions are those of the commit before the lag kernels,
checked by diffing the gfx950 assembly).  Also: the predictor alone and the lagged call as a whole (table, kernel, rescue pass, division)
by the host clock around synchronised calls -- launch overheads included, so upper bounds for those two small kernels.  No ratio is fixed
in advance.  Usage: lag_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed launches after 3 warm-ups).  Prints one JSON line.

The small kernels on their own: run this tool under `rocprofv3 --kernel-trace -d DIR -o lag -- python tools/lag_rate.py`, then
`lag_rate.py --trace DIR/lag_results.db` prints the durations of lag_fill_kernel, lag_divide_kernel and lag_predict_kernel per grid size
from the trace (and, with a `--pmc` run's database and the launches per timed block, `--trace DB 5` for STEPS = 2, the mean of every counter per
block of launches of the PIV kernels, in launch order: shifted, shifted, ones, fours, profile, shifted, fours, shifted per size)."""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "--trace" else 200
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] != "--trace" else 8
H, W, WARMUP, HALO = 1080, 1920, 3, 8
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


def wall_ms(lib, call):
    """Host clock around ONE synchronised `call`."""
    for _ in range(WARMUP):
        call()
    out = []
    for _ in range(STEPS):
        _lib.check(lib.lspiv_synchronize())
        t0 = time.perf_counter()
        call()
        _lib.check(lib.lspiv_synchronize())
        out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def ratio(a, b):
    """median / median, and the range the two min - max spans allow"""
    return {"median": a["median"] / b["median"], "min": a["min"] / b["max"], "max": a["max"] / b["min"]}


def profile_field(rows, cols, n, o):
    """(u, v) (PAIRS, rows, cols) float32 of the river profile at the window centres."""
    y = np.arange(rows) * (n - o) + (n - 1) / 2.0
    s = np.clip((y - 0.375 * H) / (0.5 * H), 0.0, 1.0)
    u = (0.15 + 2.4 * s * s * (3.0 - 2.0 * s)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(u[None, :, None], (PAIRS, rows, cols))), np.zeros((PAIRS, rows, cols), np.float32)


def trace_summary(path, per_block=0):
    """Per (kernel, grid size): launches and the median (min - max) duration in microseconds of the small kernels of a kernel trace; per
    block of consecutive launches of one PIV kernel: the mean of every counter a --pmc run collected."""
    import sqlite3

    c = sqlite3.connect(path)
    small, out = {}, {"small_kernels_us": {}, "piv_blocks": []}
    tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
    for name, start, end, grid in (c.execute("select name, start, end, grid_x from kernels order by start") if "kernels" in tables else ()):
        for key in ("lag_fill_kernel", "lag_divide_kernel", "lag_predict_kernel"):
            if key in name:
                small.setdefault(f"{key} x {grid // 256} blocks", []).append((end - start) / 1e3)
    for key, v in sorted(small.items()):
        out["small_kernels_us"][key] = dict(stats(v), launches=len(v))
    if "counters_collection" in tables:   # (per_block: launches per timed block, WARMUP + STEPS -- the three tables run back to back)
        blocks = []
        for name, disp, counter, value in c.execute("select kernel_name, dispatch_id, counter_name, sum(value) from counters_collection "
                                                    "group by dispatch_id, counter_name order by dispatch_id"):
            if "piv_fft_lag_kernel" not in name and "piv_fft_shift_kernel" not in name:
                continue
            short = name.split("(")[0].split("::")[-1]
            if not blocks or blocks[-1]["kernel"] != short or (per_block and disp not in blocks[-1]["launches"] and len(blocks[-1]["launches"]) == per_block):
                blocks.append({"kernel": short, "launches": set(), "sums": {}})
            blocks[-1]["launches"].add(disp)
            blocks[-1]["sums"][counter] = blocks[-1]["sums"].get(counter, 0.0) + value
        for b in blocks:
            n = len(b["launches"])
            out["piv_blocks"].append({"kernel": b["kernel"], "launches": n, **{k: v / n for k, v in sorted(b["sums"].items())}})
    print(json.dumps(out))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return trace_summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    lib = _lib.load()
    _lib.require_device()
    T = PAIRS + HALO
    d = DeviceFrames.empty((T, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261021, 0.02))
    res = {"pairs": PAIRS, "halo": HALO, "steps": STEPS, "frame": [H, W]}
    _lib.set_option("time_kernel", 1)
    try:
        for n, o in SIZES:
            rows, cols = window.get_array_shape((H, W), (n, n), (o, o))
            n_win = rows * cols
            out = DeviceFrames.empty((4, PAIRS, n_win), np.float32)
            lag_out = DeviceFrames.empty((1, PAIRS, n_win), np.uint8)
            table = DeviceFrames.empty((1, PAIRS, n_win), np.uint8)
            shift = DeviceFrames.empty((PAIRS, n_win, 4), np.uint8)      # (int16 {dy, dx} per window and pair)
            u, v = profile_field(rows, cols, n, o)
            d_uv = DeviceFrames.empty((2, PAIRS, n_win), np.float32)
            _lib.check(lib.lspiv_memcpy_h2d(d_uv.c_ptr, _lib.ptr(u), u.nbytes))
            _lib.check(lib.lspiv_memcpy_h2d(C.c_void_p(d_uv.ptr + u.nbytes), _lib.ptr(v), v.nbytes))
            predict = lambda: _lib.check(lib.lspiv_lag_predict_dev(d_uv.c_ptr, C.c_void_p(d_uv.ptr + u.nbytes), PAIRS, T, H, W, n, n, o, o, HALO,
                                                                   32 * n, table.c_ptr, shift.c_ptr, None))

            def lagged(form, k, lag=None, sh=None):
                return lambda: _lib.check(lib.lspiv_piv_lag_pairs_dev_at(d.c_ptr, 0, T, PAIRS, H, W, n, n, o, o, -1.0, 0, form, k, 0, lag, sh,
                                                                         out.c_ptr, None, lag_out.c_ptr, None, None))

            shifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, PAIRS + 1, H, W, n, n, o, o, -1.0, 0, None, out.c_ptr, None, None))
            r = {"windows_per_pair": n_win, "predict_wall_ms": wall_ms(lib, predict)}
            lags = np.bincount(table.to_host().reshape(-1), minlength=HALO + 1)[1:]
            r["profile_lag_shares"] = [round(float(x), 4) for x in lags / lags.sum()]
            cases = {"ones": lagged(window.LAG_UNIFORM, 1), "fours": lagged(window.LAG_UNIFORM, 4),
                     "profile": lagged(window.LAG_TABLE, 0, table.c_ptr, shift.c_ptr)}
            r["first_block_ms"] = kernel_ms(lib, shifted)            # (the first timed block of a size runs on clocks still ramping: reported, not used)
            r["shifted_kernel_ms"] = kernel_ms(lib, shifted)
            for name, call in cases.items():
                r[f"{name}_kernel_ms"] = kernel_ms(lib, call)
            r["shifted_again_ms"] = kernel_ms(lib, shifted)          # the order of the launches is no part of a ratio
            for name in cases:
                r[f"{name}_over_shifted"] = ratio(r[f"{name}_kernel_ms"], r["shifted_kernel_ms"])
                r[f"{name}_over_shifted_again"] = ratio(r[f"{name}_kernel_ms"], r["shifted_again_ms"])
            r["fours_call_wall_ms"] = wall_ms(lib, cases["fours"])    # table + kernel + rescue pass + division, and their launches
            r["shifted_call_wall_ms"] = wall_ms(lib, shifted)         # kernel + rescue pass (no offsets: no add step)
            r["fours_pairs_per_s"] = 1e3 * PAIRS / r["fours_kernel_ms"]["median"]
            del out, lag_out, table, shift, d_uv
            res[f"{n}@{o}"] = r
    finally:
        _lib.set_option("time_kernel", 0)
        _lib.check(lib.lspiv_synchronize())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
