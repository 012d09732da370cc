#!/usr/bin/env python
"""Rate of the two STIV kernels, in one session on one box.

1080p frames resident in HBM (lspiv_synth_particles_dev; float32: the same stack through filters.smooth), FRAMES frames, LINES search
lines of SAMPLES samples laid across a transect from bank to bank, 0.1 rad off the image rows, 1.5 px between samples.  Every step puts two
events on the library's stream around ONE entry point: lspiv_sti_gather_dev (the host prepares the sample table and queues its upload,
then one kernel launch: the span holds the table's copy and the kernel) and lspiv_sti_orientation_dev (one kernel launch, nothing else)
for one window over all frames and for windows of a quarter of the frames at half-window stride.  Requests: the gather makes
4 x FRAMES x LINES x SAMPLES loads of 1 (uint8) or 4 (float32) bytes and writes FRAMES x LINES x SAMPLES floats; the figure
"gather_G_samples_per_s" is samples over the median span.  No figure is fixed in advance.
Usage: stiv_rate.py [FRAMES [STEPS [LINES [SAMPLES]]]] (default 1000 frames, 8 timed steps after 3 warm-ups, 200 lines of 256 samples).
Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyorc_amd import _lib, filters, stiv  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

ARGS = [int(a) for a in sys.argv[1:]]
FRAMES, STEPS, LINES, SAMPLES = (ARGS + [1000, 8, 200, 256][len(ARGS):])[:4]
STEPS = max(3, STEPS)
H, W, WARMUP = 1080, 1920, 3


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def main():
    lib = _lib.load()
    _lib.require_device()
    T, S, L = FRAMES, LINES, SAMPLES
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.lspiv_event_create(C.byref(e0)))
    _lib.check(lib.lspiv_event_create(C.byref(e1)))

    def timed(call):
        spans = []
        for step in range(WARMUP + STEPS):
            _lib.check(lib.lspiv_event_record(e0))
            call()
            _lib.check(lib.lspiv_event_record(e1))
            _lib.check(lib.lspiv_synchronize())
            span = C.c_float(0)
            _lib.check(lib.lspiv_event_elapsed_ms(e0, e1, C.byref(span)))
            if step >= WARMUP:
                spans.append(span.value)
        return np.asarray(spans)

    length = 1.5 * (L - 1)
    transect = np.stack([np.full(S, W / 2.0), np.linspace(40.0, H - 41.0, S)], axis=1)
    lines = stiv.lines_across(transect, length, direction=0.1)
    pts = np.ascontiguousarray(stiv.line_points(lines, L))
    res = {"frames": T, "steps": STEPS, "frame": [H, W], "lines": S, "samples": L, "ds_px": float(stiv.line_spacing(lines, L)[0])}
    tw = max(T // 4, 5)
    windows = {"one_window": (T, T), "quarter_windows": (tw, max(tw // 2, 1))}
    try:
        for dtype in (np.uint8, np.float32):
            d = DeviceFrames.empty((T, H, W), np.uint8)
            _lib.check(lib.lspiv_synth_particles_dev(d.c_ptr, T, H, W, 20261021, 0.02))
            if dtype == np.float32:
                d = filters.smooth(d, 1)
            sti = DeviceFrames.empty((S, T, L), np.float32)
            code = d.dtype_code
            ms = timed(lambda: _lib.check(lib.lspiv_sti_gather_dev(d.c_ptr, code, T, H, W, _lib.ptr(pts), S, L, sti.c_ptr, 0, T, None)))
            r = {"gather_ms": stats(ms), "gather_G_samples_per_s": T * S * L / (np.median(ms) * 1e-3) / 1e9}
            if dtype == np.uint8:     # the orientation reads the space-time images, whatever the frames were
                for name, (Tw, stride) in windows.items():
                    K = (T - Tw) // stride + 1
                    out = [DeviceFrames.empty((1, 1, S * K * n * 8), np.uint8) for n in (3, 1, 1)]
                    for smooth in (0, 1, 3):
                        oms = timed(lambda: _lib.check(lib.lspiv_sti_orientation_dev(sti.c_ptr, S, T, L, Tw, stride, smooth, 1, out[0].c_ptr,
                                                                                     out[1].c_ptr, out[2].c_ptr, None)))
                        r[f"orientation_{name}_smooth{smooth}_ms"] = stats(oms)
                    r[f"orientation_{name}"] = {"time_window": Tw, "time_stride": stride, "windows": K}
            res[np.dtype(dtype).name] = r
            del d, sti
    finally:
        _lib.check(lib.lspiv_synchronize())
        lib.lspiv_event_destroy(e0)
        lib.lspiv_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
