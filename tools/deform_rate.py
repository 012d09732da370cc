#!/usr/bin/env python
"""Rate of the window deformation passes in one session on one box.

1080p uint8, PAIRS pairs resident in HBM (lspiv_synth_particles_dev), overlap 50 % in every pass.  The chains 64 -> 32 and 64 -> 32 -> 16
with no and with one deformation pass, each whole call between two events on the library's stream.  Per final size (32, 16): the
predictor, one deformation pass as a call (warp + mixed-type kernel + rescue pass + node add, batch by batch) with the rescue pass on
and off -- their difference is the rescue pass --, the mixed-type kernel alone summed over the call's batches (the library's events
around the PIV kernel, "time_kernel"), and against it the shifted kernel of the same size in the same session.  The warp has no entry
point of its own: "warp_and_add_ms" is the call without the rescue pass minus the mixed-type kernel (the node add is one float32 per
result).  Usage: deform_rate.py [PAIRS [STEPS]] (default 200 pairs, 8 timed launches after 3 warm-ups).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from pyorc_amd import _lib, window  # noqa: E402
from pyorc_amd.device import DeviceFrames  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
T, H, W, WARMUP = PAIRS + 1, 1080, 1920, 3
CHAINS = ([(64, 32), (32, 16)], [(64, 32), (32, 16), (16, 8)])


def stats(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def kernel_ms(lib, call):
    """PIV-kernel time of ONE `call`, summed over its launches (the "time_kernel" ring holds 16: a call runs at most that many batches)."""
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
    grid = {n: window.get_array_shape((H, W), (n, n), (o, o)) for n, o in CHAINS[1]}
    tiles = {n: PAIRS * g[0] * g[1] for n, g in grid.items()}
    out = DeviceFrames.empty((4, 1, max(tiles.values())), np.float32)
    res = {"pairs": PAIRS, "steps": STEPS, "frame": [H, W], "windows_per_pair": {str(n): g[0] * g[1] for n, g in grid.items()},
           "batches_per_pass": -(-PAIRS // max(1, (256 << 20) // (H * W * 4)))}
    for chain in CHAINS:
        arr = (C.c_int * (4 * len(chain)))(*[q for m, ov in chain for q in (m, m, ov, ov)])
        name = "chain " + "->".join(str(m) for m, _ in chain)
        for D in (0, 1):
            run = lambda D=D: _lib.check(lib.lspiv_piv_multipass_deform_dev_at(d.c_ptr, 0, T, H, W, len(chain), arr, D, -1.0, 0, out.c_ptr, None, None, None))
            t = span_ms(lib, run)
            res[f"{name} D={D}"] = {"ms": t, "pairs_per_s": 1e3 * PAIRS / t["median"]}
        res[name + " D=1 over D=0"] = res[f"{name} D=1"]["ms"]["median"] / res[f"{name} D=0"]["ms"]["median"]
        # per kernel on the final grid of this chain: out holds the chain's result, which the predictor turns into the nodes
        n, o = chain[-1]
        _lib.check(lib.lspiv_piv_multipass_dev_at(d.c_ptr, 0, T, H, W, len(chain), arr, -1.0, 0, out.c_ptr, None, None, None))
        nodes = DeviceFrames.empty((1, 1, tiles[n] * 8), np.uint8)
        pred = lambda: _lib.check(lib.lspiv_piv_predict_deform_dev(out.c_ptr, C.c_void_p(out.ptr + 4 * tiles[n]), PAIRS, grid[n][0], grid[n][1],
                                                                   nodes.c_ptr, None))
        r = {"predictor_ms": span_ms(lib, pred)}
        res_out = DeviceFrames.empty((4, 1, tiles[n]), np.float32)
        deform = lambda: _lib.check(lib.lspiv_piv_deform_pairs_dev_at(d.c_ptr, 0, T, H, W, n, n, o, o, -1.0, 0, nodes.c_ptr, res_out.c_ptr, None, None))
        shifted = lambda: _lib.check(lib.lspiv_piv_shift_pairs_dev_at(d.c_ptr, 0, T, H, W, n, n, o, o, -1.0, 0, None, res_out.c_ptr, None, None))
        r["deform_call_ms"] = span_ms(lib, deform)
        r["shifted_call_ms"] = span_ms(lib, shifted)
        _lib.set_option("rescue", 0)
        r["deform_call_no_rescue_ms"] = span_ms(lib, deform)
        _lib.set_option("rescue", 1)
        r["rescue_ms"] = r["deform_call_ms"]["median"] - r["deform_call_no_rescue_ms"]["median"]
        _lib.set_option("time_kernel", 1)
        r["mixed_kernel_ms"] = kernel_ms(lib, deform)
        r["shifted_kernel_ms"] = kernel_ms(lib, shifted)
        _lib.set_option("time_kernel", 0)
        r["mixed_over_shifted_kernel"] = r["mixed_kernel_ms"]["median"] / r["shifted_kernel_ms"]["median"]
        r["warp_and_add_ms"] = r["deform_call_no_rescue_ms"]["median"] - r["mixed_kernel_ms"]["median"]
        r["warp_bytes_per_s"] = PAIRS * H * W * (1 + 4) / (1e-3 * r["warp_and_add_ms"])      # one byte read, one float32 written per pixel
        r["deform_call_over_shifted_call"] = r["deform_call_ms"]["median"] / r["shifted_call_ms"]["median"]
        res[f"{n}@{o}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
