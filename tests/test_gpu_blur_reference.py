"""The five kernel families of smooth / edge_detect (launch_blur_clip in pyorc_amd/csrc/filters.hip) against the float64 reference of
tests/blur_ref.py: every result must have the reference's NaN, +Inf and -Inf masks and lie within the DERIVED gate of it on the finite
outputs (blur_ref's docstring: (2 (R + 2) + 2) u max|x| for smooth, equality for uint8 at windows <= 3), the host and the device entry
must give the same bits, and every case asserts through blur_ref.family that it reaches the kernel it is meant for.  The shapes are the
smallest at which each kernel can still go wrong (blur_ref.TABLE says what each reaches).

Largest error / gate measured on an MI355X over all tests of this file: 0.205 (float64 frames, T = 3 stack; each test prints its own;
the project's float32 oracle uses 0.223 on the same stacks, tests/test_blur_ref_host.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import blur_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
INF = float("inf")


def _run(fr, w):
    """filters.smooth / edge_detect on the host stack and (uint8, float32) on the device-resident one: the same bits."""
    from pyorc_amd import DeviceFrames, filters

    w1, w2 = br.split(w)
    call = (lambda f: filters.smooth(f, w1)) if w2 is None else (lambda f: filters.edge_detect(f, w1, w2))
    got = call(fr)
    assert got.dtype == np.float32 and got.shape == fr.shape
    if fr.dtype != np.float64:                                          # float64 stacks have no device-resident form
        dev = call(DeviceFrames.from_host(fr)).to_host()
        assert np.array_equal(dev.view(np.uint32), got.view(np.uint32)), ("host and device entries differ", fr.shape, fr.dtype, w)
    return got


def _check(kind, key, dt, w, fam):
    fr = br.STACKS[kind](key, dt)
    assert br.family(dt, *br.split(w), fr.shape[2]) == fam, (key, dt, w)
    masks, ratio = br.compare(_run(fr, w), br.reference(kind, key, dt, w), fr, w)
    assert masks, ("NaN / Inf masks differ from the reference's", kind, key, dt, w)
    assert ratio <= 1.0, ("error / gate", ratio, kind, key, dt, w)
    return ratio


CASES = [(row, shape) for row, (_, shapes) in br.TABLE.items() for shape, _ in shapes]


@pytest.mark.parametrize("row,shape", CASES, ids=[f"{r}-{'x'.join(map(str, s))}" for r, s in CASES])
def test_gpu_blur_families_against_the_float64_reference(gpu, row, shape):
    windows, shapes = br.TABLE[row]
    worst = max(_check("table", shape, dt, w, fam) for dt in dict(shapes)[shape] for w, fam in windows.items())
    print(f"{row} {shape}: largest error / gate = {worst:.3f}")


@pytest.mark.parametrize("row", ["strip", "stripr", "ring"])
@pytest.mark.parametrize("dt", br.F)
def test_gpu_blur_nan_and_inf_samples_reach_exactly_the_references_outputs(gpu, row, dt):
    """NaN in the interior, within R of a corner, in the halo rows between two strips and the halo columns between two tiles, +Inf and
    -Inf apart from them: a row pass, a halo or a reflect101 that let a sample in or out wrongly changes a mask."""
    worst = max(_check("nonfinite", row, dt, w, fam) for w, fam in br.TABLE[row][0].items())
    print(f"{row} {dt}: largest error / gate = {worst:.3f}")


@pytest.mark.parametrize("dt,row,w", [("float32", "strip", (1, 2)), ("uint8", "strip4", (2, 3)), ("float32", "stripr", (2, 4)),
                                      ("float32", "stripr", (6, 10)), ("float32", "ring", (11, 15)), ("uint8", "ring", (3, 12))])
def test_gpu_edge_detect_clip_in_the_store_against_the_clipped_reference(gpu, dt, row, w):
    from pyorc_amd import DeviceFrames, _lib

    kind, key = ("frames", None) if dt == "uint8" else ("nonfinite", row)
    fr = br.STACKS[kind](key, dt)
    T, H, W = fr.shape
    assert br.family(dt, w[0], w[1], W) == br.TABLE[row][0][w]
    d, worst = DeviceFrames.from_host(fr), 0.0
    for lo, hi in ((-5.0, 5.0), (-INF, 0.25), (0.0, INF), (-INF, INF)):
        out = DeviceFrames.empty((T, H, W), np.float32)
        _lib.check(gpu.lspiv_edge_detect_clip_dev(d.c_ptr, d.dtype_code, T, H, W, 2 * w[0] + 1, 2 * w[1] + 1, lo, hi, out.c_ptr, None))
        masks, ratio = br.compare(out.to_host(), br.reference(kind, key, dt, w, lo, hi), fr, w)
        assert masks and ratio <= 1.0, (lo, hi, masks, ratio)
        worst = max(worst, ratio)
    print(f"clip {row} {dt} {w}: largest error / gate = {worst:.3f}")


@pytest.mark.parametrize("dt", br.F + br.U8)
def test_gpu_blur_of_several_frames_with_a_constant_per_frame(gpu, dt):
    fam = {2: "strip4" if dt == "uint8" else "strip", (2, 3): "strip4" if dt == "uint8" else "strip", 4: "stripr5", (6, 10): "stripr10",
           12: "ring", (11, 15): "ring"}
    worst = max(_check("frames", None, dt, w, f) for w, f in fam.items())
    print(f"frames {dt}: largest error / gate = {worst:.3f}")


@pytest.mark.parametrize("switch,mode", [("LSPIV_BLUR_BLOCK", "runtime"), ("LSPIV_BLUR_RING", "runtime"), ("LSPIV_BLUR_ONE_COLUMN", "unrolled")])
def test_gpu_blur_kernels_behind_the_ab_switches_against_the_reference(gpu, switch, mode):
    """The tile-per-block kernel, the LDS-ring kernel at windows 4 .. 10 and the one-column kernel on uint8 widths of the four-column
    one, each in a fresh process with its switch set: a comparison against a broken alternative is worthless."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSPIV_BLUR_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blur_ab_worker.py"), mode], capture_output=True, text=True, cwd=ROOT,
                         env=dict(env, **{switch: "1"}))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"{switch}: {res['n']} results, largest error / gate = {res['worst']:.3f}")
    assert res["n"] >= (200 if mode == "runtime" else 36) and res["failed"] == [] and res["worst"] <= 1.0, res["failed"][:10]
