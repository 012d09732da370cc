"""The "lds_light" form of the flagship 32 x 32 walking kernel (csrc/piv_fft_impl.h, LITE) without a GPU: the device compiler's own output
says what an iteration holds.  tests/native/walk_lite_count.hip instantiates the kernel (uint8, no planes, no signal score, batched fit,
un-packing through DPP) in its former form and in the new one; tools/isa_phases.py splits the loop body into its phases.

* no ds_swizzle is left in the loop body of the new form (the former has the ten of the hot path and the cold path's);
* the LDS round trips an iteration waits for (column rt) go down by at least the eight that ended in a ds_swizzle;
* the VALU count of the iteration does not go up;
* with -DLSPIV_UNPACK_GROUP=16 (not adopted: no measurable gain) the scalar instructions of the un-pack segment go down (one mask set per
  16 exchanged values instead of one per two) and the VALU count of that segment stays;
* neither form touches scratch memory in the loop."""
import functools
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "walk_lite_count.hip")
CSRC = os.path.join(ROOT, "pyorc_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "isa_phases.py")
FORMER, LIGHT = "piv_fft_walk_kernelIhLi32ELb0ELb0ELb1ELb1ELb0E", "piv_fft_walk_kernelIhLi32ELb0ELb0ELb1ELb1ELb1E"
UNPACK_SEGMENT = 4   # conversion | fft | transpose | fft | UN-PACK | fft | transpose | fft | epilogue


@functools.lru_cache(maxsize=None)
def phases(*defines):
    """{kernel: (rows per segment, totals)}, each a dict column -> count"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library: it has to be here"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "walk_lite_count.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I", CSRC, "-S", "--cuda-device-only", SRC, "-o", asm] + list(defines),
                       check=True, capture_output=True)
        for key in (FORMER, LIGHT):
            txt = subprocess.run([sys.executable, TOOL, "--asm", asm, SRC, key], check=True, capture_output=True, text=True).stdout
            print(txt)
            lines = txt.splitlines()
            cols = lines[1].split()[2:]
            segs = [dict(zip(cols, map(int, l.split()[2:]))) for l in lines[2:] if l.split()[0].isdigit()]
            tot = next(dict(zip(cols, map(int, l.split()[1:]))) for l in lines if l.split()[0] == "all")
            out[key] = (segs, tot)
    return out


def test_no_swizzle_left_in_the_loop():
    assert phases()[FORMER][1]["lds_swz"] >= 10
    assert phases()[LIGHT][1]["lds_swz"] == 0


def test_round_trips_go_down_by_those_of_the_swizzles():
    former, light = phases()[FORMER][1], phases()[LIGHT][1]
    assert light["rt"] <= former["rt"] - 8
    assert light["lds"] <= former["lds"] - 10
    assert light["waitcnt"] < former["waitcnt"]


def test_valu_count_does_not_go_up():
    assert phases()[LIGHT][1]["valu"] <= phases()[FORMER][1]["valu"]


def test_unpack_group_switch_sets_the_mask_per_group():
    ph = phases("-DLSPIV_UNPACK_GROUP=16")
    former, light = ph[FORMER][0][UNPACK_SEGMENT], ph[LIGHT][0][UNPACK_SEGMENT]
    assert former["cndmask"] == light["cndmask"] == 64, "not the un-pack segment"
    assert light["salu"] <= former["salu"] - 60
    assert light["valu"] == former["valu"]
    assert ph[LIGHT][1]["scratch"] == 0


def test_no_scratch_in_the_loop():
    assert phases()[FORMER][1]["scratch"] == 0 and phases()[LIGHT][1]["scratch"] == 0
