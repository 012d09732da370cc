"""The "scalar_epilogue" form of the flagship 32 x 32 walking kernel (csrc/piv_fft_impl.h, SCAL) without a GPU: the device compiler's own
output says what an iteration holds.  tests/native/walk_scalar_count.hip instantiates the kernel (uint8, no planes, no signal score,
batched fit, un-packing through DPP, lane-swap reductions) in its former form and in the new one; tools/isa_phases.py splits the loop
body into its phases.  Every threshold is what the former form measures in the same compilation:

* the new form's loop body has fewer VALU instructions, in total and in the epilogue segment (the first-match searches, the near-tie
  test, the neighbour indices and the record word left the vector unit), and more scalar ones (they went to the scalar unit);
* no more LDS instructions, no more s_waitcnt, no scratch in the loop and none in the kernel;
* no VGPR above the three-wave step of 168;
* the un-pack segment keeps its VALU count although the plane means no longer go through ds_bpermute (two LDS instructions fewer)."""
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "walk_scalar_count.hip")
CSRC = os.path.join(ROOT, "pyorc_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "isa_phases.py")
FORMER, SCALAR = "piv_fft_walk_kernelIhLi32ELb0ELb0ELb1ELb1ELb1ELb0E", "piv_fft_walk_kernelIhLi32ELb0ELb0ELb1ELb1ELb1ELb1E"
UNPACK_SEGMENT, EPILOGUE_SEGMENT = 4, 8   # conversion | fft | transpose | fft | UN-PACK | fft | transpose | fft | EPILOGUE
VGPR_STEP = 168                            # three waves per SIMD


@functools.lru_cache(maxsize=None)
def compiled():
    """{kernel: (rows per segment, totals, resource metadata)}"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library: it has to be here"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "walk_scalar_count.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I", CSRC, "-S", "--cuda-device-only", SRC, "-o", asm],
                       check=True, capture_output=True)
        text = open(asm).read()
        for key in (FORMER, SCALAR):
            txt = subprocess.run([sys.executable, TOOL, "--asm", asm, SRC, key], check=True, capture_output=True, text=True).stdout
            print(txt)
            lines = txt.splitlines()
            cols = lines[1].split()[2:]
            segs = [dict(zip(cols, map(int, l.split()[2:]))) for l in lines[2:] if l.split()[0].isdigit()]
            tot = next(dict(zip(cols, map(int, l.split()[1:]))) for l in lines if l.split()[0] == "all")
            meta = re.search(r"\.name:\s+_ZN5lspiv19" + key + r"\w*\n(.*?)\.wavefront_size:", text, re.S).group(1)
            res = {k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}
            print(key, res)
            out[key] = (segs, tot, res)
    return out


def test_it_is_the_epilogue_segment():
    for key in (FORMER, SCALAR):
        segs = compiled()[key][0]
        assert len(segs) == 9
        assert segs[UNPACK_SEGMENT]["cndmask"] == 64, "not the un-pack segment"
        assert segs[EPILOGUE_SEGMENT]["trans"] >= 8 and segs[EPILOGUE_SEGMENT]["arith_f32"] < 100, "not the epilogue segment"


def test_fewer_valu_in_total_and_in_the_epilogue():
    former, scalar = compiled()[FORMER], compiled()[SCALAR]
    assert scalar[1]["valu"] < former[1]["valu"]
    assert scalar[0][EPILOGUE_SEGMENT]["valu"] < former[0][EPILOGUE_SEGMENT]["valu"]
    # what left the vector unit is DPP steps, selects and integer arithmetic; the transforms keep theirs
    assert scalar[0][EPILOGUE_SEGMENT]["dpp"] < former[0][EPILOGUE_SEGMENT]["dpp"]
    assert scalar[1]["arith_f32"] == former[1]["arith_f32"]
    assert scalar[1]["salu"] > former[1]["salu"]


def test_no_more_lds_instructions_waits_or_scratch():
    former, scalar = compiled()[FORMER], compiled()[SCALAR]
    assert scalar[1]["lds"] <= former[1]["lds"]
    assert scalar[1]["waitcnt"] <= former[1]["waitcnt"]
    assert scalar[1]["scratch"] == 0 and former[1]["scratch"] == 0
    assert scalar[2]["private_segment_fixed_size"] == 0


def test_vgprs_stay_inside_the_three_wave_step():
    assert compiled()[SCALAR][2]["vgpr_count"] <= VGPR_STEP
    assert compiled()[FORMER][2]["vgpr_count"] <= VGPR_STEP


def test_plane_means_without_bpermute_cost_the_unpack_segment_no_valu():
    former, scalar = compiled()[FORMER][0][UNPACK_SEGMENT], compiled()[SCALAR][0][UNPACK_SEGMENT]
    assert scalar["lds_perm"] == former["lds_perm"] - 2
    assert scalar["valu"] <= former["valu"]
