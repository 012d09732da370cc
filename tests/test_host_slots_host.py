"""The slot layout of the host twins' staged call (csrc/host_slots.h, used by HostCall in csrc/api_internal.h) without a GPU: a small
program with its own main (tests/native/slot_layout_host.cpp) is built with AddressSanitizer and UndefinedBehaviorSanitizer by the host
compiler and run.  It checks mixed sizes (0, absent entries, sizes that are no multiple of the alignment): every offset aligned, no two
slots overlapping, absent entries taking no room, and the total -- what the workspace is sized to -- holding every slot to its last byte.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "slot_layout_host.cpp")
CSRC = os.path.join(ROOT, "pyorc_amd", "csrc")


def test_slot_layout_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "the host compiler that builds host_stage.cpp has to be here"
    exe = str(tmp_path / "slot_layout_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr
