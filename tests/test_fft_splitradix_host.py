"""Conjugate-pair split-radix register FFTs (csrc/fft_regs.h, fft_sr / LSPIV_FFT_SR) without a GPU: the templates are __host__ __device__,
so a small program (tests/native/fft_forms_host.hip) runs them on the CPU, and the device compiler's own output says what they cost.

* lengths 16 / 32 / 64, forward and inverse, on 200 seeded rows plus every unit impulse and a constant row, against numpy.fft in complex128:
  the worst error relative to the row's largest bin may not exceed 1.5 x that of the un-folded radix-4 x 8 form ON THE SAME ROWS -- the
  yardstick and the factor of tests/test_gpu_fft_fold.py, which the GPU test of the split-radix form uses as well;
* compile only (hipcc -S --cuda-device-only): the float32 arithmetic of a kernel that holds nothing else is 144 / 372 / 912 instructions,
  none of them a v_mul_f32 or a v_fma_f32 of three vector registers, and the clip of the clamped inverse rides on the last instruction
  (there the FMA takes its VOP3 form for the clamp bit, with the constant in a scalar register).
"""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fft_forms_host.hip")
CSRC = os.path.join(ROOT, "pyorc_amd", "csrc")
FACTOR = 1.5          # tests/test_gpu_fft_fold.py: a form may be no worse than 1.5 x the un-folded one
COUNTS = {16: 144, 32: 372, 64: 912}


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(exe), "hipcc is what builds the library: it has to be here"
    return exe


def _flags():
    return ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I", CSRC]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fft_forms") / "fft_forms_host")
    subprocess.run([_hipcc()] + _flags() + [SRC, "-o", exe], check=True, capture_output=True)
    return exe


@functools.lru_cache(maxsize=None)
def rows(n):
    rng = np.random.default_rng(20261020 + n)
    z = np.zeros((n + 1 + 200, n), np.complex128)
    z[np.arange(n), np.arange(n)] = 1.0
    z[n] = 1.0
    z[n + 1:] = rng.uniform(-1, 1, (200, n)) + 1j * rng.uniform(-1, 1, (200, n))
    z = z.astype(np.complex64)
    z.setflags(write=False)
    return z


def run_form(program, tmp_path, z, form, inverse):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / f"out{form}.bin")
    np.ascontiguousarray(z).tofile(fin)
    subprocess.run([program, str(z.shape[1]), str(int(inverse)), str(form), fin, fout], check=True, capture_output=True)
    return np.fromfile(fout, np.complex64).reshape(z.shape)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_split_radix_rows_on_the_host(program, tmp_path, n, inverse):
    z = rows(n)
    z128 = z.astype(np.complex128)
    ref = np.fft.ifft(z128, axis=1) * n if inverse else np.fft.fft(z128, axis=1)
    scale = np.abs(ref).max(axis=1, keepdims=True)
    fig = {}
    for form in (1, 2, 4):
        e = np.abs(run_form(program, tmp_path, z, form, inverse).astype(np.complex128) - ref) / scale
        fig[form] = (float(e.max()), float(np.sqrt((e * e).mean())))
    print(f"n={n} inverse={inverse}: " + "; ".join(f"{name} max {fig[f][0]:.3e} rms {fig[f][1]:.3e}" for f, name in ((1, "un-folded"), (2, "folded"), (4, "split radix"))))
    assert fig[4][0] <= FACTOR * fig[1][0]
    assert fig[4][1] <= FACTOR * fig[1][1]


def test_program_rejects_a_form_it_does_not_have(program, tmp_path):
    fin = str(tmp_path / "in.bin")
    np.zeros((1, 16), np.complex64).tofile(fin)
    assert subprocess.run([program, "16", "0", "3", fin, str(tmp_path / "o.bin")], capture_output=True).returncode == 2


@functools.lru_cache(maxsize=None)
def _device_asm():
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fft_forms.s")
        subprocess.run([_hipcc()] + _flags() + ["-S", "--cuda-device-only", SRC, "-o", out], check=True, capture_output=True)
        return open(out).read()


def _kernel_body(n, inverse, clamp):
    key = f"sr_count_kernelILi{n}ELb{int(inverse)}ELb{int(clamp)}E"
    m = re.search(r"\n(_Z\w*" + re.escape(key) + r"\w*):[^\n]*\n(.*?)s_endpgm", _device_asm(), re.S)
    assert m, key
    lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
    return [l for l in lines if l and not l.endswith(":") and not l.startswith(".")]


def _arith_f32(body):
    """tools/isa_phases.py, class arith_f32"""
    out = []
    for l in body:
        base = l.split()[0].replace("_e32", "").replace("_e64", "")
        if base.startswith("v_") and re.match(r"v_(fma|fmac|mul|add|sub|mad|pk_)", base) and "f32" in base:
            out.append((base, l))
    return out


@pytest.mark.parametrize("inverse,clamp", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_instruction_counts(n, inverse, clamp):
    body = _kernel_body(n, inverse, clamp)
    arith = _arith_f32(body)
    mix = {}
    for base, _ in arith:
        mix[base] = mix.get(base, 0) + 1
    print(f"n={n} inverse={inverse} clamp={clamp}: {len(arith)} float32 arithmetic instructions {dict(sorted(mix.items()))}")
    assert len(arith) == COUNTS[n]
    assert not any(base in ("v_mul_f32", "v_mad_f32") or base.startswith("v_pk_") for base, _ in arith)
    # an FMA is two registers and a constant (v_fmamk / v_fmac); the VOP3 form appears only where it carries the clip, and then its
    # constant is a scalar register or a literal, never a third vector register
    for base, l in arith:
        if base == "v_fma_f32":
            srcs = [o.strip() for o in l.split(None, 1)[1].replace(" clamp", "").split(",")][1:]
            assert clamp and " clamp" in l and sum(1 for o in srcs if re.match(r"-?v\d+$", o)) == 2, l
    if clamp:   # the clip rides on the last instruction of each of the 2 n outputs and is nowhere else
        assert not [l for l in body if re.match(r"v_(med3|max|min)", l)], "the clip did not fold into the last instruction"
        assert sum(1 for _, l in arith if " clamp" in l) == 2 * n
    else:
        assert not any(" clamp" in l for _, l in arith)
