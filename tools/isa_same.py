#!/usr/bin/env python3
"""Is the device code of the tree the same as that of a revision?   usage: tools/isa_same.py <git-rev> [unit ...]
Compiles each translation unit twice with the Makefile's HIPFLAGS plus --cuda-device-only -S -- once with the sources of <git-rev>
(git archive, as build_variant.sh -r takes them with git show), once with the tree's --, replaces the __hip_cuid_<hash> symbol by a
fixed word and compares the assembly text.  One line per unit: `same`, or the first differing line and the symbol it lies in; exit
status 1 on any difference.  Default units: every pyorc_amd/csrc/*.hip and tests/native/*.hip that includes piv_fft_impl.h or
fft_regs.h, directly or through another header.  A unit is named by its file (piv_fft64, piv_fft64.hip or a path)."""
import concurrent.futures, glob, io, os, re, shutil, subprocess, sys, tarfile, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRS = ("pyorc_amd/csrc", "include", "tests/native")
KERNEL_HEADERS = {"piv_fft_impl.h", "fft_regs.h"}


def includes(path, seen):
    """names of the headers `path` reaches through #include "..." (all of them live in pyorc_amd/csrc)"""
    for name in re.findall(r'^\s*#include\s+"([^"]+)"', open(path).read(), re.M):
        name = os.path.basename(name)
        if name not in seen and os.path.exists(os.path.join(ROOT, DIRS[0], name)):
            seen.add(name)
            includes(os.path.join(ROOT, DIRS[0], name), seen)
    return seen


def compile_unit(side, unit, flags):
    out = os.path.join(side, unit.replace("/", "_") + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the Makefile's default
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", "-I", os.path.join(side, DIRS[0]), os.path.join(side, unit), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return (out, "") if r.returncode == 0 else (None, r.stderr[-2000:])


def compare(unit, ra, rb):
    if ra[0] is None or rb[0] is None:
        return f"{unit}: DOES NOT COMPILE ({'revision' if ra[0] is None else 'tree'})\n{ra[1] or rb[1]}"
    a, b = (re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(r[0]).read()).splitlines() for r in (ra, rb))
    if a == b:
        return None
    i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    named = re.search(r"\.text\.(\w+)", b[i] if i < len(b) else "")   # a function's .section line stands before its label
    sym = named.group(1) if named else next((l.split(":")[0] for l in reversed(b[:i + 1]) if re.match(r"^[A-Za-z_][\w.$]*:", l)), "the unit's head")
    return f"{unit}: DIFFERS at line {i + 1} in {sym}\n  - {a[i] if i < len(a) else '<end>'}\n  + {b[i] if i < len(b) else '<end>'}"


def main():
    rev, named = sys.argv[1], sys.argv[2:]
    mk = open(os.path.join(ROOT, DIRS[0], "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    if named:
        units = [next(p for p in (u, f"{DIRS[0]}/{u}", f"{DIRS[0]}/{u}.hip", f"{DIRS[2]}/{u}", f"{DIRS[2]}/{u}.hip") if os.path.isfile(os.path.join(ROOT, p))) for u in named]
    else:
        units = [os.path.relpath(p, ROOT) for d in (DIRS[0], DIRS[2]) for p in sorted(glob.glob(os.path.join(ROOT, d, "*.hip"))) if KERNEL_HEADERS & includes(p, set())]
    with tempfile.TemporaryDirectory() as tmp:
        ref, new = os.path.join(tmp, "ref"), os.path.join(tmp, "new")
        tarfile.open(fileobj=io.BytesIO(subprocess.check_output(["git", "-C", ROOT, "archive", rev, *DIRS]))).extractall(ref)
        for d in DIRS:
            shutil.copytree(os.path.join(ROOT, d), os.path.join(new, d), ignore=shutil.ignore_patterns("*.o", "*.so", "__pycache__"))
        with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            asm = list(pool.map(lambda su: compile_unit(su[0], su[1], flags), [(s, u) for u in units for s in (ref, new)]))
        results = [compare(u, asm[2 * k], asm[2 * k + 1]) for k, u in enumerate(units)]
    for u, r in zip(units, results):
        print(r or f"{u}: same")
    return 1 if any(results) else 0


if __name__ == "__main__":
    sys.exit(main())
