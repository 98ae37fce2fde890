"""tools/mutant_build.py -- the copy-and-substitute build of the mutant tools (error_budget_mutants.py, ordering_mutants.py).

build(name, substitutions): copy fft_wgpu_amd/csrc, objects included, to build/variants/<name>/csrc (as tools/build_variant.sh
does), apply the textual substitutions [(file, old, new), ...] -- each must match exactly once, so a tool fails loudly when the
source drifts -- and `make lab -j16`: only what depends on a mutated file is rebuilt.  The laboratory library of the mutant
is lib_path(name).
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = os.path.join(ROOT, "build", "variants")
CSRC = os.path.join(ROOT, "fft_wgpu_amd", "csrc")
TREE_LAB_LIBRARY = os.path.join(ROOT, "fft_wgpu_amd", "libfft_wgpu_amd_lab.so")   # the unmutated control


def lib_path(name):
    return os.path.join(VARIANTS, name, "libfft_wgpu_amd_lab.so")


def build(name, substitutions):
    dst = os.path.join(VARIANTS, name, "csrc")
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    inc = os.path.join(VARIANTS, "include")       # csrc includes ../../include/fft_wgpu_amd.h
    os.makedirs(inc, exist_ok=True)
    for f in os.listdir(os.path.join(ROOT, "include")):
        shutil.copy2(os.path.join(ROOT, "include", f), inc)
    for f in os.listdir(CSRC):
        if f.endswith(".so"):
            continue
        shutil.copy2(os.path.join(CSRC, f), dst)   # keeps mtimes: make rebuilds only what depends on the mutated file
    for fname, old, new in substitutions:
        p = os.path.join(dst, fname)
        src = open(p).read()
        hits = src.count(old)
        if hits != 1:
            raise SystemExit("%s: substitution in %s matched %d times (expected exactly once): %r" % (name, fname, hits, old))
        with open(p, "w") as f:
            f.write(src.replace(old, new))
    jobs = min(16, os.cpu_count() or 1)
    subprocess.check_call(["make", "-s", "-C", dst, "-j%d" % jobs, "lab"])
    print("%s: built %s" % (name, os.path.relpath(lib_path(name), ROOT)), flush=True)
