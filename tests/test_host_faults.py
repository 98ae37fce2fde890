"""The host layer on a simulated HIP runtime, on a CPU: every HIP call and every launch of the host code fails once.

The host side of the library (fft_wgpu_amd/csrc/{ctx_streams,buffers,tables,plan,tuning,comm,lab_present}.cpp and the four
side-library hosts) is plain C++ behind the launcher prototypes, so it links against anything that defines them.
tools/host_sim/ defines them: fake_hip.cpp is a HIP runtime whose device memory is address space only and whose streams and
events carry logical clocks, fake_kernels.cpp records for every launcher the bytes its kernel reads and writes, and
host_faults.cpp runs scenarios over the public C ABI -- clean, over every tiled geometry of 2^16 .. 2^30, and once per
injectable call with that call failing -- under the checks its header comment lists.  No device, no Python bindings, no
threads; AddressSanitizer + UBSan guard the host side of every copy and the library's own bookkeeping.  A violation, a
leak or a sanitizer report shows up as a non-zero exit status, a missing summary line or output on stderr.
"""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SOURCES = [os.path.join("fft_wgpu_amd", "csrc", f + ".cpp")
                for f in ("ctx_streams", "buffers", "tables", "plan", "tuning", "comm", "lab_present")] + \
               [os.path.join("fft_wgpu_amd", d, d + ".cpp") for d in ("strided", "fft2d", "real", "conv")]
SIM_SOURCES = [os.path.join("tools", "host_sim", f + ".cpp") for f in ("fake_hip", "fake_kernels", "host_faults")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _fixed_layout():
    """As in tests/test_handles.py: the sanitizer runtime reserves fixed address ranges for its shadow memory, so the program
    is started with address randomisation off for itself (`setarch -R`) where the host allows that."""
    setarch = shutil.which("setarch")
    cmd = [setarch, platform.machine(), "-R"] if setarch else []
    return cmd if cmd and subprocess.run(cmd + ["true"], capture_output=True).returncode == 0 else []


def _rocm():
    """ROCm's clang++ and its include directory, found the way fft_wgpu_amd/csrc/Makefile finds the latter: next to hipcc."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    clang = next((c for c in (os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++"),
                              os.path.join(root, "bin", "amdclang++")) if os.path.exists(c)), None)
    assert clang, "ROCm's clang++ not found next to " + hipcc
    return clang, os.path.join(root, "include")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_sim")
    clang, include = _rocm()
    common = [clang, *FLAGS, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include]
    jobs = []
    for src in HOST_SOURCES + SIM_SOURCES:
        obj = out / (src.replace(os.sep, "_") + ".o")
        strict = ["-Wall", "-Wextra", "-Werror"] if src in SIM_SOURCES else []   # the three new files only
        jobs.append((obj, subprocess.Popen(common + strict + ["-c", os.path.join(ROOT, src), "-o", str(obj)],
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for obj, job in jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log[-4000:]
    exe = out / "host_faults"
    # the sanitizer runtime is linked into the program; a missing runtime entry point or launcher is a link error here
    subprocess.check_call([clang, "-fsanitize=address,undefined", "-static-libsan", *[str(o) for o, _ in jobs], "-ldl",
                           "-o", str(exe)])
    return exe


def _run(program, *args):
    r = subprocess.run(_fixed_layout() + [str(program), *args], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return r.stdout


def test_the_checks_bite(program):
    """Misuse of the fake itself: a double hipFree, a launch 8 bytes past an allocation, a read of an unwritten table, two
    overlapping ring writes on two streams with no event between them, one leaked event -- each its own kind of violation."""
    out = _run(program, "--selftest")
    assert "host_faults selftest: 5 of 5 misuse kinds reported, each as its own kind: ok" in out
    for kind in ("double-free", "out-of-bounds", "unwritten-read", "hazard", "leak"):
        assert "-> %s x1, 1 in all: reported" % kind in out


def test_clean_audit(program):
    """Every scenario with nothing armed: no violation of any kind, launches per exec as launches_per_exec says, no exec
    allocates or creates a stream or an event, nothing alive after the last destroy, LeakSanitizer silent."""
    out = _run(program, "--clean")
    m = re.search(r"^host_faults clean: (\d+) scenarios, (\d+) execs, 0 violations, 0 live resources: ok$", out, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (60, 119), out[-300:]


def test_geometry_sweep(program):
    """Tiled and pipelined plans of every log2 n = 16 .. 30 x batch {1, 3, 17, 40} (n x batch <= 2^32) x group {1, 2,
    default} x streams {1, 2, 3}: every range inside a live allocation, every byte read written, two chains' slabs disjoint."""
    out = _run(program, "--geometry")
    # 15 lengths x (4 batches, fewer where the cap makes them meet: 3 each at 2^28 .. 2^30) x 3 groups x 3 streams
    assert "host_faults geometry: 513 plans of 2^16 .. 2^30, " in out and ", 0 violations, 0 live resources: ok" in out


def test_fault_sweep(program):
    """Every scenario on n <= 2^20, once per injectable call of its clean run with that call failing; every injectable
    runtime function and every launcher has been the failing call at least once.  The expected set is declared by the fake
    itself before anything runs (every entry point of fake_hip.cpp but the three error reporters, every launcher and setup of
    fake_kernels.cpp), so a function that no scenario reaches any more is a row "never failed" and fails the run; the counts
    are held here as well: 26 runtime functions, 32 launchers and setups, the 52 scenarios on n <= 2^20, and no fewer
    injection points than when this was written (a host change that adds a HIP call adds points; losing some loses cover)."""
    out = _run(program, "--faults")
    m = re.search(r"^host_faults faults: (\d+) scenarios, (\d+) injection points, 0 violations, failing call at least once: "
                  r"(\d+) runtime functions and (\d+) launchers and setups, 0 never: ok$", out, re.M)
    assert m, out[-400:]
    scenarios, points, runtime, launchers = map(int, m.groups())
    assert (scenarios, runtime, launchers) == (52, 26, 32) and points >= 3582, m.group(0)
    assert "never failed" not in out
    assert out.count("counters after a failed fwa_plan_set_i64") > 0      # printed, not asserted


def test_a_partial_sweep_fails_the_coverage_condition(program):
    """One scenario alone reaches 18 of the 58 functions: the condition must say so (it once passed on whatever it saw)."""
    r = subprocess.run(_fixed_layout() + [str(program), "--faults", "--only", "side libraries: small"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert re.search(r"0 violations, failing call at least once: 10 runtime functions and 8 launchers and setups, 40 never: FAILED$",
                     r.stdout, re.M), r.stdout[-400:]
    assert r.stdout.count("<-- never failed") == 40
