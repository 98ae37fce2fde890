"""The host layer on a simulated HIP runtime and a simulated RCCL, on a CPU: every HIP call, every RCCL call and every launch of
the host code fails once, and scatter / gather / sendrecv run at world 1 .. 8.

The host side of the library (fft_wgpu_amd/csrc/{ctx_streams,buffers,tables,plan,tuning,comm,lab_present}.cpp and the five
side-library hosts) is plain C++ behind the launcher prototypes, so it links against anything that defines them.
tools/host_sim/ defines them: fake_hip.cpp is a HIP runtime whose device memory is address space only and whose streams and
events carry logical clocks, fake_kernels.cpp records for every launcher the bytes its kernel reads and writes, fake_rccl.cpp
holds the contract of the eight RCCL entry points comm.cpp resolves (the program has the books; a forwarding librccl.so.1 built
here from the same file is what comm.cpp's dlopen finds, through the child's LD_LIBRARY_PATH), and host_faults.cpp runs
scenarios over the public C ABI -- clean, over every tiled geometry of 2^16 .. 2^30 and every framed geometry of 2 .. 4096, and
once per injectable call with that call failing -- under the checks its header comment lists.  No device, no Python bindings,
no threads; AddressSanitizer + UBSan guard the host side of every copy and the library's own bookkeeping.  A violation, a
leak or a sanitizer report shows up as a non-zero exit status, a missing summary line or output on stderr.
"""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMM = os.path.join("fft_wgpu_amd", "csrc", "comm.cpp")
HOST_SOURCES = [os.path.join("fft_wgpu_amd", "csrc", f + ".cpp")
                for f in ("ctx_streams", "buffers", "tables", "plan", "tuning", "comm", "lab_present")] + \
               [os.path.join("fft_wgpu_amd", d, d + ".cpp") for d in ("strided", "fft2d", "real", "conv", "stft")]
SIM_SOURCES = [os.path.join("tools", "host_sim", f + ".cpp") for f in ("fake_hip", "fake_kernels", "fake_rccl", "host_faults")]
FAKE_RCCL = os.path.join("tools", "host_sim", "fake_rccl.cpp")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
LINK = ["-fsanitize=address,undefined", "-static-libsan", "-rdynamic"]   # -rdynamic: librccl.so.1 finds fake_rccl_* in the program

# Three mutants of comm.cpp, one textual substitution each into a temporary copy (as tools/mutant_build.py does for the library;
# never committed, never built into it): (name, old, new, arguments of the program, the kind that must be reported).
MUTANTS = [
    # a rank that posts one piece posts it even when it is empty, while the root skips empty pieces
    ("posts_empty_piece", "if (sends[i].peer >= 0 && sends[i].bytes)", "if (sends[i].peer >= 0 && (sends[i].bytes || ns == 1))",
     ["--clean", "--only", "comm audit: world 3"], "unmatched: "),
    # the offset of a slab in the full batch taken from its count instead of its first transform
    ("offset_from_count", "offset[p] = f * tb;", "offset[p] = n * tb;",
     ["--clean", "--only", "comm audit: world 3"], "the transfer records differ from the slab rule"),
    # ncclGroupEnd skipped after a failed send or receive
    ("group_left_open", "const ncclResult_t ge = r->GroupEnd();", "const ncclResult_t ge = e != ncclSuccess ? ncclSuccess : r->GroupEnd();",
     ["--faults", "--only", "comm: scatter, exec, gather, world 3"], "group-open: "),
]


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


class Built:
    """The program, the directories of the two librccl.so.1 (the fake, and the stub that lacks ncclRecv), and the mutants."""

    def __init__(self, exe, fake_dir, stub_dir, mutants):
        self.exe, self.fake_dir, self.stub_dir, self.mutants = exe, fake_dir, stub_dir, mutants


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_sim")
    clang, include = _rocm()
    common = [clang, *FLAGS, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include]
    jobs, mutant_jobs, so_jobs = [], [], []

    def start(cmd):
        return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    for src in HOST_SOURCES + SIM_SOURCES:
        obj = out / (src.replace(os.sep, "_") + ".o")
        strict = ["-Wall", "-Wextra", "-Werror"] if src in SIM_SOURCES else []   # the simulator's own files only
        jobs.append((src, obj, start(common + strict + ["-c", os.path.join(ROOT, src), "-o", str(obj)])))
    text = open(os.path.join(ROOT, COMM)).read()
    for name, old, new, _, _ in MUTANTS:
        assert text.count(old) == 1, "mutant %s: its text occurs %d times in comm.cpp" % (name, text.count(old))
        copy = out / ("comm_%s.cpp" % name)
        copy.write_text(text.replace(old, new))
        obj = out / ("comm_%s.o" % name)
        mutant_jobs.append((name, obj, start(common + ["-I" + os.path.join(ROOT, "fft_wgpu_amd", "csrc"), "-c", str(copy), "-o", str(obj)])))
    # The two librccl.so.1: forwarding only, no sanitizer (an instrumented object does not load beside -static-libsan), undefined
    # fake_rccl_* left for the program to supply; the soname is the name comm.cpp asks for
    dirs = {}
    for kind, defs in (("fake", []), ("stub", ["-DFAKE_RCCL_NO_RECV"])):
        dirs[kind] = out / ("rccl_" + kind)
        dirs[kind].mkdir()
        so_jobs.append((kind, start([clang, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include,
                                     "-DFAKE_RCCL_SHARED", *defs, "-fPIC", "-shared", "-Wl,-soname,librccl.so.1", os.path.join(ROOT, FAKE_RCCL),
                                     "-o", str(dirs[kind] / "librccl.so.1")])))
    for _, _, job in jobs + mutant_jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log[-4000:]
    for _, job in so_jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log[-4000:]
    # the sanitizer runtime is linked into the program; a missing runtime entry point or launcher is a link error here
    exe = out / "host_faults"
    links = [(exe, [str(o) for _, o, _ in jobs])]
    mutants = {}
    for name, obj, _ in mutant_jobs:
        mutants[name] = out / ("host_faults_" + name)
        links.append((mutants[name], [str(obj) if s == COMM else str(o) for s, o, _ in jobs]))
    link_jobs = [start([clang, *LINK, *objs, "-ldl", "-o", str(target)]) for target, objs in links]
    for job in link_jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log[-4000:]
    return Built(exe, dirs["fake"], dirs["stub"], mutants)


def _start(exe, rccl_dir, *args):
    """The child alone gets the directory of a librccl.so.1, in front of whatever the search path holds."""
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([str(rccl_dir)] + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
    return subprocess.run(_fixed_layout() + [str(exe), *args], capture_output=True, text=True, timeout=300, env=env)


def _run(program, *args, rccl_dir=None):
    r = _start(program.exe, rccl_dir or program.fake_dir, *args)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    return r.stdout


def test_the_checks_bite(program):
    """Misuse of the fakes themselves: a double hipFree, a launch 8 bytes past an allocation, a read of an unwritten table, two
    overlapping ring writes on two streams with no event between them, one leaked event; a send nobody receives, a send that meets
    a shorter receive, two ranks of one id on one device, a group left open, a receive into memory of another device, a framed
    launch whose last frame runs 4 bytes past src -- each reported once, as its own kind of violation."""
    out = _run(program, "--selftest")
    assert "host_faults selftest: 11 of 11 misuse kinds reported, each as its own kind: ok" in out
    for kind in ("double-free", "out-of-bounds", "unwritten-read", "hazard", "leak", "unmatched", "size-mismatch", "comm-init", "group-open"):
        assert "-> %s x1, 1 in all: reported" % kind in out
    assert out.count("-> out-of-bounds x1, 1 in all: reported") == 3
    assert "the ordered forms of the same uses" in out and "0 violations: clean" in out


def test_clean_audit(program):
    """Every scenario with nothing armed: no violation of any kind, launches per exec as launches_per_exec says, no exec
    allocates or creates a stream or an event, nothing alive after the last destroy, LeakSanitizer silent.  Among them the
    communicator audits: world 1 .. 8 x every root x n {2, 512, 2^20} x batch {0, 1, W - 1, W, 3 W + 2} x three orders of the ranks
    and one batch past 4 GiB per world, each scatter -> exec per rank -> gather with the transfer records equal to the slab rule
    restated, one device copy or none for the root's own slab, every byte of the result written once, nothing pending."""
    out = _run(program, "--clean")
    m = re.search(r"^host_faults clean: (\d+) scenarios, (\d+) execs, 0 violations, 0 live resources: ok$", out, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == CLEAN, out[-300:]


def test_geometry_sweep(program):
    """Tiled and pipelined plans of every log2 n = 16 .. 30 x batch {1, 3, 17, 40} (n x batch <= 2^32) x group {1, 2,
    default} x streams {1, 2, 3}: every range inside a live allocation, every byte read written, two chains' slabs disjoint.
    Framed plans of every n = 2 .. 4096 x hop {1, 2, 3, n/4, n/2, n, n + 5} x L {n, n + 1, whole and partial workgroups of
    frames and half a hop} x signals {1, 3}: the same, no two workgroups on one byte, every byte of dst written once, grid and
    getters as fwt_describe says."""
    out = _run(program, "--geometry")
    # 15 lengths x (4 batches, fewer where the cap makes them meet: 3 each at 2^28 .. 2^30) x 3 groups x 3 streams
    assert "host_faults geometry: 513 plans of 2^16 .. 2^30, " in out and ", 0 violations, 0 live resources: ok" in out
    # 12 lengths x 7 hops (4 at n = 2, 5 at n = 4, 6 at n = 8, where they repeat or fall below 1) x 3 signal lengths x 2
    assert ", %d framed plans of 2 .. 4096, " % ((4 + 5 + 6 + 9 * 7) * 3 * 2) in out


def test_fault_sweep(program):
    """Every scenario on n <= 2^20, once per injectable call of its clean run with that call failing; every injectable
    runtime function, every RCCL entry point and every launcher has been the failing call at least once.  The expected set is
    declared by the fakes before anything runs (every entry point of fake_hip.cpp but the three error reporters, the seven of
    fake_rccl.cpp but ncclGetErrorString, every launcher and setup of fake_kernels.cpp), so a function that no scenario reaches
    any more is a row "never failed" and fails the run; the counts are held here as well, and no fewer injection points than when
    this was written (a host change that adds a HIP call adds points; losing some loses cover).  The communicator audits are
    sweeps and stay out; the single cases of every world size stand in for them."""
    out = _run(program, "--faults")
    m = re.search(r"^host_faults faults: (\d+) scenarios, (\d+) injection points, 0 violations, failing call at least once: "
                  r"(\d+) runtime functions and (\d+) launchers and setups, 0 never: ok$", out, re.M)
    assert m, out[-400:]
    scenarios, points, runtime, launchers = map(int, m.groups())
    assert (scenarios, runtime, launchers) == FAULTS[:3] and points >= FAULTS[3], m.group(0)
    assert "never failed" not in out
    for name in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv",
                 "launch_stft", "setup_stft_kernels"):
        assert re.search(r"^  %s +\d+ +[1-9]\d*$" % name, out, re.M), name
    assert out.count("counters after a failed fwa_plan_set_i64") > 0      # printed, not asserted


def test_a_partial_sweep_fails_the_coverage_condition(program):
    """One scenario alone reaches 18 of the 67 functions: the condition must say so (it once passed on whatever it saw)."""
    r = _start(program.exe, program.fake_dir, "--faults", "--only", "side libraries: small")
    assert r.returncode == 1 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert re.search(r"0 violations, failing call at least once: 10 runtime functions and 8 launchers and setups, 49 never: FAILED$",
                     r.stdout, re.M), r.stdout[-400:]
    assert r.stdout.count("<-- never failed") == 49


def test_a_library_without_ncclRecv_is_unsupported(program):
    """Against a second librccl.so.1 that lacks ncclRecv: fwa_comm_unique_id and fwa_comm_create (what can be reached without a
    communicator) answer FWA_ERR_UNSUPPORTED and name the symbol, no entry point of the library is called, fwa_slab and
    fwa_comm_pieces still work.  (No "no library at all" case: the search would fall through to an installed RCCL.)"""
    out = _run(program, "--stub", rccl_dir=program.stub_dir)
    assert "fwa_comm_create" in out and "librccl has no symbol ncclRecv" in out
    assert re.search(r"^host_faults stub: .* 0 violations: ok$", out, re.M), out[-400:]
    # and the scenarios refuse that library, as they refuse to run without one
    r = _start(program.exe, program.stub_dir, "--clean")
    assert r.returncode == 3 and "needs the simulated RCCL with ncclRecv" in r.stdout and r.stderr == "", (r.returncode, r.stdout[-400:], r.stderr[-400:])
    r = _start(program.exe, os.path.join(str(program.stub_dir), "nothing_here"), "--clean")
    assert r.returncode == 3 and r.stderr == "", (r.returncode, r.stdout[-400:], r.stderr[-400:])


@pytest.mark.parametrize("mutant", [m[0] for m in MUTANTS])
def test_a_mutant_of_comm_cpp_is_reported(program, mutant):
    """Each mutant fails with its kind: an empty piece posted to a root that skips it is an operation left pending, an offset
    taken from the count moves other bytes than the slab rule, a group left open after a failed send is seen when the call
    returns (that one needs a failing send, so it runs the fault sweep of one scenario)."""
    _, _, _, args, kind = next(m for m in MUTANTS if m[0] == mutant)
    r = _start(program.mutants[mutant], program.fake_dir, *args)
    print(r.stdout[-3000:])
    assert r.returncode == 1 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert kind in r.stdout and re.search(r"FAILED$", r.stdout, re.M)


# scenarios and execs of the clean audit; scenarios, runtime functions (26 of the HIP runtime + 7 of RCCL), launchers and setups (32 + 2
# framed) and the injection points of the fault sweep when this was written
CLEAN = (91, 6300)
FAULTS = (71, 33, 34, 6516)
