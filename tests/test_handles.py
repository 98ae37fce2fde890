"""The handle registry (fft_wgpu_amd/csrc/handles.h) raced on a CPU, under ThreadSanitizer and under AddressSanitizer + UBSan.

include/fft_wgpu_amd.h promises that buffer, stream and event handles may be freed from any thread, also while another thread
destroys their context.  tools/handle_stress.cpp is a stand-alone program over handles.h alone (no HIP, no Python): worker
threads detach and delete handles while one more thread detaches them all and deletes the context, and rounds of concurrent
attach / detach; it checks counts, creation order, null links and an empty list itself.  A data race, a use after free or a
failed check shows up as output on stderr or a non-zero exit status.
"""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixed_layout():
    """The sanitizer runtimes g++ links reserve fixed address ranges for their shadow memory: where the kernel randomises
    mappings over more bits than they expect, the program ends before main ("FATAL: ThreadSanitizer: unexpected memory
    mapping").  So the program is started with address randomisation off for itself (`setarch -R`: a flag of that one process)
    where the host allows that; what is checked does not depend on where the mappings lie."""
    setarch = shutil.which("setarch")
    cmd = [setarch, platform.machine(), "-R"] if setarch else []
    return cmd if cmd and subprocess.run(cmd + ["true"], capture_output=True).returncode == 0 else []


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_handle_registry_races_clean_under_sanitizers(tmp_path, sanitize):
    exe = tmp_path / "handle_stress"
    # the sanitizer runtimes are linked into the program: it then starts whatever else the loader has been told to load first
    static = ["-static-lib" + {"thread": "tsan", "address": "asan", "undefined": "ubsan"}[s] for s in sanitize.split(",")]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize,
                           "-fno-sanitize-recover=all", *static, "-I" + os.path.join(ROOT, "fft_wgpu_amd", "csrc"),
                           os.path.join(ROOT, "tools", "handle_stress.cpp"), "-o", str(exe)])
    r = subprocess.run(_fixed_layout() + [str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "200 destroy rounds and 200 churn rounds, 4 threads x 64 handles: ok" in r.stdout
