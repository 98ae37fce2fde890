"""The layering of fft_wgpu_amd/csrc, checked without a device: the host side of the C ABI is plain C++ behind kernels.h (launcher
prototypes, no device code), it is compiled once for the product and the laboratory library, and the two libraries differ at link
time only (internal.h; no FWA_LAB in any host file).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fft_wgpu_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_FILES = ("ctx_streams.cpp", "buffers.cpp", "tables.cpp", "plan.cpp", "tuning.cpp", "comm.cpp")
SEAM_FILES = ("lab_absent.cpp", "lab_present.cpp")
DEVICE_HEADERS = ("cplx.h", "device_common.h", "tile_body.h", "tile_kernel.h", "tile_1m.h", "rows32.h", "small32_common.h",
                  "small32_kernel.h")
# clang in C++ mode, no offload architecture: no device pass exists that could compile a kernel
HOST_CXX = [HIPCC, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17",
            "-I" + os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(HIPCC))), "include")]


@pytest.mark.parametrize("name", HOST_FILES + SEAM_FILES)
def test_host_file_is_plain_cpp_and_reaches_no_device_header(name):
    src = os.path.join(CSRC, name)
    subprocess.run(HOST_CXX + ["-Wall", "-Wno-unused-function", "-Werror", "-fsyntax-only", src], check=True, cwd=CSRC)
    deps = subprocess.run(HOST_CXX + ["-MM", src], check=True, cwd=CSRC, capture_output=True, text=True).stdout
    deps = {os.path.basename(d) for d in deps.replace("\\\n", " ").split()[1:]}
    assert "kernels.h" in deps
    assert not deps & set(DEVICE_HEADERS), sorted(deps & set(DEVICE_HEADERS))


def test_host_side_does_not_name_the_laboratory_macro():
    for name in HOST_FILES + SEAM_FILES + ("internal.h", "kernels.h"):
        hits = [ln for ln in open(os.path.join(CSRC, name)) if "FWA_LAB" in ln]
        assert not hits, (name, hits)


def test_launcher_interface_holds_no_device_code():
    text = open(os.path.join(CSRC, "kernels.h")).read()
    assert not re.search(r"__device__|__global__|<<<", text)
    includes = re.findall(r'#\s*include\s+([<"][^>"]+[>"])', text)
    assert sorted(includes) == ['"schedule.h"', "<cstdint>", "<hip/hip_runtime_api.h>"]


def test_both_libraries_compile_every_host_file_once(tmp_path):
    """`make -n all lab` on a copy without objects: one compile per host file, and the same objects in both link lines."""
    dst = tmp_path / "fft_wgpu_amd" / "csrc"
    dst.mkdir(parents=True)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    for f in os.listdir(CSRC):
        if f == "Makefile" or f.endswith((".cpp", ".h", ".hip")):
            shutil.copy2(os.path.join(CSRC, f), dst)
    plan = subprocess.run(["make", "-n", "-C", str(dst), "all", "lab"], check=True, capture_output=True, text=True).stdout
    compiles = re.findall(r"-c (\S+\.cpp) ", plan)
    assert sorted(compiles) == sorted(HOST_FILES + SEAM_FILES)
    for ln in plan.splitlines():
        if " -c " in ln and ".cpp" in ln:
            assert "-x c++" in ln and "--offload-arch" not in ln and "-x hip" not in ln, ln
    links = [ln for ln in plan.splitlines() if " -shared " in ln]
    assert len(links) == 2
    for ln in links:
        assert all(f[:-4] + ".o" in ln.split() for f in HOST_FILES), ln
    product, lab = sorted(links, key=lambda ln: "_lab.so" in ln)
    assert "lab_absent.o" in product.split() and "lab_present.o" not in product.split()
    assert "lab_present.o" in lab.split() and "lab_absent.o" not in lab.split()
