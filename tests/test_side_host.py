"""CPU: what the five side plan libraries share is stated once -- fft_wgpu_amd/side/side_host.h (the host checks), side.mk
(the build), fft_wgpu_amd/_ffi.load (the loader) and fft_wgpu_amd/_side.Plan (the plan classes) -- and each stays what it says
it is: the header plain C++ without a device header, the build one host compile, one kernel compile and one link per library.
"""
import os
import re
import shutil
import subprocess

import pytest

import side_libs
from test_build_layers import DEVICE_HEADERS, HOST_CXX

ROOT = side_libs.ROOT
PKG = os.path.join(ROOT, "fft_wgpu_amd")
SIDE_HOST = os.path.join(PKG, "side", "side_host.h")
SHARED_LITERALS = ("belongs to another context", "unknown key: ", "2^31 - 1 workgroups")


def test_the_helper_header_is_plain_cpp_and_reaches_no_device_header(tmp_path):
    user = tmp_path / "user.cpp"
    user.write_text('#include "%s"\n' % SIDE_HOST)
    subprocess.run(HOST_CXX + ["-Wall", "-Werror", "-fsyntax-only", str(user)], check=True)
    deps = subprocess.run(HOST_CXX + ["-MM", str(user)], check=True, capture_output=True, text=True).stdout
    deps = {os.path.basename(d) for d in deps.replace("\\\n", " ").split()[1:]}
    assert {"side_host.h", "internal.h", "kernels.h"} <= deps
    assert not deps & set(DEVICE_HEADERS), sorted(deps & set(DEVICE_HEADERS))
    assert not re.search(r"__device__|__global__|<<<", open(SIDE_HOST).read())


def test_the_host_files_state_none_of_the_shared_checks():
    header = open(SIDE_HOST).read()
    hosts = {name: open(os.path.join(PKG, name, name + ".cpp")).read() for name in side_libs.NAMES}
    for literal in SHARED_LITERALS:
        assert header.count(literal) == 1, literal
        for name, text in hosts.items():
            assert literal not in text, (name, literal)
    for name, text in hosts.items():
        assert '#include "../side/side_host.h"' in text, name


def test_one_loader_and_one_plan_base():
    """`def lib` of a side module is the cache around one call of the loader; the loader's refusal is written once."""
    modules = {f: open(os.path.join(PKG, f)).read() for f in os.listdir(PKG) if f.endswith(".py")}
    assert sum(text.count("reports ABI version") for text in modules.values()) == 1
    assert sum(text.count("ctypes.CDLL(") for text in modules.values()) == 1
    for name in side_libs.NAMES:
        text = modules[name + ".py"]
        body = re.search(r"^def lib\(\):\n((?:    .*\n|\n)+)", text, flags=re.M).group(1).rstrip("\n").split("\n")
        assert len(body) <= 7 and "_ffi.load(LIB_PATH, " in "".join(body), (name, body)
        assert "class _Plan(_side.Plan):" in text and "def proc" not in text and "def __del__" not in text, name
        assert not re.search(r"^_\w+ = ctypes\.", text, flags=re.M), name       # the ctypes aliases are _ffi's


@pytest.mark.parametrize("name", side_libs.NAMES)
def test_a_side_library_is_one_host_compile_one_kernel_compile_and_one_link(tmp_path, name):
    """`make -n` on a copy of the sources that holds no object; the libraries it links against stand there as empty files,
    so that only this directory's rules speak."""
    pkg = tmp_path / "fft_wgpu_amd"
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    for d in ("csrc", "side") + side_libs.NAMES:
        (pkg / d).mkdir(parents=True)
        for f in os.listdir(os.path.join(PKG, d)):
            if f == "Makefile" or f.endswith((".cpp", ".h", ".hip", ".mk")):
                shutil.copy2(os.path.join(PKG, d, f), pkg / d)
    for lib in ("libfft_wgpu_amd.so", "libfft_wgpu_amd_strided.so"):
        if lib != "libfft_wgpu_amd_%s.so" % name:
            (pkg / lib).write_bytes(b"")
    plan = subprocess.run(["make", "-n", "-C", str(pkg / name)], check=True, capture_output=True, text=True).stdout
    lines = [ln for ln in plan.splitlines() if "hipcc" in ln]
    assert len(lines) == 3, plan
    host = [ln for ln in lines if " -x c++ " in ln]
    kernels = [ln for ln in lines if " --offload-arch=gfx950 -c " in ln]
    link = [ln for ln in lines if " -shared " in ln]
    assert (len(host), len(kernels), len(link)) == (1, 1, 1), plan
    assert " -c %s.cpp " % name in host[0] and "--offload-arch" not in host[0] and "-x hip" not in host[0], host[0]
    assert " -c kernels_%s.hip " % name in kernels[0] and "-x c++" not in kernels[0], kernels[0]
    assert ["kernels_%s.o" % name, "%s.o" % name] == [w for w in link[0].split() if w.endswith(".o")], link[0]
