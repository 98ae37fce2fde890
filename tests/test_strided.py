"""CPU: the strided-batch plans' ABI (include/fft_wgpu_amd_strided.h), host logic and mirrors -- no GPU needed.

fws_describe is pure host logic: the geometry rule of the header is checked here for every supported length, the status
codes of unsupported and invalid shapes, and that NULL handles are refused before any device is touched.
"""
import ctypes
import os
import re
import subprocess

import pytest
import side_libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fft_wgpu_amd_strided.h")
LENGTHS = [1 << lg for lg in range(1, 13)]
INVALID_ARG, UNSUPPORTED = 1, 6


@pytest.fixture(scope="session")
def strided():
    """The library is built by the session that needs it (tests/conftest.py builds csrc only)."""
    return side_libs.load("strided")


def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fws_[a-z0-9_]+)\s*\(", text)))


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd_strided.h"\n'
                   "int use(fwa_ctx *c, fwa_buf *b) { fws_plan *p = 0; int32_t t, th, l; uint64_t bl;\n"
                   "  if (fws_describe(1024, 17, 2, &t, &th, &l, &bl)) return 1;\n"
                   "  if (fws_plan_create(c, FWA_FORWARD, 1024, 17, b, &p)) return 2;\n"
                   "  return fws_plan_exec(p, 0) + fws_plan_destroy(p) + (fws_abi_version() != FWS_ABI_VERSION); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_binding_names_exactly_the_declared_functions(strided):
    names = _header_functions()
    assert names == ["fws_abi_version", "fws_describe", "fws_plan_create", "fws_plan_destroy", "fws_plan_exec",
                     "fws_plan_get_i64"]
    assert sorted(strided._SIGNATURES) == names
    out = subprocess.check_output(["nm", "-D", "--defined-only", strided.LIB_PATH], text=True)
    exported = sorted(set(re.findall(r"\bT (fws_[a-z0-9_]+)$", out, flags=re.M)))
    assert exported == names
    assert strided.lib().fws_abi_version() == strided.ABI_VERSION == 1


def test_the_library_loads_on_first_use_not_with_the_package():
    code = ("import sys; sys.path.insert(0, %r); import fft_wgpu_amd as fw; "
            "assert fw.strided._lib is None; "
            "assert not any('strided' in l for l in open('/proc/self/maps')); print('ok')" % ROOT)
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "ok"


@pytest.mark.parametrize("n", LENGTHS)
def test_describe_follows_the_rule_of_the_header(strided, n):
    """tile_cols 16 (8 at 4096); blocks = batch * ceil(ceil(howmany / tile_cols) / tiles_per_workgroup) with
    tiles_per_workgroup = 512 / n for n <= 32, else 1; the launch fits the hardware."""
    for howmany in (1, 16, 17, 1000):
        for batch in (1, 3):
            g = strided.describe(n, howmany, batch)
            assert g["tile_cols"] == (8 if n == 4096 else 16)
            assert 64 <= g["threads"] <= 1024 and g["threads"] % 64 == 0
            assert 0 <= g["lds_bytes"] <= 163840
            tiles = -(-howmany // g["tile_cols"])
            per_wg = 512 // n if n <= 32 else 1
            assert g["blocks"] == batch * -(-tiles // per_wg), (n, howmany, batch, g)
            if n <= 32:
                assert g["threads"] == 256 and g["lds_bytes"] == 0              # a thread holds a whole column
            else:
                assert g["lds_bytes"] == n * g["tile_cols"] * 4                 # one plane of the tile: re, then im
                assert g["threads"] * {64: 8, 128: 16, 256: 16}.get(n, 32) == n * g["tile_cols"]
    assert strided.describe(1024, 16)["threads"] == 512 and strided.describe(1024, 16)["lds_bytes"] == 65536


@pytest.mark.parametrize("n,status,word", [(1, UNSUPPORTED, "4096"), (8192, UNSUPPORTED, "4096"), (0, INVALID_ARG, "power"),
                                           (48, INVALID_ARG, "power")])
def test_describe_refuses_other_lengths(strided, n, status, word):
    from fft_wgpu_amd import FwaError
    with pytest.raises(FwaError) as e:
        strided.describe(n, 16)
    assert e.value.status == status and word in e.value.detail
    with pytest.raises(FwaError) as e:
        strided.describe(64, 0)
    assert e.value.status == INVALID_ARG


def test_null_handles_are_rejected_without_a_device(strided):
    L = strided.lib()
    out = ctypes.c_void_p()
    v = ctypes.c_int64()
    assert L.fws_plan_create(None, 0, 64, 16, None, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fws_plan_create(None, 0, 64, 16, None, None) == INVALID_ARG
    assert L.fws_plan_exec(None, None) == INVALID_ARG
    assert L.fws_plan_get_i64(None, b"batch", ctypes.byref(v)) == INVALID_ARG
    assert L.fws_plan_destroy(None) == 0
    assert L.fws_describe(64, 16, 1, None, None, None, None) == 0            # every output pointer is optional


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    src = tmp_path / "stale.c"
    src.write_text("int fws_abi_version(void) { return 0; }\n")
    lib = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    code = ("import sys; sys.path.insert(0, %r); from fft_wgpu_amd import strided as s; s.LIB_PATH = %r\n"
            "try:\n    s.lib()\nexcept RuntimeError as e:\n    print('refused' if 'ABI version 0' in str(e) else e)\n"
            % (ROOT, str(lib)))
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "refused"


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text('#include "fft_wgpu_strided.hpp"\n'
                   "int run(uint32_t n, uint64_t h) {\n"
                   "  fft_wgpu::Device dev(0); fft_wgpu::Buffer buf(dev, 8ull * n * h); fft_wgpu::CommandEncoder enc(dev);\n"
                   "  fft_wgpu::strided::Forward f(dev, dev, buf, n, h);\n"
                   "  fft_wgpu::strided::Inverse i(dev, dev, buf, n, h);\n"
                   "  fft_wgpu::strided::Onlyinverse o(dev, dev, buf, n, h);\n"
                   "  fft_wgpu::Buffer &r = f.proc(enc); i.proc(enc); o.proc(enc); enc.synchronize();\n"
                   "  return (&r == &buf) + (int)f.get(\"blocks\") + fft_wgpu::strided::describe(n, h).threads; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_kernels_live_beside_csrc_and_restate_nothing():
    d = os.path.join(ROOT, "fft_wgpu_amd", "strided")
    assert sorted(os.listdir(d))[:1] and not os.path.exists(os.path.join(ROOT, "fft_wgpu_amd", "csrc", "kernels_strided.hip"))
    hip = open(os.path.join(d, "kernels_strided.hip")).read()
    assert '#include "../csrc/device_common.h"' in hip
    for helper in ("void fft_reg(", "v2f cmul_tw(", "uint32_t xcd_map(", "hipError_t check_grid(", "hipError_t raise_lds_limit("):
        assert helper not in hip, helper
    for banned in ("sinf(", "cosf(", "sincosf(", "rocfft", "mfma"):
        assert banned not in hip.lower(), banned
