"""CPU: the 2-D plans' ABI (include/fft_wgpu_amd_2d.h), host logic and mirrors -- no GPU needed.

fw2_describe is pure host logic: the path table of the header is checked here for all 144 (rows, cols) pairs, the status
codes of unsupported and invalid shapes, and that NULL handles are refused before any device is touched.
"""
import ctypes
import os
import re
import subprocess

import pytest
import side_libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fft_wgpu_amd_2d.h")
LENGTHS = [1 << lg for lg in range(1, 13)]
INVALID_ARG, UNSUPPORTED = 1, 6
NAMES = ["fw2_abi_version", "fw2_describe", "fw2_plan_create", "fw2_plan_destroy", "fw2_plan_exec", "fw2_plan_get_i64"]


@pytest.fixture(scope="session")
def fft2d():
    """The library is built by the session that needs it (tests/conftest.py builds csrc only)."""
    return side_libs.load("fft2d")


@pytest.fixture(scope="session")
def strided(fft2d):
    from fft_wgpu_amd import strided as s
    s.lib()
    return s


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd_2d.h"\n'
                   "int use(fwa_ctx *c, fwa_buf *b) { fw2_plan *p = 0; int32_t n, th, l; uint64_t bl; int64_t v;\n"
                   "  if (fw2_describe(64, 512, 2, &n, &th, &l, &bl)) return 1;\n"
                   "  if (fw2_plan_create(c, FWA_INVERSE_SCALED, 64, 512, b, &p)) return 2;\n"
                   '  if (fw2_plan_get_i64(p, "col_blocks", &v)) return 3;\n'
                   "  return fw2_plan_exec(p, 0) + fw2_plan_destroy(p) + (fw2_abi_version() != FW2_ABI_VERSION); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_binding_names_exactly_the_declared_functions(fft2d):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fw2_[a-z0-9_]+)\s*\(", text))) == NAMES
    assert sorted(fft2d._SIGNATURES) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", fft2d.LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (fw2_[a-z0-9_]+)$", out, flags=re.M))) == NAMES
    assert not re.findall(r"\bT (fw[as]_[a-z0-9_]+)$", out, flags=re.M)       # the other two libraries' calls are linked, not restated
    assert fft2d.lib().fw2_abi_version() == fft2d.ABI_VERSION == 1


def test_the_library_loads_on_first_use_not_with_the_package():
    code = ("import sys; sys.path.insert(0, %r); import fft_wgpu_amd as fw; "
            "assert fw.fft2d._lib is None; "
            "assert not any('amd_2d' in l or 'strided' in l for l in open('/proc/self/maps')); print('ok')" % ROOT)
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "ok"


@pytest.mark.parametrize("rows", LENGTHS)
def test_describe_follows_the_path_table(fft2d, strided, rows):
    """all 144 pairs (12 widths per case), batch 1 and 3:
         rows <= 32 and cols <= 32   1 launch,   256 threads, row_blocks = ceil(batch rows cols / 8192)
         cols <= 32, rows >= 64      2 launches, the same row launch
         cols >= 64                  2 launches, threads and RT = tile_cols of the strided geometry of cols,
                                     row_blocks = ceil(batch rows / RT), LDS = one plane of the tile
       row_lds_bytes <= 81920 for the chunk kernel (two workgroups per CU) and <= 163840 everywhere."""
    for cols in LENGTHS:
        for batch in (1, 3):
            g = fft2d.describe(rows, cols, batch)
            assert sorted(g) == ["launches", "row_blocks", "row_lds_bytes", "row_threads"]
            assert g["launches"] == (1 if rows <= 32 and cols <= 32 else 2), (rows, cols)
            assert 0 < g["row_lds_bytes"] <= 163840
            if cols <= 32:
                assert g["row_threads"] == 256
                assert 65536 <= g["row_lds_bytes"] <= 81920                  # two planes of 8192 words plus padding
                assert g["row_blocks"] == -(-batch * rows * cols // 8192), (rows, cols, batch, g)
            else:
                s = strided.describe(cols, 16)
                rt = s["tile_cols"]
                assert rt == (8 if cols == 4096 else 16)
                assert g["row_threads"] == s["threads"] and g["row_threads"] % 64 == 0
                assert g["row_lds_bytes"] >= cols * rt * 4 and g["row_lds_bytes"] - cols * rt * 4 <= 4096   # plane + skew
                assert g["row_blocks"] == -(-batch * rows // rt), (rows, cols, batch, g)
    assert fft2d.describe(4096, 4096, 33)["row_blocks"] == 33 * 512


@pytest.mark.parametrize("n,status,word", [(1, UNSUPPORTED, "1-D"), (8192, UNSUPPORTED, "4096"), (0, INVALID_ARG, "power"),
                                           (48, INVALID_ARG, "power")])
def test_describe_refuses_other_lengths(fft2d, n, status, word):
    from fft_wgpu_amd import FwaError
    for shape, axis in (((n, 64), "rows"), ((64, n), "cols"), ((n, 8), "rows"), ((8, n), "cols")):
        with pytest.raises(FwaError) as e:
            fft2d.describe(*shape)
        assert e.value.status == status and word in e.value.detail and axis in e.value.detail, (shape, e.value.detail)
    # more than 2^31 - 1 workgroups in the row launch
    with pytest.raises(FwaError) as e:
        fft2d.describe(4096, 64, 1 << 24)
    assert e.value.status == UNSUPPORTED and "workgroups" in e.value.detail


def test_null_handles_are_rejected_without_a_device(fft2d):
    L = fft2d.lib()
    out = ctypes.c_void_p()
    v = ctypes.c_int64()
    assert L.fw2_plan_create(None, 0, 64, 16, None, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fw2_plan_create(None, 0, 64, 16, None, None) == INVALID_ARG
    assert L.fw2_plan_exec(None, None) == INVALID_ARG
    assert L.fw2_plan_get_i64(None, b"batch", ctypes.byref(v)) == INVALID_ARG
    assert L.fw2_plan_destroy(None) == 0
    assert L.fw2_describe(64, 16, 1, None, None, None, None) == 0            # every output pointer is optional


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    src = tmp_path / "stale.c"
    src.write_text("int fw2_abi_version(void) { return 0; }\n")
    lib = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    code = ("import sys; sys.path.insert(0, %r); from fft_wgpu_amd import fft2d as m; m.LIB_PATH = %r\n"
            "try:\n    m.lib()\nexcept RuntimeError as e:\n    print('refused' if 'ABI version 0' in str(e) else e)\n"
            % (ROOT, str(lib)))
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "refused"


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text('#include "fft_wgpu_2d.hpp"\n'
                   "int run(uint32_t r, uint32_t c) {\n"
                   "  fft_wgpu::Device dev(0); fft_wgpu::Buffer buf(dev, 8ull * r * c); fft_wgpu::CommandEncoder enc(dev);\n"
                   "  fft_wgpu::fft2d::Forward f(dev, dev, buf, r, c);\n"
                   "  fft_wgpu::fft2d::Inverse i(dev, dev, buf, r, c);\n"
                   "  fft_wgpu::fft2d::Onlyinverse o(dev, dev, buf, r, c);\n"
                   "  fft_wgpu::Buffer &y = f.proc(enc); i.proc(enc); o.proc(enc); enc.synchronize();\n"
                   "  return (&y == &buf) + (int)f.get(\"row_blocks\") + fft_wgpu::fft2d::describe(r, c).launches; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_kernels_live_beside_csrc_and_restate_nothing():
    d = os.path.join(ROOT, "fft_wgpu_amd", "fft2d")
    for other in ("csrc", "strided"):
        assert not os.path.exists(os.path.join(ROOT, "fft_wgpu_amd", other, "kernels_fft2d.hip"))
    hip = open(os.path.join(d, "kernels_fft2d.hip")).read()
    assert '#include "../csrc/device_common.h"' in hip
    for helper in ("void fft_reg(", "v2f cmul_tw(", "uint32_t xcd_map(", "hipError_t check_grid(", "hipError_t raise_lds_limit(",
                   "void stage(", "void exchange(", "v2f tw_n("):
        assert helper not in hip, helper
    for name in ("kernels_fft2d.hip", "fft2d_geom.h", "fft2d_kernels.h", "fft2d.cpp"):
        text = open(os.path.join(d, name)).read().lower()
        for banned in ("sinf(", "cosf(", "sincosf(", "rocfft", "mfma"):
            assert banned not in text, (name, banned)
    # the stage arithmetic is shared with k_strided, stated once
    net = open(os.path.join(ROOT, "fft_wgpu_amd", "strided", "strided_net.h")).read()
    strided_hip = open(os.path.join(ROOT, "fft_wgpu_amd", "strided", "kernels_strided.hip")).read()
    assert "void stage(" in net and "void exchange(" in net and "v2f tw_n(" in net
    assert '#include "../strided/strided_net.h"' in hip and '#include "strided_net.h"' in strided_hip
    assert "void stage(" not in strided_hip and "void exchange(" not in strided_hip
