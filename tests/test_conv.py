"""CPU: the fused FFT-convolution plans' ABI (include/fft_wgpu_amd_conv.h), host logic, mirrors and arithmetic -- no GPU needed.

fwc_describe is pure host logic: it is checked here for every n = 2 .. 4096 against the geometry rule written out in
tests/conv_cases.py, with the status codes of unsupported and invalid lengths, and NULL handles are refused before any
device is touched.  The numeric checks that tests/test_gpu_conv.py applies to the GPU's results (conv_cases: parity, cap,
the one-hot sweep, the shifts) are applied here, on the same inputs, to a numpy complex64 model of the algorithm, which
passes them, and to doctored results, which fail them.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import conv_cases as cc
import side_libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fft_wgpu_amd_conv.h")
CONV_DIR = os.path.join(ROOT, "fft_wgpu_amd", "conv")
INVALID_ARG, UNSUPPORTED = 1, 6
NAMES = ["fwc_abi_version", "fwc_describe", "fwc_plan_create", "fwc_plan_destroy", "fwc_plan_exec", "fwc_plan_get_i64"]


@pytest.fixture(scope="session")
def conv():
    """The library is built by the session that needs it (tests/conftest.py builds csrc only)."""
    return side_libs.load("conv")


@pytest.fixture(scope="module", autouse=True)
def shapes_are_the_librarys(conv):
    """Every test of this file, the ones on the numpy model included, stands on the built library: the model's inputs are
    the GPU file's, sized as one full workgroup and three rows (conv_cases.default_batch), and that is only the shape that
    matters while conv_cases.rows_per_block is what the library launches."""
    for n in cc.LENGTHS:
        assert conv.describe(n, 1)["rows_per_block"] == cc.rows_per_block(n), n


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd_conv.h"\n'
                   "int use(fwa_ctx *c, fwa_buf *a, fwa_buf *h, fwa_buf *b) { fwc_plan *p = 0; int32_t th, l, r; uint64_t bl; int64_t v;\n"
                   "  if (fwc_describe(1024, 19, &th, &l, &r, &bl)) return 1;\n"
                   "  if (fwc_plan_create(c, FWA_INVERSE_SCALED, FWC_CONJ_FILTER, 1024, a, h, b, &p)) return 2;\n"
                   '  if (fwc_plan_get_i64(p, "filters", &v)) return 3;\n'
                   "  return fwc_plan_exec(p, 0) + fwc_plan_destroy(p) + (fwc_abi_version() != FWC_ABI_VERSION); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_binding_names_exactly_the_declared_functions(conv):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fwc_[a-z0-9_]+)\s*\(", text))) == NAMES
    assert sorted(conv._SIGNATURES) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", conv.LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (fwc_[a-z0-9_]+)$", out, flags=re.M))) == NAMES
    assert not re.findall(r"\bT (fw[as2r]_[a-z0-9_]+)$", out, flags=re.M)     # the main library's calls are linked, not restated
    needed = subprocess.check_output(["readelf", "-d", conv.LIB_PATH], text=True)
    assert "libfft_wgpu_amd.so" in needed
    for other in ("strided", "amd_2d", "amd_real"):                           # what it takes from those is header-only
        assert other not in needed
    assert conv.lib().fwc_abi_version() == conv.ABI_VERSION == 1
    assert re.search(r"#define\s+FWC_ABI_VERSION\s+1\b", open(HEADER).read())
    assert re.search(r"#define\s+FWC_CONJ_FILTER\s+1u\b", open(HEADER).read()) and conv.CONJ_FILTER == 1


def test_the_library_loads_on_first_use_not_with_the_package():
    code = ("import sys; sys.path.insert(0, %r); import fft_wgpu_amd as fw; "
            "assert fw.conv._lib is None; "
            "assert not any('amd_conv' in l for l in open('/proc/self/maps')); print('ok')" % ROOT)
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "ok"


def test_build_entry_builds_and_checks_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert text.count('os.path.join(ROOT, "fft_wgpu_amd", "conv")') == 1
    assert text.count("fwc_abi_version() == 1") == 1


def test_describe_answers_from_the_geometry(conv):
    """every n = 2 .. 4096 at batch 1, one full workgroup, and one full workgroup + 3 rows:
         n <= 32    256 threads, the two parked planes of k_chunk2d (2 * (8192 + 256) words), 8192 / n rows per workgroup,
                    blocks = ceil(batch * n / 8192)
         n >= 64    T = n / points threads per row, RT = 16 rows (8 at 4096), one plane of n * RT words, blocks = ceil(batch / RT)"""
    points = {64: 8, 128: 16, 256: 16}
    for n in cc.LENGTHS:
        rows = cc.rows_per_block(n)
        for batch in (1, rows, rows + 3):
            g = conv.describe(n, batch)
            assert sorted(g) == ["blocks", "lds_bytes", "rows_per_block", "threads"]
            if n <= 32:
                assert (g["threads"], g["rows_per_block"], g["lds_bytes"]) == (256, 8192 // n, 2 * (8192 + 256) * 4), (n, g)
                assert g["blocks"] == -(-batch * n // 8192), (n, batch, g)
            else:
                rt = 8 if n == 4096 else 16
                assert (g["threads"], g["rows_per_block"], g["lds_bytes"]) == (n // points.get(n, 32) * rt, rt, n * rt * 4), (n, g)
            assert 0 < g["lds_bytes"] <= 163840 and g["threads"] % 64 == 0 and g["threads"] <= 1024
            assert g["blocks"] == -(-batch // rows) == {1: 1, rows: 1, rows + 3: 2}[batch], (n, batch, g)


@pytest.mark.parametrize("n,status,word", [(0, INVALID_ARG, "power"), (3, INVALID_ARG, "power"), (1, UNSUPPORTED, "2 .. 4096"),
                                           (8192, UNSUPPORTED, "4096")])
def test_describe_refuses_other_lengths(conv, n, status, word):
    from fft_wgpu_amd import FwaError
    with pytest.raises(FwaError) as e:
        conv.describe(n)
    assert e.value.status == status and word in e.value.detail and "fft_len" in e.value.detail, e.value.detail
    for length, batch in ((4096, 1 << 36), (2, 1 << 44), (64, 1 << 36)):     # more than 2^31 - 1 workgroups
        with pytest.raises(FwaError) as e:
            conv.describe(length, batch)
        assert e.value.status == UNSUPPORTED and "workgroups" in e.value.detail
    assert conv.describe(4096, 8 * ((1 << 31) - 1))["blocks"] == (1 << 31) - 1      # the largest grid


def test_null_handles_are_rejected_without_a_device(conv):
    L = conv.lib()
    out = ctypes.c_void_p()
    v = ctypes.c_int64()
    assert L.fwc_plan_create(None, 1, 0, 64, None, None, None, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fwc_plan_create(None, 1, 0, 64, None, None, None, None) == INVALID_ARG
    assert L.fwc_plan_exec(None, None) == INVALID_ARG
    assert L.fwc_plan_get_i64(None, b"batch", ctypes.byref(v)) == INVALID_ARG
    assert L.fwc_plan_destroy(None) == 0
    assert L.fwc_describe(64, 1, None, None, None, None) == 0                # every output pointer is optional


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    src = tmp_path / "stale.c"
    src.write_text("int fwc_abi_version(void) { return 2; }\n")
    lib = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    code = ("import sys; sys.path.insert(0, %r); from fft_wgpu_amd import conv as m; m.LIB_PATH = %r\n"
            "try:\n    m.lib()\nexcept RuntimeError as e:\n    print('refused' if 'ABI version 2' in str(e) else e)\n"
            % (ROOT, str(lib)))
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "refused"


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text('#include "fft_wgpu_conv.hpp"\n'
                   "int run(uint32_t n, uint64_t b) {\n"
                   "  fft_wgpu::Device dev(0); fft_wgpu::Buffer x(dev, 8ull * n * b), h(dev, 8ull * n * 3), y(dev, 8ull * n * b);\n"
                   "  fft_wgpu::CommandEncoder enc(dev);\n"
                   "  fft_wgpu::conv::Convolve c(dev, dev, x, h, y, n);\n"
                   "  fft_wgpu::conv::Convolve in_place(dev, dev, x, h, x, n, true);\n"
                   "  fft_wgpu::conv::OnlyConvolve o(dev, dev, x, h, y, n, true);\n"
                   "  fft_wgpu::Buffer &r = c.proc(enc); in_place.proc(enc); o.proc(enc); enc.synchronize();\n"
                   "  return (&r == &y) + (int)c.get(\"filters\") + fft_wgpu::conv::describe(n, b).rows_per_block; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_cpp_mirror_refuses_a_library_of_another_abi_version(conv, tmp_path):
    """A host program built against the real libraries and RUN against stubs (LD_LIBRARY_PATH, as tests/test_abi.py does for
    the main library).  The stub of the main library makes a Device without a GPU (the current FWA_ABI_VERSION, a create
    that hands out a dummy handle); the stub of libfft_wgpu_amd_conv.so reports the given FWC_ABI_VERSION and has a
    fwc_plan_create that says so when it is reached and succeeds.  Version 2: the constructor throws
    Error(FWA_ERR_UNSUPPORTED) and create is not reached.  Version 1, the control: the same program reaches create."""
    main_version = int(re.search(r"#define FWA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "fft_wgpu_amd.h")).read()).group(1))
    host = tmp_path / "host.cpp"
    host.write_text('#include <cstdio>\n#include "fft_wgpu_conv.hpp"\n'
                    "int main() {\n"
                    "  fft_wgpu::Device dev(0);\n"
                    "  fft_wgpu::Buffer x(dev, reinterpret_cast<fwa_buf *>(0x100)), h(dev, reinterpret_cast<fwa_buf *>(0x200));   // borrowed handles\n"
                    '  try { fft_wgpu::conv::Convolve c(dev, dev, x, h, x, 64); std::puts("constructed"); }\n'
                    '  catch (const fft_wgpu::Error &e) { std::printf("refused status %d: %s\\n", (int)e.status, e.what()); }\n'
                    "  return 0; }\n")
    exe = tmp_path / "host"
    lib_dir = os.path.join(ROOT, "fft_wgpu_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(host), "-L" + lib_dir,
                           "-lfft_wgpu_amd_conv", "-lfft_wgpu_amd", "-pthread", "-Wl,-z,lazy", "-Wl,-rpath-link," + lib_dir, "-o", str(exe)])
    out = {}
    for version in (2, 1):
        d = tmp_path / ("stubs_v%d" % version)
        d.mkdir()
        (d / "main.c").write_text("#include <stdint.h>\n"
                                  "int32_t fwa_abi_version(void) { return %d; }\n"
                                  "int32_t fwa_ctx_create(int32_t ordinal, void **out) { (void)ordinal; *out = (void *)0x40; return 0; }\n"
                                  "int32_t fwa_ctx_destroy(void *c) { (void)c; return 0; }\n"
                                  'const char *fwa_last_error_string(const void *c) { (void)c; return ""; }\n' % main_version)
        (d / "conv.c").write_text("#include <stdint.h>\n#include <stdio.h>\n"
                                  "int32_t fwc_abi_version(void) { return %d; }\n"
                                  "int32_t fwc_plan_create(void *c, int32_t kind, uint32_t flags, uint32_t n, void *s, void *f, void *d, void **out)\n"
                                  '{ (void)c; (void)kind; (void)flags; (void)n; (void)s; (void)f; (void)d; puts("create reached"); *out = (void *)0x30; return 0; }\n'
                                  "int32_t fwc_plan_destroy(void *p) { (void)p; return 0; }\n" % version)
        for name, lib in (("main.c", "libfft_wgpu_amd.so"), ("conv.c", "libfft_wgpu_amd_conv.so")):
            subprocess.check_call(["gcc", "-shared", "-fPIC", str(d / name), "-o", str(d / lib)])
        r = subprocess.run([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=str(d)), capture_output=True, text=True)
        assert r.returncode == 0, (version, r.returncode, r.stdout, r.stderr)
        out[version] = r.stdout
    assert "refused status %d" % UNSUPPORTED in out[2] and "ABI version 2" in out[2] and "version 1" in out[2], out[2]
    assert "create reached" not in out[2] and "constructed" not in out[2], out[2]
    assert "create reached" in out[1] and "constructed" in out[1] and "refused" not in out[1], out[1]


def test_the_kernels_live_beside_the_other_libraries_and_change_none_of_them():
    for other in ("csrc", "strided", "fft2d", "real"):
        assert not os.path.exists(os.path.join(ROOT, "fft_wgpu_amd", other, "kernels_conv.hip"))
    assert sorted(f for f in os.listdir(CONV_DIR) if not f.endswith(".o")) == \
        ["Makefile", "conv.cpp", "conv_geom.h", "conv_kernels.h", "kernels_conv.hip"]
    hip = open(os.path.join(CONV_DIR, "kernels_conv.hip")).read()
    assert '#include "../csrc/device_common.h"' in hip and '#include "../strided/strided_net.h"' in hip
    for helper in ("void fft_reg(", "v2f cmul_tw(", "uint32_t xcd_map(", "hipError_t check_grid(", "hipError_t raise_lds_limit(",
                   "void stage(", "void exchange(", "v2f tw_n(", "uint32_t row_word(", "uint32_t chunk_word("):
        assert helper not in hip, helper
    assert "exchange<N, P, K.r0, 1, FIRST>" in hip and "network<N, INV, false>" in hip    # the inverse starts with the barrier
    for name in ("kernels_conv.hip", "conv_geom.h", "conv_kernels.h", "conv.cpp"):
        text = open(os.path.join(CONV_DIR, name)).read().lower()
        for banned in ("sinf(", "cosf(", "sincosf(", "rocfft", "mfma"):
            assert banned not in text, (name, banned)
    # csrc/, strided/, fft2d/ and real/ are what the commit before the convolution plans left (in a checkout with history):
    # every kernel, launcher and header.  The six plain-C++ host files of csrc/ that changed are excepted: their error paths were mended later,
    # when tests/test_host_faults.py made every HIP call fail once; the convolution plans share no line of them.  So are, by exact
    # path, the host file and the Makefile of strided/, fft2d/ and real/: the host checks and the build rules that every side library
    # stated for itself moved into fft_wgpu_amd/side/.  Every kernel unit, launcher, *_geom.h, *_kernels.h and strided_net.h stays
    # under the guard.
    host = [":(exclude)fft_wgpu_amd/csrc/%s.cpp" % f for f in ("ctx_streams", "buffers", "tables", "plan", "tuning", "comm")]
    host += [":(exclude)fft_wgpu_amd/%s" % f for f in ("strided/strided.cpp", "strided/Makefile", "fft2d/fft2d.cpp", "fft2d/Makefile",
                                                        "real/real.cpp", "real/Makefile")]
    if os.path.isdir(os.path.join(ROOT, ".git")):
        first = subprocess.run(["git", "-C", ROOT, "log", "--diff-filter=A", "--format=%H", "--", "fft_wgpu_amd/conv/conv_geom.h"],
                               capture_output=True, text=True).stdout.split()
        base = first[-1] + "^" if first else "HEAD"
        if subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", base], capture_output=True).returncode:
            return                                                            # a checkout without that commit's parent
        diff = subprocess.run(["git", "-C", ROOT, "diff", "--stat", base, "--", "fft_wgpu_amd/csrc", "fft_wgpu_amd/strided",
                               "fft_wgpu_amd/fft2d", "fft_wgpu_amd/real", *host], capture_output=True, text=True)
        assert diff.returncode == 0 and diff.stdout.strip() == "", diff.stdout + diff.stderr


# ---- the arithmetic: the complex64 model passes every numeric check of the GPU file, doctored results fail them --------
@pytest.mark.parametrize("n", cc.LENGTHS)
def test_the_model_passes_parity_and_the_cap(oracle, n):
    """parity: every n, both kinds, conj off and on, F = 3, both batches; the cap on >= 2^18 samples, F = 3"""
    bad = []
    for batch in (cc.default_batch(n), 1):
        x, H = cc.inputs(oracle, n, batch, 3)
        for kind in cc.KINDS:
            for conj in (False, True):
                ref = cc.cached_reference(oracle, n, batch, 3, kind, conj)
                bad += cc.parity_failures(oracle, cc.model(x, H, kind, conj), ref, "n %d %s conj %d batch %d" % (n, kind, conj, batch))
    batch = cc.cap_batch(n)
    x, H = cc.inputs(oracle, n, batch, 3)[0], cc.cap_filters(oracle, n)
    for conj in (False, True):
        ref = cc.reference(x, H, "Convolve", conj)
        bad += cc.cap_failures(cc.model(x, H, "Convolve", conj), ref, n, "n %d conj %d batch %d" % (n, conj, batch))
    assert not bad, "\n".join(bad)


def test_the_cap_is_the_rule_of_one_transform_over_both_and_the_multiply():
    for n in cc.LENGTHS:
        lg = n.bit_length() - 1
        assert cc.cap(n) == pytest.approx(cc.eb.C * 2.0 ** -24 * np.sqrt(2 * lg + 1), rel=1e-12)
        assert cc.eb.cap(n) < cc.cap(n) < 2 * cc.eb.cap(n)


@pytest.mark.parametrize("n", cc.ONEHOT_LENGTHS)
def test_the_model_passes_the_one_hot_sweep_and_a_shifted_filter_fails_it(n):
    x, H = cc.onehot_inputs(n)
    assert not cc.onehot_failures(cc.model(x, H, "Convolve", False), n)
    # the filter shifted by one bin: every row answers with the tone of the neighbouring bin
    assert cc.onehot_failures(cc.model(x, np.roll(H, 1, axis=1), "Convolve", False), n)
    if n > 2:                                                                 # ... or, for all rows but one, with nothing
        lost = np.roll(H, 1, axis=0)
        assert cc.onehot_failures(cc.model(x, lost, "Convolve", False), n)


@pytest.mark.parametrize("n", cc.SHAPES)
def test_the_model_passes_the_shifts(oracle, n):
    batch = cc.default_batch(n)
    x, _ = cc.inputs(oracle, n, batch, 3)
    bad = []
    for q in cc.shifts(n):
        y = cc.model(x, cc.shift_filter(n, q), "Convolve", False)
        bad += cc.parity_failures(oracle, y, np.roll(x, q, axis=1).astype(np.complex128), "n %d shift %d" % (n, q))
        wrong = cc.model(x, cc.shift_filter(n, (q + 1) % n), "Convolve", False)
        assert cc.parity_failures(oracle, wrong, np.roll(x, q, axis=1).astype(np.complex128), "n %d shift %d by %d" % (n, q, q + 1))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", cc.SHAPES)
def test_doctored_results_fail_parity(oracle, n):
    batch, F = cc.default_batch(n), 3
    x, H = cc.inputs(oracle, n, batch, F)
    for kind in cc.KINDS:
        for conj in (False, True):
            ref = cc.cached_reference(oracle, n, batch, F, kind, conj)
            what = "n %d %s conj %d" % (n, kind, conj)
            good = cc.model(x, H, kind, conj)
            assert not cc.parity_failures(oracle, good, ref, what)
            # the filter shifted by one bin
            assert cc.parity_failures(oracle, cc.model(x, np.roll(H, 1, axis=1), kind, conj), ref, what + ", filter shifted")
            # the filter row chosen as (b + 1) mod F
            assert cc.parity_failures(oracle, cc.model(x, H, kind, conj, row_of=lambda b: (b + 1) % F), ref, what + ", row b + 1")
            # conj ignored (or applied where it was not asked for)
            assert cc.parity_failures(oracle, cc.model(x, H, kind, conj, use_conj=not conj), ref, what + ", conj ignored")
            # one output sample off by 1e-4 of its row's maximum
            for b, j in ((0, 0), (batch - 1, n - 1), (batch // 2, n // 3)):
                y = good.copy()
                y[b, j] += np.float32(1e-4 * np.abs(ref[b]).max())
                assert cc.parity_failures(oracle, y, ref, what + ", one sample perturbed")
