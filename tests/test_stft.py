"""CPU: the framed real-input plans' ABI (include/fft_wgpu_amd_stft.h), host logic, mirrors and arithmetic -- no GPU needed.

fwt_describe is pure host logic: it is checked here for every n = 2 .. 4096 over a grid of hops, signal lengths and signal
counts, with the status code of every refusal, and NULL handles are refused before any device is touched.  The numpy
complex64 model of the algorithm (tests/stft_cases.py) passes every numeric check tests/test_gpu_stft.py applies to the GPU,
on the same inputs, and each of its mutants fails one; the bank-conflict degrees stft_geom.h states are recomputed from the
word maps.
"""
import collections
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import stft_cases as sc
from conftest import GOLDEN
import side_libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fft_wgpu_amd_stft.h")
STFT_DIR = os.path.join(ROOT, "fft_wgpu_amd", "stft")
INVALID_ARG, UNSUPPORTED = 1, 6
NAMES = ["fwt_abi_version", "fwt_describe", "fwt_plan_create", "fwt_plan_destroy", "fwt_plan_exec", "fwt_plan_get_i64"]


@pytest.fixture(scope="session")
def stft():
    """The library is built by the session that needs it (tests/conftest.py builds csrc only)."""
    return side_libs.load("stft")


@pytest.fixture(scope="session")
def real():
    return side_libs.load("real")


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd_stft.h"\n'
                   "int use(fwa_ctx *c, fwa_buf *a, fwa_buf *w, fwa_buf *b) { fwt_plan *p = 0; int32_t th, l, r; uint64_t f, bl; int64_t v;\n"
                   "  if (fwt_describe(1024, 256, 48000, 2, &f, &th, &l, &r, &bl)) return 1;\n"
                   "  if (fwt_plan_create(c, FWT_POWER, 1024, 256, 48000, a, w, b, &p)) return 2;\n"
                   '  if (fwt_plan_get_i64(p, "frames", &v)) return 3;\n'
                   "  return fwt_plan_exec(p, 0) + fwt_plan_destroy(p) + (fwt_abi_version() != FWT_ABI_VERSION) + FWT_SPECTRUM; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_binding_names_exactly_the_declared_functions(stft):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fwt_[a-z0-9_]+)\s*\(", text))) == NAMES
    assert sorted(stft._SIGNATURES) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", stft.LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (fwt_[a-z0-9_]+)$", out, flags=re.M))) == NAMES
    assert not re.findall(r"\bT (fw[as2rc]_[a-z0-9_]+)$", out, flags=re.M)     # the other libraries' calls are linked, not restated
    needed = subprocess.check_output(["readelf", "-d", stft.LIB_PATH], text=True)
    assert "libfft_wgpu_amd.so" in needed
    for other in ("strided", "amd_2d", "amd_real", "amd_conv"):               # what it takes from them is header-only
        assert other not in needed
    assert stft.lib().fwt_abi_version() == stft.ABI_VERSION == 1
    assert "#define FWT_SPECTRUM 0" in text and "#define FWT_POWER 1" in text and (stft.SPECTRUM, stft.POWER) == (0, 1)


def test_the_library_loads_on_first_use_not_with_the_package():
    code = ("import sys; sys.path.insert(0, %r); import fft_wgpu_amd as fw; "
            "assert fw.stft._lib is None; "
            "assert not any('amd_stft' in l for l in open('/proc/self/maps')); print('ok')" % ROOT)
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "ok"


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    src = tmp_path / "stale.c"
    src.write_text("int fwt_abi_version(void) { return 0; }\n")
    lib = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    code = ("import sys; sys.path.insert(0, %r); from fft_wgpu_amd import stft as m; m.LIB_PATH = %r\n"
            "try:\n    m.lib()\nexcept RuntimeError as e:\n    print('refused' if 'ABI version 0' in str(e) else e)\n"
            % (ROOT, str(lib)))
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "refused"


CPP_USER = ('#include "fft_wgpu_stft.hpp"\n'
            "int run(uint32_t n, uint32_t hop, uint64_t len, uint64_t s) {\n"
            "  const fft_wgpu::stft::Geometry g = fft_wgpu::stft::describe(n, hop, len, s);\n"
            "  fft_wgpu::Device dev(0); fft_wgpu::Buffer x(dev, 4ull * len * s), w(dev, 4ull * n);\n"
            "  fft_wgpu::Buffer y(dev, 8ull * (n / 2 + 1) * s * g.frames_per_signal), p(dev, 4ull * (n / 2 + 1) * s * g.frames_per_signal);\n"
            "  fft_wgpu::CommandEncoder enc(dev);\n"
            "  fft_wgpu::stft::Spectrum a(dev, dev, x, y, n, hop, len, &w);\n"
            "  fft_wgpu::stft::Power b(dev, dev, x, p, n, hop, len);\n"
            "  fft_wgpu::Buffer &r = a.proc(enc); b.proc(enc); enc.synchronize();\n"
            "  return (&r == &y) + (int)a.get(\"frames\") + g.frames_per_block; }\n")


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text(CPP_USER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_cpp_mirror_checks_the_abi_version_before_it_creates_a_plan():
    hpp = open(os.path.join(ROOT, "include", "fft_wgpu_stft.hpp")).read()
    ctor = hpp[hpp.index("Plan(const Device &d"):hpp.index("~Plan()")]
    assert ctor.index("fwt_abi_version()") < ctor.index("throw Error(FWA_ERR_UNSUPPORTED") < ctor.index("fwt_plan_create(")
    assert "got != FWT_ABI_VERSION" in ctor


def test_null_handles_are_rejected_without_a_device(stft):
    L = stft.lib()
    out = ctypes.c_void_p()
    v = ctypes.c_int64()
    assert L.fwt_plan_create(None, 0, 64, 16, 640, None, None, None, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fwt_plan_create(None, 0, 64, 16, 640, None, None, None, None) == INVALID_ARG
    assert L.fwt_plan_exec(None, None) == INVALID_ARG
    assert L.fwt_plan_get_i64(None, b"frames", ctypes.byref(v)) == INVALID_ARG
    assert L.fwt_plan_destroy(None) == 0
    assert L.fwt_describe(64, 16, 640, 1, None, None, None, None, None) == 0   # every output pointer is optional


# ---- geometry -------------------------------------------------------------------------------------------------------
def test_describe_answers_from_the_formulas(stft, real):
    for n in sc.LENGTHS:
        r = real.describe(n, 1)
        for hop in sc.hops(n):
            for L in (n, n + 1, 2 * n - 1, 5 * hop + n + 2):
                for signals in (1, 7):
                    g = stft.describe(n, hop, L, signals)
                    assert sorted(g) == ["blocks", "frames_per_block", "frames_per_signal", "lds_bytes", "threads"]
                    F = 1 + (L - n) // hop
                    assert g["frames_per_signal"] == F == sc.frames_per_signal(n, hop, L), (n, hop, L, g)
                    assert (g["threads"], g["lds_bytes"], g["frames_per_block"]) == (r["threads"], r["lds_bytes"], r["rows_per_block"])
                    assert g["frames_per_block"] == (256 if n <= 64 else 16)
                    assert g["blocks"] == -(-signals * F // g["frames_per_block"]), (n, hop, L, signals, g)
    assert stft.describe(4096, 1, 4095 + (1 << 18) + 16, 1)["blocks"] == (1 << 14) + 1
    assert stft.describe(2, 1 << 31, (1 << 40) + 2, 3)["frames_per_signal"] == 1 + (1 << 9)     # hop may exceed n, L 2^32


@pytest.mark.parametrize("args,status,word", [
    ((0, 1, 8, 1), INVALID_ARG, "power"), ((3, 1, 8, 1), INVALID_ARG, "power"), ((48, 1, 64, 1), INVALID_ARG, "power"),
    ((1, 1, 8, 1), UNSUPPORTED, "2 .. 4096"), ((8192, 1, 8192, 1), UNSUPPORTED, "4096"),
    ((64, 0, 64, 1), INVALID_ARG, "hop"), ((64, 16, 63, 1), INVALID_ARG, "signal_len"),
    ((64, 16, 1 << 62, 1), INVALID_ARG, "overflows"), ((64, 1, 1 << 40, 1 << 21), INVALID_ARG, "overflows"),
    ((4096, 1, 1 << 36, 1), UNSUPPORTED, "workgroups"), ((2, 1, 1 << 20, 1 << 20), UNSUPPORTED, "workgroups")])
def test_describe_refuses(stft, args, status, word):
    from fft_wgpu_amd import FwaError
    with pytest.raises(FwaError) as e:
        stft.describe(*args)
    assert e.value.status == status and word in e.value.detail, e.value.detail


def test_the_kernels_live_beside_the_other_libraries_and_change_none_of_them():
    for other in ("csrc", "strided", "fft2d", "real", "conv"):
        assert not os.path.exists(os.path.join(ROOT, "fft_wgpu_amd", other, "kernels_stft.hip"))
    assert sorted(f for f in os.listdir(STFT_DIR) if not f.endswith(".o")) == \
        ["Makefile", "kernels_stft.hip", "stft.cpp", "stft_geom.h", "stft_kernels.h"]
    hip = open(os.path.join(STFT_DIR, "kernels_stft.hip")).read()
    assert '#include "../csrc/device_common.h"' in hip and '#include "../strided/strided_net.h"' in hip
    for helper in ("void fft_reg(", "v2f cmul_tw(", "uint32_t xcd_map(", "hipError_t check_grid(", "hipError_t raise_lds_limit(",
                   "void stage(", "void exchange(", "v2f tw_n(", "uint32_t row_word("):
        assert helper not in hip, helper
    for name in ("kernels_stft.hip", "stft_geom.h", "stft_kernels.h", "stft.cpp"):
        text = open(os.path.join(STFT_DIR, name)).read().lower()
        for banned in ("sinf(", "cosf(", "sincosf(", "rocfft", "mfma", "aux_default"):
            assert banned not in text, (name, banned)
    # the signal and the window are read through plain pointers (default cache policy), never through an AUX_NT descriptor
    assert "buf_load" not in hip and hip.count("AUX_NT") == hip.count("<AUX_NT>")
    geom = open(os.path.join(STFT_DIR, "stft_geom.h")).read()
    assert "#include <hip" not in geom and "__device__" not in geom and "__global__" not in geom    # HIP-free: g++ reads it
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(STFT_DIR, "stft_geom.h")])


# ---- the bank-conflict degrees of stft_geom.h -----------------------------------------------------------------------
def degree(word_of_lane, lanes=256):
    """the largest number of distinct words on one bank (word mod 32) within one 32-lane half of a wave, over the workgroup"""
    worst = 0
    for h in range(0, lanes, 32):
        banks = collections.defaultdict(set)
        for tid in range(h, h + 32):
            w = word_of_lane(tid)
            banks[w % 32].add(w)
        worst = max(worst, max(len(s) for s in banks.values()))
    return worst


def power_degrees(n):
    W = n // 2 + 1
    stride = W | 1
    pw = lambda w: w + (w // W) * (stride - W)                               # small_power_word
    assert all(pw(t * W + j) == t * stride + j for t in (0, 1, 77, 255) for j in range(W))   # the span word of (row, column)
    return [max(degree(lambda tid: tid * stride + j) for j in range(W)),
            max(degree(lambda tid: pw(tid + 256 * i)) for i in range(W))]


def test_the_stated_bank_conflict_degrees_are_the_computed_ones():
    text = open(os.path.join(STFT_DIR, "stft_geom.h")).read()
    head = re.search(r"^//   n\s+((?:\d+\s*)+)$", text, flags=re.M)
    ns = [int(v) for v in head.group(1).split()]
    assert ns == [2, 4, 8, 16, 32, 64]
    rows = []
    for line in text[head.end():].split("\n")[1:]:
        m = re.match(r"^//   power.*?((?:\s+\d+){6})\s*$", line)
        if not m:
            break
        rows.append([int(v) for v in m.group(1).split()])
    assert len(rows) == 2
    for i, n in enumerate(ns):
        assert [rows[0][i], rows[1][i]] == power_degrees(n), n
        assert rows[0][i] == 1 and ((n // 2 + 1) | 1) % 2 == 1 and ((n // 2 + 1) | 1) <= n + 3    # odd stride, inside the spectrum parking
    assert "return (n / 2 + 1) | 1u;" in text
    assert "return w + (w / (n / 2 + 1)) * (small_power_stride(n) - (n / 2 + 1));" in text


# ---- the model passes the GPU file's checks -------------------------------------------------------------------------
def run_model(output, x, n, hop, w, mutant=None):
    return sc.model(output, x, n, hop, w, mutant=mutant)


@pytest.mark.parametrize("n", sc.LENGTHS)
def test_model_parity(oracle, n):
    bad = []
    for hop, signals, L, windowed in sc.parity_shapes(n):
        bad += sc.check_parity(run_model, oracle, n, hop, signals, L, sc.hann(n) if windowed else None)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", sc.LENGTHS)
def test_model_budget(n):
    for name, w in (("hann", sc.hann(n)), ("random", sc.random_window(n))):
        rel_l2, bad, _ = sc.check_budget(run_model, n, w, name)
        assert rel_l2 <= sc.cap(n) and not bad, "\n".join(bad)


@pytest.mark.parametrize("n", sc.LENGTHS)
def test_model_power_sweep_and_special_values(n):
    hop, signals, L = sc.default_shape(n)
    bad = sc.check_power(run_model, n, hop, signals, L, sc.hann(n)) + sc.check_power(run_model, n, hop, signals, L, None)
    bad += sc.check_sweep(run_model, n)
    if n in (2, 16, 128, 1024):
        bad += sc.check_special_values(run_model, n, "Spectrum") + sc.check_special_values(run_model, n, "Power")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", [8, 64, 128, 4096])
@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_every_mutant_fails(oracle, n, mutant):
    hop, signals, L = sc.default_shape(n)
    w = sc.hann(n)
    run = lambda output, x, n_, hop_, w_: sc.model(output, x, n_, hop_, w_, mutant=mutant)
    if mutant == "power_mirror":
        assert not sc.check_parity(run, oracle, n, hop, signals, L, w)       # the bins themselves are right
        assert sc.check_power(run, n, hop, signals, L, w)
    else:
        assert sc.check_parity(run, oracle, n, hop, signals, L, w), mutant


# ---- why cap(2 n) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_the_window_product_fits_under_the_cap_with_the_recorded_error_of_the_real_plans(n):
    """The f32 product w * x is one rounding; its effect on the spectrum is measured here in float64 (rfft of the f32 product
    against rfft of the float64 product).  Its rounding errors are independent of the transform's, so the two rel-L2 figures add
    in quadrature: with what real.Forward left on record (tests/golden/real_error.json: whole-buffer rel-L2 and worst class) the
    sum stays at <= 0.60 of cap(2 n) over the buffer and <= 0.67 on the worst class, with the Hann window and with a random one."""
    rec = json.load(open(os.path.join(GOLDEN, "real_error.json")))["cases"]["%d/Forward" % n]
    hop, signals, L = sc.budget_shape(n)
    x = sc.signals_input(n, hop, signals, L)
    fr = sc.frames_of(x, n, hop)
    for name, w in (("hann", sc.hann(n)), ("random", sc.random_window(n))):
        exact = np.fft.rfft(fr.astype(np.float64) * w.astype(np.float64), axis=-1)
        rounded = np.fft.rfft((fr * w).astype(np.float64), axis=-1)
        product = float(np.sqrt((np.abs(rounded - exact) ** 2).sum() / (np.abs(exact) ** 2).sum()))
        whole = float(np.hypot(product, rec["rel_l2"])) / sc.cap(n)
        worst = float(np.hypot(product, rec["per_class_max_of_cap"] * rec["cap"])) / sc.cap(n)
        print("n %d %s: product rel_l2 %.4g, with real.Forward's record %.3f of cap(2n), worst class %.3f" % (n, name, product, whole, worst))
        assert whole <= 0.60 and worst <= 0.67, (n, name, whole, worst)
