"""CPU: the real-input plans' ABI (include/fft_wgpu_amd_real.h), host logic, mirrors and arithmetic -- no GPU needed.

fwr_describe is pure host logic: it is checked here for every n = 2 .. 4096, with the status codes of unsupported and
invalid lengths, and NULL handles are refused before any device is touched.  The two split formulas the kernels implement
(kernels_real.hip) are restated in numpy float64 and held to numpy.fft.rfft / irfft, and the bank-conflict degrees that
real_geom.h states are recomputed from the word maps.
"""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import side_libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fft_wgpu_amd_real.h")
REAL_DIR = os.path.join(ROOT, "fft_wgpu_amd", "real")
LENGTHS = [1 << lg for lg in range(1, 13)]
INVALID_ARG, UNSUPPORTED = 1, 6
NAMES = ["fwr_abi_version", "fwr_describe", "fwr_plan_create", "fwr_plan_destroy", "fwr_plan_exec", "fwr_plan_get_i64"]


@pytest.fixture(scope="session")
def real():
    """The library is built by the session that needs it (tests/conftest.py builds csrc only)."""
    return side_libs.load("real")


@pytest.fixture(scope="session")
def strided(real):
    return side_libs.load("strided")


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd_real.h"\n'
                   "int use(fwa_ctx *c, fwa_buf *a, fwa_buf *b) { fwr_plan *p = 0; int32_t th, l, r; uint64_t bl; int64_t v;\n"
                   "  if (fwr_describe(1024, 19, &th, &l, &r, &bl)) return 1;\n"
                   "  if (fwr_plan_create(c, FWA_INVERSE_SCALED, 1024, a, b, &p)) return 2;\n"
                   '  if (fwr_plan_get_i64(p, "blocks", &v)) return 3;\n'
                   "  return fwr_plan_exec(p, 0) + fwr_plan_destroy(p) + (fwr_abi_version() != FWR_ABI_VERSION); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_binding_names_exactly_the_declared_functions(real):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fwr_[a-z0-9_]+)\s*\(", text))) == NAMES
    assert sorted(real._SIGNATURES) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", real.LIB_PATH], text=True)
    assert sorted(set(re.findall(r"\bT (fwr_[a-z0-9_]+)$", out, flags=re.M))) == NAMES
    assert not re.findall(r"\bT (fw[as2]_[a-z0-9_]+)$", out, flags=re.M)      # the main library's calls are linked, not restated
    needed = subprocess.check_output(["readelf", "-d", real.LIB_PATH], text=True)
    assert "libfft_wgpu_amd.so" in needed and "strided" not in needed and "amd_2d" not in needed
    assert real.lib().fwr_abi_version() == real.ABI_VERSION == 1


def test_the_library_loads_on_first_use_not_with_the_package():
    code = ("import sys; sys.path.insert(0, %r); import fft_wgpu_amd as fw; "
            "assert fw.real._lib is None; "
            "assert not any('amd_real' in l for l in open('/proc/self/maps')); print('ok')" % ROOT)
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "ok"


def test_describe_answers_from_the_geometry(real, strided):
    """every n = 2 .. 4096, batch 1, 19, 259 and 2^18 + 16:
         n <= 64    256 threads, 256 rows per workgroup, LDS = 256 (n + 3) words (the padded spectrum parking)
         n >= 128   threads, LDS and rows per workgroup (= tile_cols) of the strided geometry of M = n / 2
       blocks = ceil(batch / rows_per_block)."""
    for n in LENGTHS:
        for batch in (1, 19, 259, (1 << 18) + 16):
            g = real.describe(n, batch)
            assert sorted(g) == ["blocks", "lds_bytes", "rows_per_block", "threads"]
            if n <= 64:
                assert (g["threads"], g["rows_per_block"], g["lds_bytes"]) == (256, 256, 256 * (n + 3) * 4), (n, g)
            else:
                s = strided.describe(n // 2, 16)
                assert (g["threads"], g["rows_per_block"], g["lds_bytes"]) == (s["threads"], s["tile_cols"], s["lds_bytes"]), (n, g)
                assert g["rows_per_block"] == 16 and g["lds_bytes"] == (n // 2) * 16 * 4
            assert 0 < g["lds_bytes"] <= 163840 and g["threads"] % 64 == 0
            assert g["blocks"] == -(-batch // g["rows_per_block"]), (n, batch, g)


@pytest.mark.parametrize("n,status,word", [(0, INVALID_ARG, "power"), (3, INVALID_ARG, "power"), (1, UNSUPPORTED, "2 .. 4096"),
                                           (8192, UNSUPPORTED, "4096")])
def test_describe_refuses_other_lengths(real, n, status, word):
    from fft_wgpu_amd import FwaError
    with pytest.raises(FwaError) as e:
        real.describe(n)
    assert e.value.status == status and word in e.value.detail and "fft_len" in e.value.detail, e.value.detail
    with pytest.raises(FwaError) as e:                                       # more than 2^31 - 1 workgroups
        real.describe(4096, 1 << 36)
    assert e.value.status == UNSUPPORTED and "workgroups" in e.value.detail


def test_null_handles_are_rejected_without_a_device(real):
    L = real.lib()
    out = ctypes.c_void_p()
    v = ctypes.c_int64()
    assert L.fwr_plan_create(None, 0, 64, None, None, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fwr_plan_create(None, 0, 64, None, None, None) == INVALID_ARG
    assert L.fwr_plan_exec(None, None) == INVALID_ARG
    assert L.fwr_plan_get_i64(None, b"batch", ctypes.byref(v)) == INVALID_ARG
    assert L.fwr_plan_destroy(None) == 0
    assert L.fwr_describe(64, 1, None, None, None, None) == 0                # every output pointer is optional


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    src = tmp_path / "stale.c"
    src.write_text("int fwr_abi_version(void) { return 0; }\n")
    lib = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    code = ("import sys; sys.path.insert(0, %r); from fft_wgpu_amd import real as m; m.LIB_PATH = %r\n"
            "try:\n    m.lib()\nexcept RuntimeError as e:\n    print('refused' if 'ABI version 0' in str(e) else e)\n"
            % (ROOT, str(lib)))
    assert subprocess.check_output(["python", "-c", code], text=True).strip() == "refused"


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text('#include "fft_wgpu_real.hpp"\n'
                   "int run(uint32_t n, uint64_t b) {\n"
                   "  fft_wgpu::Device dev(0); fft_wgpu::Buffer x(dev, 4ull * n * b), s(dev, 8ull * (n / 2 + 1) * b);\n"
                   "  fft_wgpu::CommandEncoder enc(dev);\n"
                   "  fft_wgpu::real::Forward f(dev, dev, x, s, n);\n"
                   "  fft_wgpu::real::Inverse i(dev, dev, s, x, n);\n"
                   "  fft_wgpu::real::Onlyinverse o(dev, dev, s, x, n);\n"
                   "  fft_wgpu::Buffer &y = f.proc(enc); i.proc(enc); o.proc(enc); enc.synchronize();\n"
                   "  return (&y == &s) + (int)f.get(\"blocks\") + fft_wgpu::real::describe(n, b).rows_per_block; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_kernels_live_beside_the_other_libraries_and_change_none_of_them():
    for other in ("csrc", "strided", "fft2d"):
        assert not os.path.exists(os.path.join(ROOT, "fft_wgpu_amd", other, "kernels_real.hip"))
    assert sorted(f for f in os.listdir(REAL_DIR) if not f.endswith(".o")) == \
        ["Makefile", "kernels_real.hip", "real.cpp", "real_geom.h", "real_kernels.h"]
    hip = open(os.path.join(REAL_DIR, "kernels_real.hip")).read()
    assert '#include "../csrc/device_common.h"' in hip and '#include "../strided/strided_net.h"' in hip
    for helper in ("void fft_reg(", "v2f cmul_tw(", "uint32_t xcd_map(", "hipError_t check_grid(", "hipError_t raise_lds_limit(",
                   "void stage(", "void exchange(", "v2f tw_n(", "uint32_t row_word("):
        assert helper not in hip, helper
    for name in ("kernels_real.hip", "real_geom.h", "real_kernels.h", "real.cpp"):
        text = open(os.path.join(REAL_DIR, name)).read().lower()
        for banned in ("sinf(", "cosf(", "sincosf(", "rocfft", "mfma"):
            assert banned not in text, (name, banned)
    # csrc/, strided/ and fft2d/ are what the commit before the real plans left (in a checkout with history): every kernel,
    # launcher and header.  The six plain-C++ host files of csrc/ that changed are excepted: their error paths were mended later, when
    # tests/test_host_faults.py made every HIP call fail once; the real plans share no line of them.  So are, by exact path, the
    # host file and the Makefile of strided/ and fft2d/: the host checks and the build rules that every side library stated for
    # itself moved into fft_wgpu_amd/side/.  Every kernel unit, launcher, *_geom.h, *_kernels.h and strided_net.h stays under the guard.
    host = [":(exclude)fft_wgpu_amd/csrc/%s.cpp" % f for f in ("ctx_streams", "buffers", "tables", "plan", "tuning", "comm")]
    host += [":(exclude)fft_wgpu_amd/%s" % f for f in ("strided/strided.cpp", "strided/Makefile", "fft2d/fft2d.cpp", "fft2d/Makefile")]
    if os.path.isdir(os.path.join(ROOT, ".git")):
        first = subprocess.run(["git", "-C", ROOT, "log", "--diff-filter=A", "--format=%H", "--", "fft_wgpu_amd/real/real_geom.h"],
                               capture_output=True, text=True).stdout.split()
        base = first[-1] + "^" if first else "HEAD"
        if subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", base], capture_output=True).returncode:
            return                                                            # a checkout without that commit's parent
        diff = subprocess.run(["git", "-C", ROOT, "diff", "--stat", base, "--", "fft_wgpu_amd/csrc", "fft_wgpu_amd/strided",
                               "fft_wgpu_amd/fft2d", *host], capture_output=True, text=True)
        assert diff.returncode == 0 and diff.stdout.strip() == "", diff.stdout + diff.stderr


# ---- the arithmetic -------------------------------------------------------------------------------------------------
def model_rfft(x):
    """kernels_real.hip, forward, in float64: rows of n reals -> rows of n / 2 + 1 bins"""
    n = x.shape[-1]
    M = n // 2
    Z = np.fft.fft(x[..., 0::2] + 1j * x[..., 1::2], axis=-1)
    k = np.arange(M)
    Zr = Z[..., (M - k) % M]
    E, O = (Z + np.conj(Zr)) / 2, (Z - np.conj(Zr)) / 2j
    X = np.empty(x.shape[:-1] + (M + 1,), dtype=np.complex128)
    X[..., :M] = E + np.exp(-2j * np.pi * k / n) * O
    X[..., M] = Z[..., 0].real - Z[..., 0].imag
    return X


def model_irfft_unscaled(X, n):
    """kernels_real.hip, inverse, in float64: rows of n / 2 + 1 bins -> rows of n reals = n * irfft"""
    M = n // 2
    X = X.copy()
    X[..., 0] = X[..., 0].real                             # Im X[0], Im X[M]: replaced by 0, never multiplied
    X[..., M] = X[..., M].real
    k = np.arange(M)
    Xr = X[..., M - k]
    Zp = (X[..., :M] + np.conj(Xr)) + 1j * np.exp(2j * np.pi * k / n) * (X[..., :M] - np.conj(Xr))
    z = np.fft.ifft(Zp, axis=-1) * M
    x = np.empty(X.shape[:-1] + (n,))
    x[..., 0::2], x[..., 1::2] = z.real, z.imag
    return x


@pytest.mark.parametrize("n", LENGTHS)
def test_the_split_formulas_equal_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (5, n))
    want = np.fft.rfft(x, axis=-1)
    assert np.abs(model_rfft(x) - want).max() <= 1e-13 * np.abs(want).max()
    # arbitrary, non-Hermitian input with garbage in the two imaginary parts numpy ignores too
    X = rng.uniform(-1, 1, (5, n // 2 + 1)) + 1j * rng.uniform(-1, 1, (5, n // 2 + 1))
    want = n * np.fft.irfft(X, n, axis=-1)
    for garbage in (0.0, 123.0, np.nan, np.inf):
        G = X.copy()
        G.imag[:, 0] = garbage
        G.imag[:, -1] = garbage
        got = model_irfft_unscaled(G, n)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), garbage


# ---- the bank-conflict degrees of real_geom.h -----------------------------------------------------------------------
NETS = {6: (8, 8, 1, 8, 16), 7: (16, 8, 1, 16, 16), 8: (16, 16, 1, 16, 16), 9: (32, 16, 1, 32, 16), 10: (32, 32, 1, 32, 16),
        11: (32, 32, 2, 32, 16)}                         # fws::net_of: r0, r1, r2, points, tile_cols
SWIZZLES = {6: (3, 7, 8), 7: (4, 7, 8), 8: (3, 31, 17), 9: (4, 31, 17)}          # fw2::row_swizzle; otherwise (5, 31, 0)


def row_word(lg, cols, r, d):
    a, m, k = SWIZZLES.get(lg, (5, 31, 0))
    return r * cols + (d ^ ((((d >> a) & m) ^ (r * k)) & 31))


def degree(word_of_lane, lanes):
    """the largest number of distinct words on one bank (word mod 32) within one 32-lane half of a wave, over the workgroup"""
    worst = 0
    for h in range(0, lanes, 32):
        banks = collections.defaultdict(set)
        for tid in range(h, h + 32):
            w = word_of_lane(tid)
            banks[w % 32].add(w)
        worst = max(worst, max(len(s) for s in banks.values()))
    return worst


def k_real_degrees(lgm):
    M = 1 << lgm
    r0, r1, r2, P, RT = NETS[lgm]
    T = M // P
    lanes = T * RT

    def word(tid, d):
        return row_word(lgm, M, tid // T, d)

    def dest(t, g, q, R, J):                             # fws::exchange
        idx = t + T * g
        j = idx & (J - 1)
        return (idx - j) * R + j + q * J
    writes = max(degree(lambda tid: word(tid, dest(tid % T, g, q, R, J)), lanes)
                 for R, J in [(r0, 1)] + ([(r1, r0)] if r2 > 1 else []) for g in range(P // R) for q in range(R))
    natural = max(degree(lambda tid: word(tid, tid % T + T * m), lanes) for m in range(P))
    mirrored = max(degree(lambda tid: word(tid, (M - (tid % T + T * m)) % M), lanes) for m in range(P))
    return [writes, natural, mirrored]


def small_degrees(n):
    M = n // 2
    rw, sw = (lambda w: w + w // n), (lambda w: w + w // (n + 2))                # small_real_word, small_spec_word
    return [max(degree(lambda tid: rw(2 * (tid + 256 * i) + b), 256) for i in range(M) for b in (0, 1)),
            max(degree(lambda tid: rw(tid * n + j), 256) for j in range(n)),
            max(degree(lambda tid: sw(tid * (n + 2) + j), 256) for j in range(n + 2)),
            max(degree(lambda tid: sw(2 * (tid + 256 * i) + b), 256) for i in range(M + 1) for b in (0, 1))]


def stated_tables():
    """the two tables of the header comment of real_geom.h: {n: [degrees, in row order]}"""
    text = open(os.path.join(REAL_DIR, "real_geom.h")).read()
    tables = []
    for head in re.finditer(r"^//   n\s+((?:\d+\s*)+)$", text, flags=re.M):
        ns = [int(v) for v in head.group(1).split()]
        rows = []
        for line in text[head.end():].split("\n")[1:]:
            m = re.match(r"^//   [a-z].*?((?:\s+\d+){%d})\s*$" % len(ns), line)
            if m:
                rows.append([int(v) for v in m.group(1).split()])
            elif not re.match(r"^//    ", line):
                break
        tables.append({n: [row[i] for row in rows] for i, n in enumerate(ns)})
    return tables


def test_the_stated_bank_conflict_degrees_are_the_computed_ones():
    small, rows = stated_tables()
    assert sorted(small) == [2, 4, 8, 16, 32, 64] and sorted(rows) == [128, 256, 512, 1024, 2048, 4096]
    for n, stated in small.items():
        assert stated == small_degrees(n), n
        assert stated[1] == stated[2] == 1                                   # the per-thread row accesses are conflict-free
    for n, stated in rows.items():
        assert stated == k_real_degrees(n.bit_length() - 2), n
    # the maps are those of real_geom.h and fft2d_geom.h, and the networks those of strided_geom.h
    geom = open(os.path.join(REAL_DIR, "real_geom.h")).read()
    assert "return w + w / n;" in geom and "return w + w / (n + 2);" in geom
    fw2 = open(os.path.join(ROOT, "fft_wgpu_amd", "fft2d", "fft2d_geom.h")).read()
    assert "return r * cols + (d ^ ((((d >> s.a) & (uint32_t)s.m) ^ (r * (uint32_t)s.k)) & 31u));" in fw2
    for lg, (a, m, k) in SWIZZLES.items():
        assert "lg_cols == %d ? RowSwizzle{%d, %d, %d}" % (lg, a, m, k) in fw2
    net = open(os.path.join(ROOT, "fft_wgpu_amd", "strided", "strided_geom.h")).read()
    for lg, v in NETS.items():
        assert "lg_n == %d ? Net{%s}" % (lg, ", ".join(str(i) for i in v)) in net
