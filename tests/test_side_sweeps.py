"""not-gpu: the checks of tests/side_sweeps.py bite, and the sweeps name every kernel the four side libraries can dispatch.

A numpy complex64 model of the shared register network, written from the comment of fft_wgpu_amd/strided/strided_net.h:
Stockham stages r0 x r1 (x r2); a stage of radix R with sub-block size J reads x[idx + m n / R], and writes output q of
butterfly idx to element (idx - j) R + j + q J, j = idx mod J, times W_n^((idx - j) q); W_n^e is entry e * 4096 / n of the
table float32(cos / sin(2 pi k / 4096)), k < 2048, negated for the upper half; the inverse conjugates.  The R-point butterflies
are numpy.fft on complex64, which runs in fp32.  Fed the sweep inputs of every n >= 64 the model passes every sweep bound --
the evidence that fp32 arithmetic of this shape stays inside the bounds at EVERY position --, numpy.fft on complex64 does
the same for n <= 32 and serves the class check.  Doctored results fail, each with a message naming the right place.
"""
import os
import re

import numpy as np
import pytest

import conv_cases as cc
import side_sweeps as ss
from conftest import ROOT
from oracle import error_budget as eb
from test_error_budget import _model_fft

TABLE = (np.cos(2 * np.pi * np.arange(2048) / 4096).astype(np.float32)
         - 1j * np.sin(2 * np.pi * np.arange(2048) / 4096).astype(np.float32)).astype(np.complex64)


def tw(n, e, table=TABLE, off=None):
    """W_n^e, 0 <= e < n; off: integer array like e, added to the table index (a doctored look-up)"""
    i = e * (4096 // n)
    if off is not None:
        i = i + off
    w = table[i & 2047]
    return np.where((i & 2048) != 0, -w, w)


def network(x, sign, doctor=None, table=TABLE):
    """The r0 x r1 (x r2) network of the last axis of x (complex64, n >= 64).  doctor = (stage, t, q, entries): the
    twiddle of output q of the butterflies of thread t in that stage is looked up `entries` table entries off."""
    n = x.shape[-1]
    r0, r1, r2, points, _ = ss.NETS[ss.lg2(n)]
    T = n // points
    lead = x.shape[:-1]
    assert x.dtype == np.complex64
    J = 1
    for s, R in enumerate(r for r in (r0, r1, r2) if r > 1):
        idx = np.arange(n // R)
        v = x.reshape(lead + (R, n // R))                                   # v[m, idx] = x[idx + m n / R]
        v = np.fft.fft(v, axis=-2) if sign < 0 else np.conj(np.fft.fft(np.conj(v), axis=-2))
        assert v.dtype == np.complex64
        j = idx % J
        if J * R < n:
            q = np.arange(R)[:, None]
            off = None
            if doctor is not None and doctor[0] == s:
                off = np.where((q == doctor[2]) & ((idx % T) == doctor[1])[None, :], doctor[3], 0)
            w = tw(n, (idx - j)[None, :] * q, table, off)
            v = v * (w if sign < 0 else np.conj(w))
        # idx = a J + j: output q goes to element a J R + q J + j
        x = np.ascontiguousarray(np.swapaxes(v.reshape(lead + (R, n // (R * J), J)), -3, -2)).reshape(lead + (n,))
        J *= R
    return x


def fft32(x, sign, axis=-1):
    """numpy.fft on complex64 (fp32 inside), unscaled either way"""
    y = np.fft.fft(x, axis=axis) if sign < 0 else np.conj(np.fft.fft(np.conj(x), axis=axis))
    assert y.dtype == np.complex64
    return y


def model(x, sign, axis=-1, **kw):
    """the transform of one axis as the kernels do it: the network from 64 points on, a register butterfly below"""
    n = x.shape[axis]
    if n < 64:
        return fft32(x, sign, axis)
    return np.moveaxis(network(np.ascontiguousarray(np.moveaxis(x, axis, -1)), sign, **kw), -1, axis)


def scaled(y, n, kind):
    return y * np.float32(1.0 / n) if kind == "Inverse" else y


def real_model(x, n, kind, **kw):
    """rfft / irfft through an n / 2-point complex transform and the split of kernels_real.hip's header, in fp32"""
    M = n // 2
    k = np.arange(M)
    W = tw(n, k) if n >= 4 else np.ones(1, dtype=np.complex64)
    if kind == "Forward":
        z = (x[:, 0::2] + 1j * x[:, 1::2]).astype(np.complex64)
        Z = model(z, -1.0, **kw) if M > 1 else z
        Zr = np.conj(Z[:, (M - k) % M])
        X = (Z + Zr) * np.float32(0.5) + W * ((Z - Zr) * np.complex64(-0.5j))
        last = (Z[:, :1].real - Z[:, :1].imag).astype(np.complex64)
        return np.concatenate([X, last], axis=1).astype(np.complex64)
    X = x.copy()
    X.imag[:, 0] = 0
    X.imag[:, M] = 0
    Xr = np.conj(X[:, M - k])
    Z = ((X[:, :M] + Xr) + 1j * np.conj(W) * (X[:, :M] - Xr)).astype(np.complex64)
    z = model(Z, 1.0, **kw) if M > 1 else Z
    out = np.empty((x.shape[0], n), dtype=np.float32)
    out[:, 0::2], out[:, 1::2] = z.real, z.imag
    return scaled(out, n, kind)


# ---- the clean models pass every sweep ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", ss.STRIDED_CASES)
def test_model_passes_the_strided_and_real_sweeps(n, kind):
    y = scaled(model(ss.strided_input(n), ss.sign_of(kind), axis=1), n, kind)
    assert ss.strided_failures(y, n, kind) == []
    assert ss.real_failures(real_model(ss.real_input(n, kind), n, kind), n, kind) == []


@pytest.mark.parametrize("rows,cols", [s for s in ss.FFT2D_SHAPES if s[0] * s[1] <= 1 << 10 or s[1] in (64, 512, 2048)])
def test_model_passes_the_2d_sweeps(rows, cols):
    """every shape of the fused and the rows = 64 sweeps; of the rows = 2 sweeps one width per stage structure (the strided sweep
    above has been through every network)"""
    for kind in ss.FFT2D_KINDS:
        y = model(model(ss.fft2d_input(rows, cols), ss.sign_of(kind), axis=2), ss.sign_of(kind), axis=1)
        assert ss.fft2d_failures(y, rows, cols, kind) == []


def test_sweep_inputs_are_complete():
    for n in (2, 8, 64):
        x = ss.strided_input(n)
        assert x.shape == (1, n, n + 5) and np.array_equal(x[0, :, :n], np.eye(n)) and not x[0, :, n:].any()
        assert np.array_equal(ss.real_input(n, "Forward"), np.eye(n))
        X = ss.real_input(n, "Onlyinverse")
        M = n // 2
        assert X.shape == (n, M + 1) and np.array_equal(X[:M + 1], np.eye(M + 1)) and np.array_equal(X[M + 1:, 1:M], 1j * np.eye(M - 1))
    for rows, cols in ((4, 8), (2, 128), (64, 16)):
        x = ss.fft2d_input(rows, cols)
        spots = {tuple(np.argwhere(img)[0]) for img in x}
        assert (x != 0).sum() == x.shape[0] == len(spots)
        if rows <= 32:
            assert {s[1] for s in spots} == set(range(cols)) and (rows > 32 or cols > 32 or len(spots) == rows * cols)
    assert cc.ONEHOT_LENGTHS == cc.LENGTHS == ss.LENGTHS
    assert ss.REAL_INVERSE_ABS == 2 * (np.pi / 2 ** 20 + 1e-6)


# ---- doctored results fail, and say where ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,stage,t,q", [(4096, 1, 37, 5), (64, 0, 3, 2)])
def test_a_twiddle_one_table_entry_off_fails_the_sweep(n, stage, t, q):
    """one (t, q) of the second stage at n = 4096; at n = 64 the second stage multiplies by no twiddle of its own (J R = n),
    so it is the twiddle its inputs carry, applied by the first.  One entry of the 4096-entry table is 2 pi / 4096, 512
    times the angle bound."""
    kind = "Forward"
    y = model(ss.strided_input(n), -1.0, axis=1, doctor=(stage, t, q, 1))
    bad = ss.strided_failures(y, n, kind)
    assert len(bad) == 8 and all(m.startswith("strided Forward n %d, impulse at row " % n) and "output row" in m and "angle error" in m for m in bad)
    # the outputs the doctored products reach, and no others: compare with the clean model
    clean = model(ss.strided_input(n), -1.0, axis=1)
    hit = np.argwhere(y[0] != clean[0])
    named = {tuple(int(v) for v in re.search(r"impulse at row (\d+) .* output row (\d+)", m).groups()) for m in bad}
    assert named <= {(int(c), int(k)) for k, c in hit}
    assert ss.real_failures(real_model(ss.real_input(2 * n, "Forward"), 2 * n, "Forward", doctor=(stage, t, q, 1)), 2 * n, "Forward") \
        if n < 4096 else True


def test_a_column_taken_from_its_neighbour_fails_the_sweep():
    n = 128
    y = model(ss.strided_input(n), 1.0, axis=1).copy()
    y[0, :, 15] = y[0, :, 14]                                                # the last column of the first tile
    bad = ss.strided_failures(y, n, "Onlyinverse")
    assert bad and all("strided Onlyinverse n 128, impulse at row 15 (column 15), output row" in m for m in bad)
    assert "output row 1:" in bad[0]                                         # row 0 is 1 in every column


def test_a_dropped_imaginary_part_fails_the_real_sweep():
    n = 256
    y = real_model(ss.real_input(n, "Forward"), n, "Forward").copy()
    y.imag[7, 33] = 0
    bad = ss.real_failures(y, n, "Forward")
    assert len(bad) == 1 and "real Forward n 256, impulse at 7, output bin 33:" in bad[0] and "modulus error" in bad[0]
    # the inverse side: bin 9 read without its imaginary part makes the row of the imaginary unit at bin 9 zero
    X = ss.real_input(n, "Inverse").copy()
    X.imag[n // 2 + 9, 9] = 0
    bad = ss.real_failures(real_model(X, n, "Inverse"), n, "Inverse")
    assert len(bad) == 8 and all("real Inverse n 256, unit 1j at bin 9, output sample" in m for m in bad)


def test_a_nonzero_word_in_a_zero_column_fails_the_sweep():
    n = 32
    y = model(ss.strided_input(n), -1.0, axis=1).copy()
    assert ss.strided_failures(y, n, "Forward") == []
    y[0, 17, n + 4] = np.float32(1e-30)
    bad = ss.strided_failures(y, n, "Forward")
    assert len(bad) == 1 and "strided Forward n 32, zero column 36, output row 17" in bad[0] and "not zero" in bad[0]


def test_a_wrong_2d_output_and_a_nan_are_named():
    rows, cols = 8, 4
    y = model(model(ss.fft2d_input(rows, cols), 1.0, axis=2), 1.0, axis=1).copy()
    y[13, 5, 2] *= np.complex64(np.exp(1j * 1e-5))
    y[30, 0, 0] = np.nan
    bad = ss.fft2d_failures(y, rows, cols, "Onlyinverse")
    assert len(bad) == 2 and "fft2d Onlyinverse 8 x 4, impulse at (3, 1), output (5, 2)" in bad[0] and "impulse at (7, 2), output (0, 0)" in bad[1]


# ---- the class check ------------------------------------------------------------------------------------------------------
def _budget_shape(oracle, n):
    howmany = eb.MIN_SAMPLES // n
    x = oracle.gen_input(n * howmany, 1, first_transform=7).reshape(1, n, howmany)
    return x, np.fft.fft(x.astype(np.complex128), axis=1), howmany


@pytest.mark.parametrize("n", [4, 64, 1024, 4096])
def test_classes_of_a_healthy_transform_pass(oracle, n):
    x, ref, howmany = _budget_shape(oracle, n)
    y = model(x, -1.0, axis=1)
    bad, spread = ss.class_failures(y, ref, ss.strided_classes(n, howmany), float(eb.cap(n)), "model n %d" % n)
    assert bad == [] and all(hi <= 0.8 for lo, hi in spread.values()), spread
    assert len(spread) == (1 if n <= 32 else 3)


def test_a_precision_loss_in_one_column_of_16_passes_the_whole_buffer_cap_and_fails_its_class(oracle):
    """n = 1024 in the strided layout, the fp32 radix-2 model of tests/test_error_budget.py: with correctly rounded twiddles it
    sits at 0.56 of the cap in every class.  Column 11 of every 16-column tile then takes the same model with its twiddle
    angle evaluated in fp32, 1.13 of the cap: diluted 16-fold that passes the whole-buffer cap (0.61) and the flat 1e-5 per
    line; class_errors names the class."""
    n = 1024
    x, ref, howmany = _budget_shape(oracle, n)
    lines = np.ascontiguousarray(np.moveaxis(x, 1, 2)).reshape(howmany, n)

    def columns(a):
        return np.moveaxis(a.reshape(1, -1, n), 2, 1)
    cap = float(eb.cap(n))
    y = columns(_model_fft(lines, n, False)).copy()
    bad, spread = ss.class_failures(y, ref, ss.strided_classes(n, howmany), cap, "radix-2 model n %d" % n)
    assert bad == [] and all(0.45 <= lo and hi <= 0.7 for lo, hi in spread.values()), spread
    cols = np.arange(11, howmany, 16)
    y[:, :, cols] = columns(_model_fft(lines[cols], n, True))
    whole = float(np.sqrt((np.abs(y - ref) ** 2).sum() / (np.abs(ref) ** 2).sum()))
    assert whole <= 0.7 * cap
    per_line = np.sqrt((np.abs(y - ref) ** 2).sum(axis=1) / (np.abs(ref) ** 2).sum(axis=1))
    assert per_line.max() < 1e-5 / 10
    bad, spread = ss.class_failures(y, ref, ss.strided_classes(n, howmany), cap, "doctored n %d" % n)
    assert len(bad) == 1 and "class 11 of 'column mod 16'" in bad[0] and "above the cap" in bad[0]
    assert spread["column mod 16"][1] > 1.0 and spread["row element mod 32"][1] <= 1.0


def test_class_errors_refuses_thin_classes():
    y = np.zeros((4, 64), dtype=np.complex64)
    with pytest.raises(AssertionError, match="fewer than 1024"):
        ss.class_errors(y, np.ones((4, 64), dtype=np.complex128), {"line": np.arange(4).reshape(4, 1)})


@pytest.mark.parametrize("n", ss.LENGTHS)
def test_every_class_map_holds_enough_samples_at_the_budget_shapes(n):
    """the shapes test_budget / test_error_cap of the four GPU modules run: class_errors must not refuse one of them"""
    def check(shape, classes, complex_out=True):
        y = np.zeros(shape, dtype=np.complex64 if complex_out else np.float32)
        ss.class_errors(y, np.ones(shape, dtype=np.complex128 if complex_out else np.float64), classes)
    howmany = eb.MIN_SAMPLES // n
    check((1, n, howmany), ss.strided_classes(n, howmany))
    batch = -(-eb.MIN_SAMPLES // n)
    check((batch, n // 2 + 1), ss.real_classes(n, "Forward", batch))
    check((batch, n), ss.real_classes(n, "Inverse", batch), complex_out=False)
    check((cc.cap_batch(n), n), ss.lines_classes(n, cc.cap_batch(n)))
    for rows, cols in [(r, n) for r in ss.SMALL + [64]] + [(n, 64)]:
        b = -(-eb.MIN_SAMPLES // (rows * cols))
        check((b, rows, cols), ss.fft2d_classes(rows, cols, b))


# ---- every dispatchable kernel meets a sweep ------------------------------------------------------------------------------
def _dispatch_table():
    """What the four launch functions can return, written out from their switch statements: library -> {(kernel, log2 n,
    dir)}.  strided_launch also has a 64-bit-pointer twin of every entry (test_matrix_past_2gib_... runs those); conv_launch's
    third key is conj_filter."""
    t = {}
    t["strided"] = {("k_strided_small" if lg <= 5 else "k_strided", lg, d) for lg in range(1, 13) for d in ("FWD", "INV")}
    t["fft2d"] = {("k_chunk2d<%d>" % lgh, lgw, d) for lgw in range(1, 6) for lgh in range(0, 6) for d in ("FWD", "INV")} \
        | {("k_rows2d", lgw, d) for lgw in range(6, 13) for d in ("FWD", "INV")}
    t["real"] = {("k_real_small" if lg <= 6 else "k_real", lg, d) for lg in range(1, 13) for d in ("FWD", "INV")}
    t["conv"] = {("k_conv_small" if lg <= 5 else "k_conv", lg, c) for lg in range(1, 13) for c in (False, True)}
    return t


def _dir(kind):
    return "FWD" if kind == "Forward" else "INV"


def test_every_dispatchable_kernel_is_named_by_a_sweep_case():
    table = _dispatch_table()
    assert [len(table[k]) for k in ("strided", "fft2d", "real", "conv")] == [24, 74, 24, 24]
    swept = {
        "strided": {("k_strided_small" if n <= 32 else "k_strided", ss.lg2(n), _dir(kind)) for n, kind in ss.STRIDED_CASES},
        "real": {("k_real_small" if n <= 64 else "k_real", ss.lg2(n), _dir(kind)) for n, kind in ss.REAL_CASES},
        "fft2d": {("k_rows2d", ss.lg2(c), _dir(kind)) if c >= 64 else
                  ("k_chunk2d<%d>" % (ss.lg2(r) if r <= 32 else 0), ss.lg2(c), _dir(kind)) for r, c, kind in ss.FFT2D_CASES},
        "conv": {("k_conv_small" if n <= 32 else "k_conv", ss.lg2(n), conj) for n in cc.ONEHOT_LENGTHS for conj in cc.ONEHOT_CONJ},
    }
    for lib in table:
        assert swept[lib] == table[lib], (lib, sorted(table[lib] - swept[lib], key=str), sorted(swept[lib] - table[lib], key=str))
    # the strided column pass of the 2-D plans is the strided library's kernel, swept there at every length and direction


def test_the_dispatch_table_matches_the_launch_functions():
    """the switch statements themselves: one case per log2 length, 1 .. 12, and the kernel each one names"""
    def cases(path, func):
        text = open(os.path.join(ROOT, "fft_wgpu_amd", path)).read()
        body = text[text.index("static KernelLaunch %s(" % func):]
        body = body[:body.index("\n}\n")]
        return re.findall(r"case (\d+): k = (\w+)<(\d+)>", body)
    assert cases("strided/kernels_strided.hip", "strided_launch") == [(str(1 << lg), "kernel_of_lg", str(lg)) for lg in range(1, 13)]
    assert cases("fft2d/kernels_fft2d.hip", "rows_launch") == [(str(lg), "chunk_kernel_lgh" if lg <= 5 else "rows_kernel", str(lg)) for lg in range(1, 13)]
    assert cases("real/kernels_real.hip", "real_launch") == [(str(lg), "small_kernel" if lg <= 6 else "rows_kernel", str(lg if lg <= 6 else lg - 1))
                                                              for lg in range(1, 13)]
    assert cases("conv/kernels_conv.hip", "conv_launch") == [(str(lg), "small_kernel" if lg <= 5 else "rows_kernel", str(lg)) for lg in range(1, 13)]
    text = open(os.path.join(ROOT, "fft_wgpu_amd", "fft2d", "kernels_fft2d.hip")).read()
    assert re.findall(r"case (\d): return chunk_kernel<LGW, (\d)>", text) == [(str(h), str(h)) for h in range(6)]
    # the networks and tile widths the class maps were written from
    geom = open(os.path.join(ROOT, "fft_wgpu_amd", "strided", "strided_geom.h")).read()
    nets = {int(lg): tuple(int(v) for v in vals.split(",")) for lg, vals in re.findall(r"lg_n == (\d+) \? Net\{([\d, ]+)\}", geom)}
    assert nets == ss.NETS
