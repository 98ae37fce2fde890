"""GPU: the strided-batch plans (include/fft_wgpu_amd_strided.h) -- the columns of row-major matrices, in place.

The float64 reference is numpy.fft.fft / ifft on complex128 along the row axis; the input is oracle.gen_input, reshaped to
(batch, n rows, howmany columns).  A reference is computed once per shape and shared by the three plan kinds.  Bounds:
  parity       per column, oracle.compare's max_rel and rel-L2 <= REL_TOL (tests/conftest.py)
  budget       whole-buffer rel-L2 <= oracle.error_budget.cap(n), the one cap of every kernel family
  per class    test_budget_per_class: the same cap on the rel-L2 of every class of tests/side_sweeps.py's maps (column mod
               16 / 8 / 256, row mod T and div T), on the exec test_budget made
  impulses     pi / 2^20 in angle and 1e-6 in modulus, the bound of the project's impulse sweeps; test_dft_matrix_sweep
               (tests/side_sweeps.py) reads the whole DFT matrix out of every kernel, every kind, every n, per output
Everything else is bit for bit.  With STRIDED_RECORD=<path> in the environment the budget tests also write the measured
figures there (tests/golden/strided_error.json is such a record; no test pins to it).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # before the library: one HIP runtime in the process, the one torch brings (as in bench.py)

import guarded_arena as ga
import side_sweeps as ss
from conftest import REL_TOL
from oracle import error_budget as eb
from oracle.device_run import open_gpu
import side_libs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1 << lg for lg in range(1, 13)]
KINDS = ("Forward", "Inverse", "Onlyinverse")
INVALID_ARG, UNSUPPORTED = 1, 6


@pytest.fixture(scope="session")
def strided():
    return side_libs.load("strided")


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


_cache = {}


def matrices(oracle, n, howmany, batch):
    """(input, {kind: float64 reference}) as (batch, n, howmany) arrays, computed once per shape and left unchanged."""
    key = (n, howmany, batch)
    if key not in _cache:
        x = oracle.gen_input(n * howmany, batch, first_transform=7).reshape(batch, n, howmany)
        x64 = x.astype(np.complex128)
        inv = np.fft.ifft(x64, axis=1)
        _cache[key] = (x, {"Forward": np.fft.fft(x64, axis=1), "Inverse": inv, "Onlyinverse": inv * n})
        for a in (x,) + tuple(_cache[key][1].values()):
            a.setflags(write=False)
    return _cache[key]


def run(strided, gpu, kind, x, n, howmany, buf=None, encoder=None):
    """upload -> one exec -> read back; on `buf` (a view the caller owns) or on a fresh buffer at an allocation base"""
    fw, dev, queue = gpu
    own = buf is None
    if own:
        buf = dev.create_buffer(x.nbytes)
    queue.write_buffer(buf, 0, x)
    enc = encoder or dev.create_command_encoder()
    plan = getattr(strided, kind)(dev, queue, buf, n, howmany)
    assert plan.get("launches_per_exec") == 1 and plan.get("batch") == x.size // (n * howmany)
    assert plan.proc(enc) is buf
    y = buf.map_read(stream=enc).reshape(x.shape)
    plan.destroy()
    if encoder is None:
        enc.destroy()
    if own:
        buf.destroy()
    return y


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_parity(strided, gpu, oracle, n, kind):
    """howmany 1, 5, 16, 21, 67: a lone column, a partial first tile, exactly one tile, one tile plus a partial one, several
    tiles plus a partial one; batch 2: a second matrix."""
    bad = []
    for howmany in (1, 5, 16, 21, 67):
        x, ref = matrices(oracle, n, howmany, 2)
        y = run(strided, gpu, kind, x, n, howmany)
        worst = (0.0, 0.0)
        for b in range(2):
            for c in range(howmany):
                mx, l2 = oracle.compare(y[b, :, c], ref[kind][b, :, c])
                worst = max(worst, (mx, l2))
                if not (mx <= REL_TOL and l2 <= REL_TOL):
                    bad.append("howmany %d, matrix %d, column %d: max_rel %.3g rel_l2 %.3g" % (howmany, b, c, mx, l2))
        print("parity n=%d %s howmany=%d: worst max_rel %.3g rel_l2 %.3g" % (n, kind, howmany, worst[0], worst[1]))
    assert not bad, "\n".join(bad[:8])


# ---- budget ---------------------------------------------------------------------------------------------------------
_measured = {}
_budget_runs = {}


def budget_run(strided, gpu, oracle, n, kind):
    """One exec per (n, kind) at >= 2^18 samples (the smallest power-of-two howmany, one matrix), shared by the two budget
    tests: (whole-buffer rel-L2, failures of the per-class check)."""
    if (n, kind) not in _budget_runs:
        howmany = eb.MIN_SAMPLES // n
        x, ref = matrices(oracle, n, howmany, 1)
        y = run(strided, gpu, kind, x, n, howmany)
        r = ref[kind]
        rel_l2 = float(np.sqrt((np.abs(y - r) ** 2).sum() / (np.abs(r) ** 2).sum()))
        print("budget n=%d %s howmany=%d: rel_l2 %.4g = %.3f of the cap %.4g" % (n, kind, howmany, rel_l2, rel_l2 / eb.cap(n), eb.cap(n)))
        bad, spread = ss.class_failures(y, r, ss.strided_classes(n, howmany), float(eb.cap(n)), "strided %s n %d" % (kind, n))
        _measured["%d/%s" % (n, kind)] = dict({"n": n, "kind": kind, "howmany": howmany, "batch": 1, "rel_l2": rel_l2,
                                               "cap": float(eb.cap(n))}, **ss.spread_record(spread))
        path = os.environ.get("STRIDED_RECORD")
        if path:
            with open(path, "w") as f:
                json.dump({"metric": "whole-buffer rel-L2 against numpy.fft in float64; per class (tests/side_sweeps.py) as a "
                                     "fraction of the cap", "cases": _measured}, f, indent=1, sort_keys=True)
        _budget_runs[(n, kind)] = (rel_l2, bad)
    return _budget_runs[(n, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_budget(strided, gpu, oracle, n, kind):
    """>= 2^18 samples per shape (the smallest power-of-two howmany, one matrix): whole-buffer rel-L2 under the cap."""
    rel_l2, _ = budget_run(strided, gpu, oracle, n, kind)
    assert rel_l2 <= eb.cap(n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_budget_per_class(strided, gpu, oracle, n, kind):
    """the same exec: every class of columns (the lane group of a tile) and of rows (thread and register of the network)
    under the same cap"""
    _, bad = budget_run(strided, gpu, oracle, n, kind)
    assert not bad, "\n".join(bad)


# ---- the DFT matrix, per output -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", ss.STRIDED_CASES)
def test_dft_matrix_sweep(strided, gpu, n, kind):
    """one matrix of n rows x (n + 5) columns, column c a unit at row c: the output columns are the DFT matrix (/ n for
    Inverse), every entry within pi / 2^20 and 1e-6; the five zero columns, a partial last tile at every n, stay zero"""
    x = ss.strided_input(n)
    bad = ss.strided_failures(run(strided, gpu, kind, x, n, n + ss.ZERO_COLUMNS), n, kind)
    assert not bad, "\n".join(bad)


# ---- round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_round_trip(strided, gpu, oracle, n):
    fw, dev, queue = gpu
    howmany = 21
    x, _ = matrices(oracle, n, howmany, 2)
    y = run(strided, gpu, "Forward", x, n, howmany)
    z = run(strided, gpu, "Inverse", y, n, howmany)
    assert np.abs(z - x).max() <= 1e-5 * np.abs(x).max()
    # 1 / n is an exact power of two and |x| < 1: the scaled inverse times n is the unscaled one, bit for bit
    assert same_bits(run(strided, gpu, "Inverse", x, n, howmany) * np.float32(n), run(strided, gpu, "Onlyinverse", x, n, howmany))


# ---- 2-D composition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(256, 256), (64, 1024), (1024, 64)])
def test_two_plans_make_a_2d_transform_without_a_transpose(strided, gpu, oracle, rows, cols):
    fw, dev, queue = gpu
    x = oracle.gen_input(rows * cols, 1, first_transform=11)
    buf = dev.create_buffer(x.nbytes)
    queue.write_buffer(buf, 0, x)
    enc = dev.create_command_encoder()
    row_plan = fw.Forward(dev, queue, buf, cols)                     # fft_len = cols, batch = rows
    out = row_plan.proc(enc)
    col_plan = strided.Forward(dev, queue, out, rows, cols)          # the columns of the buffer proc returned
    y = col_plan.proc(enc).map_read(stream=enc).reshape(rows, cols)
    r = np.fft.fft2(x.reshape(rows, cols).astype(np.complex128))
    err = np.abs(y - r).max()
    print("2-D %d x %d: max |y - r| / max |r| = %.3g" % (rows, cols, err / np.abs(r).max()))
    assert err <= REL_TOL * np.abs(r).max()
    col_plan.destroy()
    row_plan.destroy()
    buf.destroy()


# ---- containment ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_arena(gpu):
    fw, dev, queue = gpu
    G = ga.guard_bytes(4096 * 64)
    arena = ga.GuardedArena(dev, queue, ga.straddle_arena_bytes([2 * 4096 * 64 * 8], G), G)
    yield arena
    arena.destroy()


@pytest.mark.parametrize("howmany", [17, 64])
@pytest.mark.parametrize("n", [16, 256, 1024, 4096])
def test_plan_stays_inside_its_view(strided, gpu, oracle, big_arena, n, howmany):
    """Views inside a poisoned arena at the four START_EXTRAS offsets, and one whose middle lies on a 4-GiB address
    boundary: no guard word changes, and the result has the bits of the same plan on a buffer at an allocation base."""
    fw, dev, queue = gpu
    x, ref = matrices(oracle, n, howmany, 2)
    base = run(strided, gpu, "Forward", x, n, howmany)
    assert np.abs(base - ref["Forward"]).max() <= REL_TOL * np.abs(ref["Forward"]).max()   # identical, and not identically wrong
    G = ga.guard_bytes(n * howmany)
    bad = []
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes([x.nbytes], G + max(ga.START_EXTRAS), G), G)
    placements = [("G + %d" % e, arena, G + e, True) for e in ga.START_EXTRAS]
    delta = (n + n // 2) * howmany * 8 + 16              # in the second matrix: row n / 2, column 2
    assert delta % 16 == 0 and x.nbytes // 2 < delta < x.nbytes
    big_arena.guard = G
    placements.append(("4-GiB boundary %d bytes into the view" % delta, big_arena,
                       ga.straddle_start(big_arena.device_ptr, delta, G), False))
    for where, a, start, whole in placements:
        (view,) = a.layout([x.nbytes], start, names=["buf"], whole=whole)
        assert view.device_ptr % 16 == 0 and view.device_ptr != a.device_ptr
        if not whole:
            assert view.device_ptr // ga.FOUR_GIB + 1 == (view.device_ptr + x.nbytes - 1) // ga.FOUR_GIB
        y = run(strided, gpu, "Forward", x, n, howmany, buf=view)
        bad += ["%s: %s" % (where, m) for m in a.check()]
        if not same_bits(y, base):
            bad.append("%s: the result differs from the base-buffer result in %d words" %
                       (where, int((y.view(np.uint32) != base.view(np.uint32)).sum())))
        view.destroy()
        a.views = []
    arena.destroy()
    assert not bad, "\n".join(bad)


# ---- special values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("Forward", "Inverse"))
@pytest.mark.parametrize("n", [8, 512, 2048])
def test_nan_stays_in_its_column_and_powers_of_two_scale_exactly(strided, gpu, oracle, n, kind):
    howmany = 21
    x, _ = matrices(oracle, n, howmany, 1)
    clean = run(strided, gpu, kind, x, n, howmany)
    assert not np.isnan(clean.view(np.float32)).any()
    for c in (0, howmany - 1, 15):                       # the first, the last, the last of a full tile beside a partial one
        p = x.copy()
        p[0, n // 3, c] = complex(np.nan, np.nan)
        y = run(strided, gpu, kind, p, n, howmany)
        assert np.isnan(y[0, :, c].real).all() and np.isnan(y[0, :, c].imag).all(), "column %d" % c
        others = [k for k in range(howmany) if k != c]
        assert same_bits(np.ascontiguousarray(y[:, :, others]), np.ascontiguousarray(clean[:, :, others])), "column %d" % c
    for s in (-40, 40, 90):
        f = np.float32(2.0) ** np.float32(s)
        y = run(strided, gpu, kind, x * f, n, howmany)
        assert np.isfinite(y.view(np.float32)).all()
        assert same_bits(y, clean * f), "2^%d" % s


# ---- past 4 GiB -----------------------------------------------------------------------------------------------------
def _impulse_failures(strided, gpu, n, howmany, impulses, rows, windows, kind="Forward"):
    """One zeroed matrix with a unit impulse at (j0, c) for every c: j0 of `impulses`; one exec of `kind`; in every window
    (first column, count) of every row of `rows`: the impulse columns hold exp(-+2 pi i j0 k / n) (/ n for Inverse: the
    exact power of two is taken off first) within pi / 2^20 in angle and 1e-6 in modulus, every other column is exactly
    zero."""
    sign, scale = (-1.0 if kind == "Forward" else 1.0), (float(n) if kind == "Inverse" else 1.0)
    fw, dev, queue = gpu
    row_bytes = howmany * 8
    t = torch.zeros(n * howmany, dtype=torch.complex64, device="cuda")       # zeroed on the device
    torch.cuda.synchronize()
    buf = dev.wrap_buffer(t.data_ptr(), n * row_bytes)
    one = np.array([1 + 0j], dtype=np.complex64)
    for c, j0 in impulses.items():
        queue.write_buffer(buf, j0 * row_bytes + c * 8, one)
    enc = dev.create_command_encoder()
    plan = getattr(strided, kind)(dev, queue, buf, n, howmany)
    per_wg = plan.get("tile_cols") * (512 // n if n <= 32 else 1)
    assert plan.get("batch") == 1 and plan.get("blocks") == -(-howmany // per_wg)
    plan.proc(enc)
    bad = []
    for k in rows:
        for c0, count in windows:
            y = buf.map_read(offset=k * row_bytes + c0 * 8, size=count * 8, stream=enc)
            cols = np.array(sorted(c for c in impulses if c0 <= c < c0 + count))
            assert cols.size
            got = y[cols - c0].astype(np.complex128) * scale
            j0 = np.array([impulses[c] for c in cols])
            want = np.exp(sign * 2j * np.pi * ((j0 * k) % n) / n)
            angle = np.abs(np.angle(got * np.conj(want)))
            modulus = np.abs(np.abs(got) - 1.0)
            if not (angle.max() <= np.pi / 2 ** 20 and modulus.max() <= 1e-6):
                bad.append("row %d: angle error %.3g, modulus error %.3g" % (k, angle.max(), modulus.max()))
            rest = y.copy()
            rest[cols - c0] = 0
            if np.count_nonzero(rest):
                bad.append("row %d: %d columns without an impulse are not zero, first %d" %
                           (k, np.count_nonzero(rest), c0 + int(np.flatnonzero(rest)[0])))
    plan.destroy()
    buf.destroy()
    del t
    torch.cuda.empty_cache()
    return bad


def test_matrix_past_4gib(strided, gpu):
    """n = 4096, howmany = 2^17 + 16, one matrix of 4.0005 GiB: byte offset 2^32 lies in the middle of the last row.  Unit
    impulses in eight columns of the first, middle and the last tile, two of them behind that offset; eight whole rows
    come back, the first and the last among them."""
    n, howmany = 4096, (1 << 17) + 16
    row_bytes = howmany * 8
    assert n * row_bytes > 1 << 32
    row_4g = (1 << 32) // row_bytes                                          # the row that contains byte offset 2^32:
    col_4g = ((1 << 32) - row_4g * row_bytes) // 8                           # the last one, from this column on
    assert row_4g == n - 1 and 0 < col_4g < howmany - 16
    impulses = {0: 0, 7: row_4g, 8: 1,                                       # the first tile (8 columns at n = 4096)
                col_4g - 13: row_4g, col_4g + 8: row_4g, 70001: 2047,        # middle tiles: just before and behind 2^32
                howmany - 8: row_4g, howmany - 1: row_4g - 1}                # the last tile
    assert sum((j0 * howmany + c) * 8 >= 1 << 32 for c, j0 in impulses.items()) == 2
    bad = _impulse_failures(strided, gpu, n, howmany, impulses, (0, 1, 1023, 2048 + 5, 3000, row_4g - 2, row_4g - 1, row_4g),
                            [(0, howmany)])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [2, 16, 64, 1024, 2048])
def test_matrix_past_2gib_takes_the_64bit_pointer_kernels(strided, gpu, n, kind):
    """A matrix of more than 2^31 bytes leaves the one-descriptor form of every kernel shape, in every kind (one column per
    thread, with 16 steps per workgroup at n = 2 and 2 at n = 16; two stages; three stages of 16 columns at 2048; three
    stages of 8 columns: the 4-GiB case above).  Same check, in three windows of 4096 columns of four rows."""
    howmany = (1 << 31) // (8 * n) + 5
    assert 8 * n * howmany > 1 << 31
    mid = howmany // 2
    impulses = {0: 0, 15: n - 1, 16: 1, mid + 1: n // 2, mid + 40: n - 1, howmany - 3: n - 1, howmany - 1: 1}
    windows = [(0, 4096), (mid - 2048, 4096), (howmany - 4096, 4096)]
    bad = _impulse_failures(strided, gpu, n, howmany, impulses, (0, 1, n // 2, n - 1), windows, kind)
    assert not bad, "\n".join(bad)


# ---- ordering -------------------------------------------------------------------------------------------------------
def test_execs_are_stream_ordered_and_allocate_nothing(strided, gpu, oracle):
    fw, dev, queue = gpu
    n, howmany = 1024, 67
    x, _ = matrices(oracle, n, howmany, 2)
    buf = dev.create_buffer(x.nbytes)
    enc = dev.create_command_encoder()
    plans = [strided.Forward(dev, queue, buf, n, howmany), strided.Inverse(dev, queue, buf, n, howmany),
             strided.Forward(dev, queue, buf, n, howmany)]
    queue.write_buffer(buf, 0, x)
    for p in plans:                                       # three synchronised execs
        p.proc(enc)
        enc.synchronize()
    want = buf.map_read(stream=enc)
    queue.write_buffer(buf, 0, x)
    for p in plans:                                       # the same three with nothing in between
        p.proc(enc)
    assert same_bits(buf.map_read(stream=enc), want)
    # a stream torch made, wrapped
    ts = torch.cuda.Stream()
    wrapped = dev.create_command_encoder(hip_stream=ts.cuda_stream)
    queue.write_buffer(buf, 0, x)
    for p in plans:
        p.proc(wrapped)
    assert same_bits(buf.map_read(stream=wrapped), want)
    wrapped.destroy()
    # exec allocates nothing
    dev.poll()
    before = dev.stats()["mem_free_bytes"]
    for _ in range(50):
        plans[0].proc(enc)
        plans[1].proc(enc)
    dev.poll()
    assert dev.stats()["mem_free_bytes"] == before
    for p in plans:
        p.destroy()
    buf.destroy()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_status_codes(strided, gpu):
    fw, dev, queue = gpu
    L = strided.lib()
    n, howmany = 64, 17
    buf = dev.create_buffer(2 * n * howmany * 8)
    out = ctypes.c_void_p()

    def create(ctx, kind, fft_len, hm, b):
        st = L.fws_plan_create(ctx, kind, fft_len, hm, b, ctypes.byref(out))
        if st == 0:
            L.fws_plan_destroy(out)
        else:
            assert not out.value
        return st
    assert create(dev._h, 0, n, howmany, buf._h) == 0
    assert create(None, 0, n, howmany, buf._h) == INVALID_ARG
    assert create(dev._h, 0, n, howmany, None) == INVALID_ARG
    assert L.fws_plan_create(dev._h, 0, n, howmany, buf._h, None) == INVALID_ARG
    assert L.fws_plan_exec(None, None) == INVALID_ARG
    for bad_len in (0, 48, 3):
        assert create(dev._h, 0, bad_len, howmany, buf._h) == INVALID_ARG
    assert create(dev._h, 0, n, 0, buf._h) == INVALID_ARG
    assert create(dev._h, 0, n, howmany + 1, buf._h) == INVALID_ARG          # not a whole number of matrices
    for kind in (3, 4, -1):                                                  # FWA_NORMALIZE, unknown kinds
        assert create(dev._h, kind, n, howmany, buf._h) == INVALID_ARG
    for fft_len in (1, 8192):
        with pytest.raises(fw.FwaError) as e:
            strided.Forward(dev, queue, buf, fft_len, howmany)
        assert e.value.status == UNSUPPORTED and "4096" in e.value.detail
    # a buffer and a stream of another context; a buffer whose context was destroyed
    other = fw.Device(0)
    foreign = other.create_buffer(2 * n * howmany * 8)
    assert create(dev._h, 0, n, howmany, foreign._h) == INVALID_ARG
    plan = strided.Forward(dev, queue, buf, n, howmany)
    foreign_stream = other.create_command_encoder()
    assert L.fws_plan_exec(plan._h, foreign_stream._h) == INVALID_ARG
    stale_stream = other.create_command_encoder()
    other.destroy()
    assert create(dev._h, 0, n, howmany, foreign._h) == INVALID_ARG
    assert L.fws_plan_exec(plan._h, stale_stream._h) == INVALID_ARG
    v = ctypes.c_int64()
    assert L.fws_plan_get_i64(plan._h, b"no_such_key", ctypes.byref(v)) == INVALID_ARG
    g = strided.describe(n, howmany, 2)
    assert {k: plan.get(k) for k in g} == g and plan.get("fft_len") == n and plan.get("howmany") == howmany
    plan.destroy()
    for h in (foreign, foreign_stream, stale_stream):
        h.destroy()
    buf.destroy()
