"""GPU: the real-input plans (include/fft_wgpu_amd_real.h) -- rfft / irfft of batched rows, out of place, one launch.

The float64 reference is numpy.fft.rfft / irfft on float64 / complex128 along the last axis.  Real rows are the real parts
of oracle.gen_input; spectra (the inverse kinds' input) are oracle.gen_input itself, which is not Hermitian: an inverse plan
is held to numpy.fft.irfft of exactly that.  A reference is computed once per shape and left unchanged.  Bounds:
  parity       per row, oracle.compare's max_rel and rel-L2 <= REL_TOL (tests/conftest.py); the real rows of the inverse
               kinds as float arrays, same two metrics
  budget       whole-buffer rel-L2 <= oracle.error_budget.cap(n): an n-point real transform is log2 n butterfly levels,
               the split being the last; a radix-2 fp32 model of this algorithm sits at 0.40 - 0.60 of cap(n)
  impulses     pi / 2^20 in angle and 1e-6 in modulus per output of the forward plans; 2 (pi / 2^20 + 1e-6) absolute per
               sample of the inverse plans (two unit-modulus terms, each at that bound)
  per class    test_budget_per_class: the cap of the budget on the rel-L2 of every class of tests/side_sweeps.py's maps
               (line mod RT or mod 256 / 128, element mod T and div T of the half-length network), on the exec test_budget
               made
  sweeps       test_dft_matrix_sweep (tests/side_sweeps.py): a unit at every sample of a forward row, a real unit at every
               bin and an imaginary unit at every interior bin of an inverse one, at every n, every output at the bounds
               above
Everything else is bit for bit.  With REAL_RECORD=<path> in the environment the budget tests also write the measured
figures there (tests/golden/real_error.json is such a record; no test pins to it).
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
IMPULSE_ANGLE, IMPULSE_MODULUS = np.pi / 2 ** 20, 1e-6
IMPULSE_ABS = 2 * (IMPULSE_ANGLE + IMPULSE_MODULUS)
assert (ss.ANGLE, ss.MODULUS, ss.REAL_INVERSE_ABS) == (IMPULSE_ANGLE, IMPULSE_MODULUS, IMPULSE_ABS)


def default_batch(n):
    """n <= 64: one full workgroup of 256 rows and three more; n >= 128: one full tile of 16 rows and three more"""
    return 259 if n <= 64 else 19


@pytest.fixture(scope="session")
def real():
    return side_libs.load("real")


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


_cache = {}


def rows(oracle, n, batch):
    """({kind: input}, {kind: float64 reference}) as (batch, n) / (batch, n / 2 + 1) arrays, computed once per shape"""
    key = (n, batch)
    if key not in _cache:
        x = np.ascontiguousarray(oracle.gen_input(n, batch, first_transform=7).real.reshape(batch, n))
        X = oracle.gen_input(n // 2 + 1, batch, first_transform=11).reshape(batch, n // 2 + 1)
        inv = np.fft.irfft(X.astype(np.complex128), n, axis=-1)
        _cache[key] = ({"Forward": x, "Inverse": X, "Onlyinverse": X},
                       {"Forward": np.fft.rfft(x.astype(np.float64), axis=-1), "Inverse": inv, "Onlyinverse": inv * n})
        for a in (x, X) + tuple(_cache[key][1].values()):
            a.setflags(write=False)
    return _cache[key]


def out_spec(kind, n, batch):
    """(bytes, dtype, row length) of a plan's destination"""
    return (batch * (n // 2 + 1) * 8, np.complex64, n // 2 + 1) if kind == "Forward" else (batch * n * 4, np.float32, n)


def run(real, gpu, kind, x, n, src=None, dst=None, keep_src=False):
    """upload -> one exec -> read back; on views the caller owns or on fresh buffers at an allocation base.
    keep_src: also return what src holds after the exec."""
    fw, dev, queue = gpu
    batch = x.shape[0]
    nbytes, dtype, width = out_spec(kind, n, batch)
    own = src is None
    if own:
        src, dst = dev.create_buffer(x.nbytes), dev.create_buffer(nbytes)
    queue.write_buffer(src, 0, x)
    enc = dev.create_command_encoder()
    plan = getattr(real, kind)(dev, queue, src, dst, n)
    assert plan.get("launches_per_exec") == 1 and plan.get("batch") == batch and plan.get("fft_len") == n
    assert plan.proc(enc) is dst
    y = dst.map_read(stream=enc, dtype=dtype).reshape(batch, width)
    after = src.map_read(stream=enc, dtype=x.dtype).reshape(x.shape) if keep_src else None
    plan.destroy()
    enc.destroy()
    if own:
        src.destroy()
        dst.destroy()
    return (y, after) if keep_src else y


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare_rows(oracle, y, ref):
    """worst (max_rel, rel_l2) over the rows: oracle.compare for complex rows, the same two metrics for float rows"""
    worst = (0.0, 0.0)
    for b in range(y.shape[0]):
        if np.iscomplexobj(y):
            mx, l2 = oracle.compare(y[b], ref[b])
        else:
            d = y[b].astype(np.float64) - ref[b]
            mx = float(np.abs(d).max() / np.abs(ref[b]).max()) if not np.isnan(d).any() else float("nan")
            l2 = float(np.sqrt((d * d).sum() / (ref[b] * ref[b]).sum()))
        worst = (max(worst[0], mx) if mx == mx else mx, max(worst[1], l2) if l2 == l2 else l2)
    return worst


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_parity(real, gpu, oracle, n, kind):
    """every n, a full workgroup / tile and a partial one; and batch 1"""
    bad = []
    for batch in (default_batch(n), 1):
        x, ref = rows(oracle, n, batch)
        y = run(real, gpu, kind, x[kind], n)
        mx, l2 = compare_rows(oracle, y, ref[kind])
        print("parity n %d %s batch %d: worst max_rel %.3g rel_l2 %.3g" % (n, kind, batch, mx, l2))
        if not (mx <= REL_TOL and l2 <= REL_TOL):
            bad.append("n %d %s batch %d: max_rel %.3g rel_l2 %.3g" % (n, kind, batch, mx, l2))
    assert not bad, "\n".join(bad)


# ---- budget ---------------------------------------------------------------------------------------------------------
_measured = {}
_budget_runs = {}


def budget_run(real, gpu, oracle, n, kind):
    """One exec per (n, kind) at >= 2^18 real samples, shared by the two budget tests: (whole-buffer rel-L2, failures of the
    per-class check)."""
    if (n, kind) not in _budget_runs:
        batch = -(-eb.MIN_SAMPLES // n)
        x, ref = rows(oracle, n, batch)
        y = run(real, gpu, kind, x[kind], n).astype(np.complex128 if kind == "Forward" else np.float64)
        r = ref[kind]
        rel_l2 = float(np.sqrt((np.abs(y - r) ** 2).sum() / (np.abs(r) ** 2).sum()))
        print("budget n %d %s batch %d: rel_l2 %.4g = %.3f of the cap %.4g" % (n, kind, batch, rel_l2, rel_l2 / eb.cap(n), eb.cap(n)))
        bad, spread = ss.class_failures(y, r, ss.real_classes(n, kind, batch), float(eb.cap(n)), "real %s n %d" % (kind, n))
        _measured["%d/%s" % (n, kind)] = dict({"n": n, "kind": kind, "batch": batch, "rel_l2": rel_l2, "cap": float(eb.cap(n))},
                                              **ss.spread_record(spread))
        path = os.environ.get("REAL_RECORD")
        if path:
            with open(path, "w") as f:
                json.dump({"metric": "whole-buffer rel-L2 against numpy.fft.rfft / irfft in float64; per class (tests/side_sweeps.py) "
                                     "as a fraction of the cap", "cases": _measured}, f, indent=1, sort_keys=True)
        _budget_runs[(n, kind)] = (rel_l2, bad)
    return _budget_runs[(n, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_budget(real, gpu, oracle, n, kind):
    """>= 2^18 real samples per length: whole-buffer rel-L2 under the cap of n"""
    rel_l2, _ = budget_run(real, gpu, oracle, n, kind)
    assert rel_l2 <= eb.cap(n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_budget_per_class(real, gpu, oracle, n, kind):
    """the same exec: every class of rows (the lane group of a tile, the thread of the small kernel) and of elements (thread
    and register of the half-length network) under the same cap"""
    _, bad = budget_run(real, gpu, oracle, n, kind)
    assert not bad, "\n".join(bad)


# ---- the DFT matrix, per output -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", ss.REAL_CASES)
def test_dft_matrix_sweep(real, gpu, n, kind):
    """Forward: batch n, row b a unit at b, bins 0 .. n / 2 of every row.  The inverse kinds: batch n, a real unit at every bin,
    then an imaginary unit at every interior bin; every sample of every row (the scaled kind times n)."""
    x = ss.real_input(n, kind)
    bad = ss.real_failures(run(real, gpu, kind, x, n), n, kind)
    assert not bad, "\n".join(bad)


# ---- impulses -------------------------------------------------------------------------------------------------------
def impulse_spots(n, top, seed):
    """0, 1, top / 2 (n / 2 of a real row), top - 1 and 16 seeded others, inside [0, top)"""
    rng = np.random.default_rng(seed + n)
    first = [p for p in (0, 1, top // 2, top - 1) if 0 <= p < top]
    return list(dict.fromkeys(first)) + [int(rng.integers(top)) for _ in range(16)]


@pytest.mark.parametrize("n", [2, 64, 128, 1024, 4096])
def test_forward_impulses(real, gpu, n):
    """row b holds one unit impulse at p: bin k is exp(-2 pi i p k / n), k = 0 .. n / 2"""
    spots = impulse_spots(n, n, 0xF0)
    x = np.zeros((len(spots), n), dtype=np.float32)
    for b, p in enumerate(spots):
        x[b, p] = 1
    y = run(real, gpu, "Forward", x, n).astype(np.complex128)
    k = np.arange(n // 2 + 1)
    bad = []
    for b, p in enumerate(spots):
        want = np.exp(-2j * np.pi * ((p * k) % n) / n)
        angle = np.abs(np.angle(y[b] * np.conj(want))).max()
        modulus = np.abs(np.abs(y[b]) - 1.0).max()
        print("impulse n %d Forward at %d: angle error %.3g, modulus error %.3g" % (n, p, angle, modulus))
        if not (angle <= IMPULSE_ANGLE and modulus <= IMPULSE_MODULUS):
            bad.append("impulse at %d: angle error %.3g, modulus error %.3g" % (p, angle, modulus))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", [2, 64, 128, 1024, 4096])
def test_onlyinverse_impulses(real, gpu, n):
    """a unit at bin q gives 2 cos(2 pi q j / n) (1 at q = 0, (-1)^j at q = n / 2); a unit imaginary at an interior q gives
    -2 sin(2 pi q j / n)"""
    M = n // 2
    spots = [(q, 1) for q in impulse_spots(n, M + 1, 0x1F) + [M]]
    spots += [(q, 1j) for q in impulse_spots(n, M + 1, 0x2F) if 0 < q < M]
    X = np.zeros((len(spots), M + 1), dtype=np.complex64)
    for b, (q, v) in enumerate(spots):
        X[b, q] = v
    y = run(real, gpu, "Onlyinverse", X, n).astype(np.float64)
    j = np.arange(n)
    bad = []
    for b, (q, v) in enumerate(spots):
        phase = 2 * np.pi * ((q * j) % n) / n
        if v == 1:
            want = np.cos(phase) * (1 if q in (0, M) else 2)
        else:
            want = -2 * np.sin(phase)
        err = np.abs(y[b] - want).max()
        print("impulse n %d Onlyinverse %s at bin %d: error %.3g" % (n, v, q, err))
        if not err <= IMPULSE_ABS:
            bad.append("unit %s at bin %d: error %.3g" % (v, q, err))
    assert not bad, "\n".join(bad)


# ---- round trip and scaling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 64, 256, 2048])
def test_round_trip_and_exact_scaling(real, gpu, oracle, n):
    batch = default_batch(n)
    x, _ = rows(oracle, n, batch)
    X = run(real, gpu, "Forward", x["Forward"], n)
    z = run(real, gpu, "Inverse", X, n)
    assert np.abs(z - x["Forward"]).max() <= REL_TOL * np.abs(x["Forward"]).max()
    # 1 / n is an exact power of two and nothing underflows: the scaled inverse times n is the unscaled one
    assert same_bits(run(real, gpu, "Inverse", x["Inverse"], n) * np.float32(n), run(real, gpu, "Onlyinverse", x["Onlyinverse"], n))


# ---- Im X[0], Im X[n/2] ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("Inverse", "Onlyinverse"))
@pytest.mark.parametrize("n", [2, 32, 512])
def test_imaginary_parts_of_bin_0_and_bin_half_are_ignored(real, gpu, oracle, n, kind):
    batch = default_batch(n)
    x, _ = rows(oracle, n, batch)
    zeros, nans, infs = (x[kind].copy() for _ in range(3))
    for a, v in ((zeros, 0.0), (nans, np.nan), (infs, np.inf)):
        a.imag[:, 0] = v
        a.imag[:, n // 2] = v
    want = run(real, gpu, kind, zeros, n)
    assert np.isfinite(want).all()
    assert same_bits(run(real, gpu, kind, nans, n), want)
    assert same_bits(run(real, gpu, kind, infs, n), want)


# ---- batch isolation, special values --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("Forward", "Inverse"))
@pytest.mark.parametrize("n", [16, 128, 4096])
def test_nan_stays_in_its_row_and_powers_of_two_scale_exactly(real, gpu, oracle, n, kind):
    """One NaN sample (a real sample of a forward plan; a real or an imaginary part of an inverse plan's bin, not one of the
    two ignored parts) makes every output of its row NaN -- a complex output counts as NaN when either part is -- and the
    other rows keep the bits of the clean exec."""
    batch = default_batch(n)
    x, _ = rows(oracle, n, batch)
    clean = run(real, gpu, kind, x[kind], n)
    assert not np.isnan(clean).any()
    width = x[kind].shape[1]
    places = [(0, 0, "re"), (batch // 2, width // 3, "im"), (batch - 1, width - 1, "re"), (1, width // 2, "im"), (batch - 2, 1 % width, "re")]
    for b, c, part in places:
        p = x[kind].copy()
        if kind == "Forward":
            p[b, c] = np.nan
        elif part == "im" and 0 < c < n // 2:
            p.imag[b, c] = np.nan
        else:
            p.real[b, c] = np.nan
        y = run(real, gpu, kind, p, n)
        assert np.isnan(y[b]).all(), "row %d, NaN at %d (%s)" % (b, c, part)
        others = [k for k in range(batch) if k != b]
        assert same_bits(y[others], clean[others]), "row %d" % b
    for s in (-40, 40):
        f = np.float32(2.0) ** np.float32(s)
        y = run(real, gpu, kind, x[kind] * f, n)
        assert np.isfinite(y).all()
        assert same_bits(y, clean * f), "2^%d" % s


# ---- containment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("Forward", "Onlyinverse"))
@pytest.mark.parametrize("n,batch", [(2, 515), (64, 259), (128, 19), (4096, 3)])
def test_plan_stays_inside_its_views(real, gpu, oracle, n, batch, kind):
    """src and dst as views inside one poisoned arena at the four START_EXTRAS offsets: no guard word changes, src keeps its
    bits, and dst has the bits of the same plan on buffers at allocation bases.  515 and 259 rows: full workgroups of 256
    and three rows; 19 rows: a 16-row tile and three; 3 rows: one partial tile."""
    fw, dev, queue = gpu
    x, ref = rows(oracle, n, batch)
    base = run(real, gpu, kind, x[kind], n)
    mx, l2 = compare_rows(oracle, base, ref[kind])
    assert mx <= REL_TOL and l2 <= REL_TOL                                   # identical, and not identically wrong
    nbytes = out_spec(kind, n, batch)[0]
    sizes = [x[kind].nbytes, nbytes]
    G = ga.guard_bytes(n)
    bad = []
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, G + max(ga.START_EXTRAS), G), G)
    for e in ga.START_EXTRAS:
        src, dst = arena.layout(sizes, G + e, names=["src", "dst"])
        assert src.device_ptr % 16 == 0 and dst.device_ptr % 16 == 0 and src.device_ptr != arena.device_ptr
        y, after = run(real, gpu, kind, x[kind], n, src=src, dst=dst, keep_src=True)
        bad += ["G + %d: %s" % (e, m) for m in arena.check()]
        if not same_bits(after, x[kind]):
            bad.append("G + %d: src changed" % e)
        if not same_bits(y, base):
            bad.append("G + %d: the result differs from the base-buffer result in %d words" %
                       (e, int((y.view(np.uint32) != base.view(np.uint32)).sum())))
        for v in (src, dst):
            v.destroy()
        arena.views = []
    arena.destroy()
    assert not bad, "\n".join(bad)


# ---- past 4 GiB -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("Forward", "Onlyinverse"))
def test_buffers_past_4gib(real, gpu, kind):
    """n = 4096, batch = 2^18 + 16: 4 GiB + 256 KiB of real rows and 4 GiB + 2.25 MiB of spectra, zeroed on the device.
    Unit impulses in row 0, in the rows that straddle byte offset 2^32 of the real and of the spectrum buffer, and in the
    last row: those rows are held to the impulse bounds, sampled other rows stay exactly zero."""
    fw, dev, queue = gpu
    n, M = 4096, 2048
    batch = (1 << 18) + 16
    real_row, spec_row = n * 4, (M + 1) * 8
    assert batch * real_row > 1 << 32 and batch * spec_row > 1 << 32
    t_real = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    t_spec = torch.zeros(batch * (M + 1), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    b_real, b_spec = dev.wrap_buffer(t_real.data_ptr(), batch * real_row), dev.wrap_buffer(t_spec.data_ptr(), batch * spec_row)
    straddle_real, straddle_spec = ((1 << 32) - 1) // real_row, ((1 << 32) - 1) // spec_row
    assert straddle_spec * spec_row < 1 << 32 < (straddle_spec + 1) * spec_row and straddle_real == (1 << 18) - 1
    hot = {0: 1, straddle_spec: M - 1, straddle_real: 5, straddle_real + 1: 2047, batch - 1: M}    # row -> impulse position
    assert len(hot) == 5
    src, dst = (b_real, b_spec) if kind == "Forward" else (b_spec, b_real)
    for b, p in hot.items():
        if kind == "Forward":
            queue.write_buffer(src, b * real_row + p * 4, np.array([1], dtype=np.float32))
        else:
            queue.write_buffer(src, b * spec_row + p * 8, np.array([1], dtype=np.complex64))
    enc = dev.create_command_encoder()
    plan = getattr(real, kind)(dev, queue, src, dst, n)
    assert plan.get("batch") == batch and plan.get("blocks") == batch // 16 and plan.get("launches_per_exec") == 1
    plan.proc(enc)
    bad = []
    k, j = np.arange(M + 1), np.arange(n)
    sampled = sorted(set(hot) | {1, 15, 16, straddle_spec - 1, straddle_spec + 1, straddle_real - 1, straddle_real + 2,
                                 batch - 17, batch - 2})
    for b in sampled:
        if kind == "Forward":
            y = dst.map_read(offset=b * spec_row, size=spec_row, stream=enc).astype(np.complex128)
        else:
            y = dst.map_read(offset=b * real_row, size=real_row, stream=enc, dtype=np.float32).astype(np.float64)
        if b not in hot:
            if np.count_nonzero(y):
                bad.append("row %d: %d outputs are not zero" % (b, np.count_nonzero(y)))
            continue
        p = hot[b]
        if kind == "Forward":
            want = np.exp(-2j * np.pi * ((p * k) % n) / n)
            angle, modulus = np.abs(np.angle(y * np.conj(want))).max(), np.abs(np.abs(y) - 1.0).max()
            if not (angle <= IMPULSE_ANGLE and modulus <= IMPULSE_MODULUS):
                bad.append("row %d: angle error %.3g, modulus error %.3g" % (b, angle, modulus))
        else:
            want = np.cos(2 * np.pi * ((p * j) % n) / n) * (1 if p in (0, M) else 2)
            err = np.abs(y - want).max()
            if not err <= IMPULSE_ABS:
                bad.append("row %d: error %.3g" % (b, err))
    plan.destroy()
    enc.destroy()
    b_real.destroy()
    b_spec.destroy()
    del t_real, t_spec
    torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ---- ordering -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 256, 4096])
def test_execs_are_stream_ordered_and_allocate_nothing(real, gpu, oracle, n):
    fw, dev, queue = gpu
    batch = default_batch(n)
    x = rows(oracle, n, batch)[0]["Forward"]
    spec_bytes = batch * (n // 2 + 1) * 8
    a, spec, b, copy = dev.create_buffer(x.nbytes), dev.create_buffer(spec_bytes), dev.create_buffer(x.nbytes), dev.create_buffer(x.nbytes)
    enc = dev.create_command_encoder()
    fwd, inv = real.Forward(dev, queue, a, spec, n), real.Onlyinverse(dev, queue, spec, b, n)
    assert fwd.get("launches_per_exec") == inv.get("launches_per_exec") == 1
    queue.write_buffer(a, 0, x)
    for p in (fwd, inv):                                  # two synchronised execs
        p.proc(enc)
        enc.synchronize()
    want = b.map_read(stream=enc, dtype=np.float32)
    assert np.abs(want.reshape(x.shape) - x * np.float32(n)).max() <= REL_TOL * n
    queue.write_buffer(spec, 0, np.zeros(spec_bytes // 8, dtype=np.complex64))
    queue.write_buffer(b, 0, np.zeros_like(x))
    fwd.proc(enc)                                         # the same two and a copy that depends on them, nothing in between
    inv.proc(enc)
    enc.copy_buffer_to_buffer(b, 0, copy, 0, x.nbytes)
    assert same_bits(copy.map_read(stream=enc, dtype=np.float32), want)
    dev.poll()
    before = dev.stats()["mem_free_bytes"]
    for _ in range(10):
        fwd.proc(enc)
        inv.proc(enc)
    dev.poll()
    assert dev.stats()["mem_free_bytes"] == before
    for h in (fwd, inv, enc, a, spec, b, copy):
        h.destroy()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_status_codes(real, gpu):
    fw, dev, queue = gpu
    L = real.lib()
    n, batch = 64, 6
    xb, sb = dev.create_buffer(batch * n * 4), dev.create_buffer(batch * (n // 2 + 1) * 8)
    out = ctypes.c_void_p()

    def create(ctx, kind, length, src, dst):
        st = L.fwr_plan_create(ctx, kind, length, src, dst, ctypes.byref(out))
        if st == 0:
            L.fwr_plan_destroy(out)
        else:
            assert not out.value
        return st
    assert create(dev._h, 0, n, xb._h, sb._h) == 0
    assert create(dev._h, 1, n, sb._h, xb._h) == 0 and create(dev._h, 2, n, sb._h, xb._h) == 0
    assert create(None, 0, n, xb._h, sb._h) == INVALID_ARG
    assert create(dev._h, 0, n, None, sb._h) == INVALID_ARG and create(dev._h, 0, n, xb._h, None) == INVALID_ARG
    assert L.fwr_plan_create(dev._h, 0, n, xb._h, sb._h, None) == INVALID_ARG
    assert L.fwr_plan_exec(None, None) == INVALID_ARG
    for bad_len in (0, 48, 3):
        assert create(dev._h, 0, bad_len, xb._h, sb._h) == INVALID_ARG
    for kind in (3, 4, -1):                                                  # FWA_NORMALIZE, unknown kinds
        assert create(dev._h, kind, n, xb._h, sb._h) == INVALID_ARG
    for length, word in ((1, "2 .. 4096"), (8192, "4096")):
        with pytest.raises(fw.FwaError) as e:
            real.Forward(dev, queue, xb, sb, length)
        assert e.value.status == UNSUPPORTED and word in e.value.detail
    # the buffers the wrong way round: sizes that are not whole rows of that side
    assert create(dev._h, 0, n, sb._h, xb._h) == INVALID_ARG and create(dev._h, 1, n, xb._h, sb._h) == INVALID_ARG
    # mismatched batch: 6 real rows, 4 spectrum rows
    short = dev.wrap_buffer(sb.device_ptr, 4 * (n // 2 + 1) * 8)
    with pytest.raises(fw.FwaError) as e:
        real.Forward(dev, queue, xb, short, n)
    assert e.value.status == INVALID_ARG and "batch" in e.value.detail
    assert create(dev._h, 2, n, short._h, xb._h) == INVALID_ARG
    # overlapping views: the same buffer, and two views of one allocation whose byte ranges share 16 bytes
    same = dev.create_buffer(n * 4 * 33)                                      # 33 real rows = 32 spectrum rows of n = 64
    assert same.size == 32 * (n // 2 + 1) * 8
    with pytest.raises(fw.FwaError) as e:
        real.Forward(dev, queue, same, same, n)
    assert e.value.status == INVALID_ARG and "overlap" in e.value.detail
    arena = dev.create_buffer(2 * n * 4 + 2 * (n // 2 + 1) * 8)
    v_real = dev.wrap_buffer(arena.device_ptr, 2 * n * 4)
    v_over = dev.wrap_buffer(arena.device_ptr + 2 * n * 4 - 16, 2 * (n // 2 + 1) * 8)
    v_next = dev.wrap_buffer(arena.device_ptr + 2 * n * 4, 2 * (n // 2 + 1) * 8)
    assert create(dev._h, 0, n, v_real._h, v_over._h) == INVALID_ARG and create(dev._h, 2, n, v_over._h, v_real._h) == INVALID_ARG
    assert create(dev._h, 0, n, v_real._h, v_next._h) == 0 and create(dev._h, 1, n, v_next._h, v_real._h) == 0   # adjacent is fine
    # a buffer and a stream of another context; a buffer whose context was destroyed
    other = fw.Device(0)
    foreign = other.create_buffer(batch * n * 4)
    assert create(dev._h, 0, n, foreign._h, sb._h) == INVALID_ARG and create(dev._h, 1, n, sb._h, foreign._h) == INVALID_ARG
    plan = real.Forward(dev, queue, xb, sb, n)
    foreign_stream = other.create_command_encoder()
    assert L.fwr_plan_exec(plan._h, foreign_stream._h) == INVALID_ARG
    stale_stream = other.create_command_encoder()
    other.destroy()
    assert create(dev._h, 0, n, foreign._h, sb._h) == INVALID_ARG
    assert L.fwr_plan_exec(plan._h, stale_stream._h) == INVALID_ARG
    v = ctypes.c_int64()
    assert L.fwr_plan_get_i64(plan._h, b"no_such_key", ctypes.byref(v)) == INVALID_ARG
    g = real.describe(n, batch)
    assert {k: plan.get(k) for k in g} == g
    assert (plan.get("fft_len"), plan.get("batch"), plan.get("launches_per_exec")) == (n, batch, 1)
    plan.destroy()
    for h in (foreign, foreign_stream, stale_stream, short, same, v_real, v_over, v_next, arena, xb, sb):
        h.destroy()
