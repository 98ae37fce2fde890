"""GPU: the fused FFT-convolution plans (include/fft_wgpu_amd_conv.h) -- ifft(fft(x) * H[b mod F]) of batched rows, one launch.

The inputs, the float64 reference and every numeric bound live in tests/conv_cases.py, which tests/test_conv.py also applies
to a numpy complex64 model on the CPU: parity (per row, REL_TOL), the cap (whole-buffer rel-L2 <= cap(2 n n)), the one-hot
sweep (2 pi / 2^20 in angle, 2e-6 in modulus relative to 1 / n; at every n, through both conj_filter forms) and the shifts;
test_budget_per_class holds every class of tests/side_sweeps.py's maps (line mod RT or the owning thread of a chunk, element
mod T and div T) to the same cap, on the execs test_error_cap made.  Everything else here is bit for bit.  With
CONV_RECORD=<path> in the environment the cap tests also write the measured figures there (tests/golden/conv_error.json is
such a record; no test pins to it).

Shapes: n = 2 (one butterfly), 32 (the last chunk-shape length), 64 (the first network, 8 x 8), 512 and 1024 (32-point
stages), 2048 (three stages, two exchanges each way), 4096 (RT = 8); parity at every n.  Batch: one full workgroup and three
rows, and 1.  F = 3 divides no tile: the filter row wraps inside a workgroup.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # before the library: one HIP runtime in the process, the one torch brings (as in bench.py)

import conv_cases as cc
import guarded_arena as ga
import side_sweeps as ss
from oracle.device_run import open_gpu
import side_libs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 6
SPECIAL = [32, 64, 2048]


@pytest.fixture(scope="module")
def conv():
    return side_libs.load("conv")


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


def run(conv, gpu, kind, x, H, n, conj=False, in_place=False, views=None, keep=False):
    """upload -> one exec -> read back; on the views (src, filter, dst) the caller owns or on fresh buffers at allocation
    bases.  keep: also return what src and filter hold after the exec."""
    fw, dev, queue = gpu
    batch = x.shape[0]
    own = views is None
    if own:
        src, flt = dev.create_buffer(x.nbytes), dev.create_buffer(H.nbytes)
        dst = src if in_place else dev.create_buffer(x.nbytes)
    else:
        src, flt, dst = views
    queue.write_buffer(src, 0, x)
    queue.write_buffer(flt, 0, H)
    enc = dev.create_command_encoder()
    plan = getattr(conv, kind)(dev, queue, src, flt, dst, n, conj_filter=conj)
    assert plan.get("launches_per_exec") == 1 and plan.get("batch") == batch and plan.get("fft_len") == n
    assert plan.get("filters") == H.shape[0] and plan.get("in_place") == int(dst is src)
    assert plan.proc(enc) is dst
    y = dst.map_read(stream=enc).reshape(batch, n)
    after = (src.map_read(stream=enc).reshape(x.shape), flt.map_read(stream=enc).reshape(H.shape)) if keep else None
    plan.destroy()
    enc.destroy()
    if own:
        for b in {src, flt, dst}:
            b.destroy()
    return (y,) + after if keep else y


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def nan_rows(y):
    """rows whose every output is NaN (a complex output counts as NaN when either part is) / rows with any NaN"""
    bad = np.isnan(y)
    return set(np.flatnonzero(bad.all(axis=1))), set(np.flatnonzero(bad.any(axis=1)))


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("n", cc.LENGTHS)
def test_parity(conv, gpu, oracle, n, kind):
    """every n, conj_filter off and on, F = 3; a full workgroup and a partial one, and batch 1"""
    bad = []
    for batch in (cc.default_batch(n), 1):
        x, H = cc.inputs(oracle, n, batch, 3)
        for conj in (False, True):
            ref = cc.cached_reference(oracle, n, batch, 3, kind, conj)
            y = run(conv, gpu, kind, x, H, n, conj)
            bad += cc.parity_failures(oracle, y, ref, "n %d %s conj %d batch %d" % (n, kind, conj, batch))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", cc.SHAPES)
def test_one_filter_and_one_filter_per_row(conv, gpu, oracle, n):
    """F = 1 (every row the same spectrum) and F = batch (no wrap at all)"""
    batch = cc.default_batch(n)
    bad = []
    for F in (1, batch):
        x, H = cc.inputs(oracle, n, batch, F)
        ref = cc.cached_reference(oracle, n, batch, F, "Convolve", False)
        bad += cc.parity_failures(oracle, run(conv, gpu, "Convolve", x, H, n), ref, "n %d F %d" % (n, F))
    assert not bad, "\n".join(bad)


# ---- error cap ------------------------------------------------------------------------------------------------------
_measured = {}
_cap_runs = {}


def cap_run(conv, gpu, oracle, n):
    """The two execs (conj_filter off and on) of one length at >= 2^18 samples, shared by the two cap tests: (failures of
    the whole-buffer cap, failures of the per-class check)."""
    if n not in _cap_runs:
        batch = cc.cap_batch(n)
        x, H = cc.inputs(oracle, n, batch, 3)[0], cc.cap_filters(oracle, n)
        bad, class_bad = [], []
        for conj in (False, True):
            ref = cc.reference(x, H, "Convolve", conj)
            y = run(conv, gpu, "Convolve", x, H, n, conj)
            what = "n %d conj %d batch %d" % (n, conj, batch)
            bad += cc.cap_failures(y, ref, n, what)
            mx, _ = cc.row_errors(oracle, y, ref)
            more, spread = ss.class_failures(y, ref, ss.lines_classes(n, batch), cc.cap(n), "conv " + what)
            class_bad += more
            _measured["%d/%s" % (n, "conj" if conj else "plain")] = dict(
                {"n": n, "conj_filter": conj, "batch": batch, "rel_l2": cc.whole_rel_l2(y, ref), "max_rel": mx, "cap": cc.cap(n)},
                **ss.spread_record(spread))
        path = os.environ.get("CONV_RECORD")
        if path:
            with open(path, "w") as f:
                json.dump({"metric": "whole-buffer rel-L2 (and worst per-row max_rel) against numpy.fft.ifft(numpy.fft.fft(x) * H) in float64, "
                                     "scaled kind, three filters; per class (tests/side_sweeps.py) as a fraction of the cap",
                           "cases": _measured}, f, indent=1, sort_keys=True)
        _cap_runs[n] = (bad, class_bad)
    return _cap_runs[n]


@pytest.mark.parametrize("n", cc.LENGTHS)
def test_error_cap(conv, gpu, oracle, n):
    """>= 2^18 samples per length, three filters (flat random, a decaying impulse response, a 60-dB low-pass): whole-buffer
    rel-L2 under cap(2 n n)"""
    bad, _ = cap_run(conv, gpu, oracle, n)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", cc.LENGTHS)
def test_budget_per_class(conv, gpu, oracle, n):
    """the same execs: every class of rows (the lane group of a tile, the thread of a chunk) and of elements (thread and
    register of the network) under the same cap"""
    _, bad = cap_run(conv, gpu, oracle, n)
    assert not bad, "\n".join(bad)


# ---- every bin meets its own filter sample ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.ONEHOT_LENGTHS)
def test_every_bin_meets_its_own_filter_sample(conv, gpu, n):
    """batch = F = n, filter row b one-hot at bin b, src row b a unit impulse: row b answers with the tone of bin b, through
    the plain and the conjugating form of the kernel (1 + 0i is its own conjugate: the same answer)"""
    x, H = cc.onehot_inputs(n)
    bad = []
    for conj in cc.ONEHOT_CONJ:
        bad += ["conj %d, %s" % (conj, m) for m in cc.onehot_failures(run(conv, gpu, "Convolve", x, H, n, conj), n)]
    assert not bad, "\n".join(bad)


# ---- shifts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.SHAPES)
def test_shifts(conv, gpu, oracle, n):
    """the spectrum of a unit impulse at q rotates every row by q"""
    batch = cc.default_batch(n)
    x, _ = cc.inputs(oracle, n, batch, 3)
    bad = []
    for q in cc.shifts(n):
        y = run(conv, gpu, "Convolve", x, cc.shift_filter(n, q), n)
        bad += cc.parity_failures(oracle, y, np.roll(x, q, axis=1).astype(np.complex128), "n %d shift %d" % (n, q))
    assert not bad, "\n".join(bad)


# ---- in place -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.SHAPES)
def test_in_place_gives_the_same_bits_and_inputs_are_not_written(conv, gpu, oracle, n):
    batch = cc.default_batch(n)
    x, H = cc.inputs(oracle, n, batch, 3)
    for kind, conj in (("Convolve", False), ("OnlyConvolve", True)):
        y, src_after, flt_after = run(conv, gpu, kind, x, H, n, conj, keep=True)
        assert not cc.parity_failures(oracle, y, cc.cached_reference(oracle, n, batch, 3, kind, conj), "n %d %s" % (n, kind))
        assert same_bits(src_after, x) and same_bits(flt_after, H)
        z, _, flt_after = run(conv, gpu, kind, x, H, n, conj, in_place=True, keep=True)
        assert same_bits(z, y) and same_bits(flt_after, H)
    # 1 / n is an exact power of two and nothing underflows: the scaled kind times n is the unscaled one
    assert same_bits(run(conv, gpu, "Convolve", x, H, n) * np.float32(n), run(conv, gpu, "OnlyConvolve", x, H, n))


# ---- special values, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SPECIAL)
def test_a_nan_stays_in_its_row_and_in_the_rows_of_its_filter(conv, gpu, oracle, n):
    batch, F = cc.default_batch(n), 3
    x, H = cc.inputs(oracle, n, batch, F)
    clean = run(conv, gpu, "Convolve", x, H, n)
    assert not np.isnan(clean).any()
    for b, c, part in ((0, 0, "re"), (batch // 2, n // 3, "im"), (batch - 1, n - 1, "re"), (batch - 4, 1, "im")):
        p = x.copy()
        if part == "re":
            p.real[b, c] = np.nan
        else:
            p.imag[b, c] = np.nan
        y = run(conv, gpu, "Convolve", p, H, n)
        whole, some = nan_rows(y)
        assert whole == some == {b}, "NaN in row %d at %d (%s): all-NaN rows %s, rows with a NaN %s" % (b, c, part, sorted(whole), sorted(some))
        others = [k for k in range(batch) if k != b]
        assert same_bits(y[others], clean[others]), "row %d" % b
    for f, c, part in ((0, 0, "re"), (1, n // 2, "im"), (2, n - 1, "re")):
        G = H.copy()
        if part == "re":
            G.real[f, c] = np.nan
        else:
            G.imag[f, c] = np.nan
        y = run(conv, gpu, "Convolve", x, G, n)
        want = {b for b in range(batch) if b % F == f}
        whole, some = nan_rows(y)
        assert whole == some == want, "NaN in filter row %d at %d (%s)" % (f, c, part)
        others = [k for k in range(batch) if k % F != f]
        assert same_bits(y[others], clean[others]), "filter row %d" % f


@pytest.mark.parametrize("n", SPECIAL)
def test_powers_of_two_scale_exactly(conv, gpu, oracle, n):
    batch = cc.default_batch(n)
    x, H = cc.inputs(oracle, n, batch, 3)
    clean = run(conv, gpu, "Convolve", x, H, n)
    for s in (-40, 40):
        f = np.float32(2.0) ** np.float32(s)
        for y in (run(conv, gpu, "Convolve", x * f, H, n), run(conv, gpu, "Convolve", x, H * f, n)):
            assert np.isfinite(y).all()
            assert same_bits(y, clean * f), "2^%d" % s


# ---- containment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(2, 4096 + 3), (32, 256 + 3), (64, 19), (1024, 19), (4096, 3)])
def test_plan_stays_inside_its_views(conv, gpu, oracle, n, batch):
    """src, filter and dst as views inside one poisoned arena at the four START_EXTRAS offsets: no guard word changes, src
    and filter keep their bits, and dst has the bits of the same plan on buffers at allocation bases -- out of place and in
    place (dst = the src view)."""
    fw, dev, queue = gpu
    F = 3
    x, H = cc.inputs(oracle, n, batch, F)
    base = run(conv, gpu, "Convolve", x, H, n)
    assert not cc.parity_failures(oracle, base, cc.cached_reference(oracle, n, batch, F, "Convolve", False), "n %d" % n)
    sizes = [x.nbytes, H.nbytes, x.nbytes]
    G = ga.guard_bytes(n)
    bad = []
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, G + max(ga.START_EXTRAS), G), G)
    for e in ga.START_EXTRAS:
        src, flt, dst = arena.layout(sizes, G + e, names=["src", "filter", "dst"])
        assert all(v.device_ptr % 16 == 0 for v in (src, flt, dst)) and src.device_ptr != arena.device_ptr
        y, src_after, flt_after = run(conv, gpu, "Convolve", x, H, n, views=(src, flt, dst), keep=True)
        bad += ["G + %d: %s" % (e, m) for m in arena.check()]
        if not (same_bits(src_after, x) and same_bits(flt_after, H)):
            bad.append("G + %d: src or filter changed" % e)
        if not same_bits(y, base):
            bad.append("G + %d: the result differs from the base-buffer result in %d words" % (e, int((y.view(np.uint32) != base.view(np.uint32)).sum())))
        z, _, flt_after = run(conv, gpu, "Convolve", x, H, n, views=(src, flt, src), keep=True)
        bad += ["G + %d, in place: %s" % (e, m) for m in arena.check()]
        if not (same_bits(z, base) and same_bits(flt_after, H)):
            bad.append("G + %d, in place: the result differs from the base-buffer result, or the filter changed" % e)
        for v in (src, flt, dst):
            v.destroy()
        arena.views = []
    arena.destroy()
    assert not bad, "\n".join(bad)


# ---- past 4 GiB -----------------------------------------------------------------------------------------------------
def _hot_rows_case(conv, gpu, oracle, n, batch, filters, hot, hot_filters, cold):
    """A zeroed `batch` x n buffer, convolved in place with a zeroed bank of `filters` rows: rows `hot` hold generator data and
    the filter rows `hot_filters` generator spectra; the hot rows are held to the reference, the rows `cold` stay exactly 0."""
    fw, dev, queue = gpu
    row = n * 8
    t_x = torch.zeros(batch * n, dtype=torch.complex64, device="cuda")
    t_h = torch.zeros(filters * n, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    buf, bank = dev.wrap_buffer(t_x.data_ptr(), batch * row), dev.wrap_buffer(t_h.data_ptr(), filters * row)
    x = oracle.gen_input(n, len(hot), first_transform=9).reshape(len(hot), n)
    H = oracle.gen_input(n, len(hot_filters), first_transform=1 << 22).reshape(len(hot_filters), n)
    for i, b in enumerate(hot):
        queue.write_buffer(buf, b * row, x[i])
    for i, f in enumerate(hot_filters):
        queue.write_buffer(bank, f * row, H[i])
    Hfull = {f: H[i].astype(np.complex128) for i, f in enumerate(hot_filters)}
    enc = dev.create_command_encoder()
    plan = conv.Convolve(dev, queue, buf, bank, buf, n)
    g = conv.describe(n, batch)
    assert plan.get("batch") == batch and plan.get("filters") == filters and plan.get("in_place") == 1
    assert plan.get("blocks") == g["blocks"] == -(-batch // cc.rows_per_block(n)) and plan.get("launches_per_exec") == 1
    plan.proc(enc)
    bad = []
    for i, b in enumerate(hot):
        y = buf.map_read(offset=b * row, size=row, stream=enc)
        h = Hfull.get(b % filters, np.zeros(n, dtype=np.complex128))
        ref = np.fft.ifft(np.fft.fft(x[i].astype(np.complex128)) * h)
        if np.abs(ref).max() == 0:
            if np.count_nonzero(y):
                bad.append("row %d (zero filter row %d): %d outputs are not zero" % (b, b % filters, np.count_nonzero(y)))
            continue
        mx, l2 = oracle.compare(y, ref)
        if not (mx <= cc.REL_TOL and l2 <= cc.REL_TOL):
            bad.append("row %d (filter row %d): max_rel %.3g rel_l2 %.3g" % (b, b % filters, mx, l2))
    for lo, hi in cold:
        y = buf.map_read(offset=lo * row, size=(hi - lo) * row, stream=enc)
        if np.count_nonzero(y):                               # by value: 0 * h may be -0
            bad.append("rows %d .. %d: %d outputs are not zero" % (lo, hi - 1, np.count_nonzero(y)))
    plan.destroy()
    enc.destroy()
    buf.destroy()
    bank.destroy()
    del t_x, t_h
    torch.cuda.empty_cache()
    return bad


@pytest.mark.parametrize("n", [32, 1024])
def test_src_and_dst_past_4gib(conv, gpu, oracle, n):
    """in place on 4 GiB + one workgroup + 3 rows; only the rows of the first workgroup, of the one that straddles byte
    offset 2^32 and of the last two (the last one partial) are non-zero; F = 3"""
    rpb = cc.rows_per_block(n)
    at4g = (1 << 32) // (n * 8)
    batch = at4g + rpb + 3
    assert batch * n * 8 > 1 << 32
    hot = sorted(set(range(rpb)) | set(range(at4g - 2, at4g + 2)) | set(range(batch - 3 - rpb, batch)))    # each row once
    cold = [(rpb, 2 * rpb), (at4g // 2, at4g // 2 + rpb), (at4g - rpb - 2, at4g - 2)]
    bad = _hot_rows_case(conv, gpu, oracle, n, batch, 3, hot, [0, 1, 2], cold)
    assert not bad, "\n".join(bad)


def test_filter_bank_past_4gib(conv, gpu, oracle):
    """n = 1024, a bank of 2^19 + 1 spectra (4 GiB + 8 KiB) and 2^19 + 19 rows: row 2^19 - 1 uses the spectrum that ends at
    byte 2^32, row 2^19 the one that starts there, row 2^19 + 1 wraps to spectrum 0.  The 64-bit filter row base."""
    n, F = 1024, (1 << 19) + 1
    batch = (1 << 19) + 19
    assert F * n * 8 > 1 << 32
    hot = [0, 5, F - 2, F - 1, F, F + 5, batch - 1]
    hot_filters = [0, F - 2, F - 1, (batch - 1) % F]                          # rows 5 and F + 5 meet a zero spectrum
    cold = [(16, 32), (F - 18, F - 2), (batch - 17, batch - 1)]
    bad = _hot_rows_case(conv, gpu, oracle, n, batch, F, hot, hot_filters, cold)
    assert not bad, "\n".join(bad)


# ---- ordering -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 256, 4096])
def test_execs_are_stream_ordered_and_allocate_nothing(conv, gpu, oracle, n):
    """filter written, exec and read-back on one non-null stream, no host synchronisation in between"""
    fw, dev, queue = gpu
    batch = cc.default_batch(n)
    x, H = cc.inputs(oracle, n, batch, 3)
    zeros = np.zeros_like(H)
    src, flt, dst = dev.create_buffer(x.nbytes), dev.create_buffer(H.nbytes), dev.create_buffer(x.nbytes)
    queue.write_buffer(src, 0, x)
    queue.write_buffer(flt, 0, zeros)
    enc = dev.create_command_encoder()
    plan = conv.Convolve(dev, queue, src, flt, dst, n)
    plan.proc(enc)                                        # a zero filter first: dst holds zeros
    queue.write_buffer(flt, 0, H, encoder=enc)
    plan.proc(enc)
    y = dst.map_read(stream=enc).reshape(batch, n)
    assert not cc.parity_failures(oracle, y, cc.cached_reference(oracle, n, batch, 3, "Convolve", False), "n %d" % n)
    dev.poll()
    before = dev.stats()["mem_free_bytes"]
    for _ in range(10):
        plan.proc(enc)
    dev.poll()
    assert dev.stats()["mem_free_bytes"] == before
    assert same_bits(dst.map_read(stream=enc).reshape(batch, n), y)
    for h in (plan, enc, src, flt, dst):
        h.destroy()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_status_codes(conv, gpu):
    fw, dev, queue = gpu
    L = conv.lib()
    n, batch, F = 64, 6, 3
    row = n * 8
    xb, hb, yb = dev.create_buffer(batch * row), dev.create_buffer(F * row), dev.create_buffer(batch * row)
    out = ctypes.c_void_p()

    def create(ctx, kind, flags, length, src, flt, dst):
        st = L.fwc_plan_create(ctx, kind, flags, length, src, flt, dst, ctypes.byref(out))
        if st == 0:
            L.fwc_plan_destroy(out)
        else:
            assert not out.value
        return st
    for kind in (1, 2):
        for flags in (0, 1):
            assert create(dev._h, kind, flags, n, xb._h, hb._h, yb._h) == 0
            assert create(dev._h, kind, flags, n, xb._h, hb._h, xb._h) == 0   # in place: the same handle
    # NULL handles
    assert create(None, 1, 0, n, xb._h, hb._h, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, None, hb._h, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, xb._h, None, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, xb._h, hb._h, None) == INVALID_ARG
    assert L.fwc_plan_create(dev._h, 1, 0, n, xb._h, hb._h, yb._h, None) == INVALID_ARG
    assert L.fwc_plan_exec(None, None) == INVALID_ARG
    # kinds and flags
    for kind in (0, 3, 4, -1):                                               # FWA_FORWARD, FWA_NORMALIZE, unknown kinds
        assert create(dev._h, kind, 0, n, xb._h, hb._h, yb._h) == INVALID_ARG
    for flags in (2, 3, 1 << 31):
        assert create(dev._h, 1, flags, n, xb._h, hb._h, yb._h) == INVALID_ARG
    # lengths
    for bad_len in (0, 48, 3):
        assert create(dev._h, 1, 0, bad_len, xb._h, hb._h, yb._h) == INVALID_ARG
    for length, word in ((1, "2 .. 4096"), (8192, "4096")):
        with pytest.raises(fw.FwaError) as e:
            conv.Convolve(dev, queue, xb, hb, yb, length)
        assert e.value.status == UNSUPPORTED and word in e.value.detail
    # a view that starts 8 bytes into a row cannot be made at all: the 16-byte accesses of n <= 32 rely on fwa_buf_wrap's rule
    with pytest.raises(fw.FwaError) as e:
        dev.wrap_buffer(xb.device_ptr + 8, row)
    assert e.value.status == INVALID_ARG and "16-byte aligned" in e.value.detail
    # sizes: not whole rows (src / dst, filter), src and dst that differ
    ragged = dev.wrap_buffer(xb.device_ptr, batch * row - 16)
    assert create(dev._h, 1, 0, n, ragged._h, hb._h, ragged._h) == INVALID_ARG
    ragged_filter = dev.wrap_buffer(hb.device_ptr, F * row - 16)
    assert create(dev._h, 1, 0, n, xb._h, ragged_filter._h, yb._h) == INVALID_ARG
    short = dev.wrap_buffer(yb.device_ptr, 4 * row)
    with pytest.raises(fw.FwaError) as e:
        conv.Convolve(dev, queue, xb, hb, short, n)
    assert e.value.status == INVALID_ARG and "batch" in e.value.detail
    assert create(dev._h, 1, 0, n, short._h, hb._h, xb._h) == INVALID_ARG
    # overlap: another handle on the same bytes is not "in place"; views that share 16 bytes; a filter inside dst
    alias = dev.wrap_buffer(xb.device_ptr, batch * row)
    with pytest.raises(fw.FwaError) as e:
        conv.Convolve(dev, queue, xb, hb, alias, n)
    assert e.value.status == INVALID_ARG and "overlap" in e.value.detail
    arena = dev.create_buffer(2 * row * 2 + F * row)
    v_src = dev.wrap_buffer(arena.device_ptr, 2 * row)
    v_over = dev.wrap_buffer(arena.device_ptr + 2 * row - 16, 2 * row)
    v_next = dev.wrap_buffer(arena.device_ptr + 2 * row, 2 * row)
    v_filter = dev.wrap_buffer(arena.device_ptr + 4 * row, F * row)
    assert create(dev._h, 1, 0, n, v_src._h, v_filter._h, v_over._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, v_over._h, v_filter._h, v_src._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, v_src._h, v_filter._h, v_next._h) == 0      # adjacent is fine
    f_in_dst = dev.wrap_buffer(arena.device_ptr + 3 * row, row)
    with pytest.raises(fw.FwaError) as e:
        conv.Convolve(dev, queue, v_src, f_in_dst, v_next, n)
    assert e.value.status == INVALID_ARG and "filter" in e.value.detail and "overlap" in e.value.detail
    assert create(dev._h, 1, 0, n, v_next._h, f_in_dst._h, v_next._h) == INVALID_ARG     # in place: dst is src, the filter inside it
    assert create(dev._h, 1, 0, n, v_next._h, f_in_dst._h, v_src._h) == 0      # a filter that overlaps src only is read twice: allowed
    # a buffer and a stream of another context; a buffer whose context was destroyed
    other = fw.Device(0)
    foreign = other.create_buffer(batch * row)
    assert create(dev._h, 1, 0, n, foreign._h, hb._h, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, xb._h, foreign._h, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, xb._h, hb._h, foreign._h) == INVALID_ARG
    plan = conv.Convolve(dev, queue, xb, hb, yb, n, conj_filter=True)
    foreign_stream = other.create_command_encoder()
    assert L.fwc_plan_exec(plan._h, foreign_stream._h) == INVALID_ARG
    stale_stream = other.create_command_encoder()
    other.destroy()
    assert create(dev._h, 1, 0, n, foreign._h, hb._h, yb._h) == INVALID_ARG
    assert create(dev._h, 1, 0, n, xb._h, foreign._h, yb._h) == INVALID_ARG
    assert L.fwc_plan_exec(plan._h, stale_stream._h) == INVALID_ARG
    v = ctypes.c_int64()
    assert L.fwc_plan_get_i64(plan._h, b"no_such_key", ctypes.byref(v)) == INVALID_ARG
    g = conv.describe(n, batch)
    assert {k: plan.get(k) for k in g} == g
    assert (plan.get("fft_len"), plan.get("batch"), plan.get("filters"), plan.get("in_place"), plan.get("launches_per_exec")) == (n, batch, F, 0, 1)
    plan.destroy()
    for h in (foreign, foreign_stream, stale_stream, ragged, ragged_filter, short, alias, v_src, v_over, v_next, v_filter, f_in_dst, arena,
              xb, hb, yb):
        h.destroy()


def test_a_plan_goes_before_its_context_and_a_stale_buffer_is_refused(conv, gpu, oracle):
    fw, dev, queue = gpu
    n, batch = 256, 5
    x, H = cc.inputs(oracle, n, batch, 3)
    other = fw.Device(0)
    q2 = fw.Queue(other)
    src, flt = other.create_buffer(x.nbytes), other.create_buffer(H.nbytes)
    q2.write_buffer(src, 0, x)
    q2.write_buffer(flt, 0, H)
    plan = conv.Convolve(other, q2, src, flt, src, n)
    enc = other.create_command_encoder()
    y = plan.proc(enc).map_read(stream=enc).reshape(batch, n)
    assert not cc.parity_failures(oracle, y, cc.cached_reference(oracle, n, batch, 3, "Convolve", False), "second context")
    plan.destroy()                                        # the plan first, then its context
    plan.destroy()                                        # and twice is harmless
    enc.destroy()
    other.destroy()
    out = ctypes.c_void_p()
    mine = dev.create_buffer(x.nbytes)
    L = conv.lib()
    assert L.fwc_plan_create(dev._h, 1, 0, n, src._h, flt._h, mine._h, ctypes.byref(out)) == INVALID_ARG and not out.value
    assert L.fwc_plan_create(dev._h, 1, 0, n, mine._h, flt._h, mine._h, ctypes.byref(out)) == INVALID_ARG and not out.value
    for h in (src, flt, mine):                            # still destroyable
        h.destroy()
