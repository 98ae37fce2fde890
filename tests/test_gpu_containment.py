"""GPU: every kernel family and every entry point that writes device memory stays inside the buffer views it is given.

The other GPU tests ask whether the bytes inside a result buffer are right.  These ask whether the library touched only
the bytes it was handed: every plan runs on views wrapped (Device.wrap_buffer, the zero-copy seam fwa_buf_wrap) somewhere
INSIDE one allocation, between guard zones filled with a NaN sentinel (tests/guarded_arena.py).  Per case, all three:

  (a) no guard byte changed (every guard byte of the arena is read back, no sampling);
  (b) the result is bit-identical to the result of the same input, plan kind and tunables on fresh buffers at an
      allocation base -- placement must not change a bit -- and that base result is compared once, per transform, with
      the fp64 DFT at REL_TOL, so that "identical" cannot mean "identically wrong".  A stray read of a guard word that
      feeds a result makes it NaN and fails here;
  (c) the plan took the path / factors / launch count the case names, so a case cannot stop exercising its kernel.

Forward / Inverse with odd log2 n write their result into the plan's own second buffer, which cannot be guarded from
outside the library: (a) then only proves that the SOURCE side stays contained.  Onlyinverse runs on two views of one arena
(src, guard, src2) and so gives the odd-log2-n kernels a guarded destination as well.

The family list is oracle.error_budget._CASES: a family added there gets its cases here by its path, and a family with no
containment case fails test_every_family_has_containment_cases (also run without a GPU, tests/test_guarded_arena.py).
The literal recurrence (path 2) has no groups or chains: it runs without the group = 2, streams = 2 variant.

Not reachable through the ABI, so not a case: a plan on a misaligned buffer (plan.cpp refuses it, but fwa_buf_alloc and
fwa_buf_wrap never hand out a buffer that is not 16-byte aligned; the wrap rejection is tested).
"""
import numpy as np
import pytest

import guarded_arena as ga
from conftest import REL_TOL
from oracle import error_budget as eb
from oracle.device_run import FACTS, facts_of, open_gpu, parity_failures, run

pytestmark = pytest.mark.gpu

KINDS = ("Forward", "Inverse", "Onlyinverse")
DIRECTION = {"Forward": -1, "Inverse": 1, "Onlyinverse": 1}
ALL_EXTRAS = ga.START_EXTRAS
ONE_EXTRA = (16,)
BIG_GRID_N = (2, 64, 256, 512, 4096, 32768)          # also on a grid of 513 .. 1023 blocks
ALL_OFFSET_ROWS = ("pipeline_2^20x4", "tile_2^16x4", "colsw_8_2^17x9", "p1_gen_2^21x2")


def per_wg(n):
    """transforms per workgroup of the one-launch kernels (launch_chunk / small32_xpw)"""
    return 8192 // n if n <= 256 else max(1, 256 // (n // 32))


def _spec(sid, family, n, batch, tunables, path, factors, launches, runs):
    return dict(id=sid, family=family, n=n, batch=batch, tunables=dict(tunables), path=path, factors=factors,
                launches=launches, runs=runs)


def build_specs(cases=None):
    """One spec per (family, batch / tunables variant); spec["runs"] = [(kind, start extras)]."""
    specs = []
    for cid, n, batch, tun, (path, factors, launches), _kernels in (eb._CASES if cases is None else cases):
        if path == 0:
            # one launch: ragged last workgroup (k * per_wg + r, 0 < r < per_wg) where a workgroup holds several transforms;
            # a grid below 512 blocks (plain block map) and, at six lengths, one of 513 .. 1023 (mapped prefix + plain tail)
            per = per_wg(n)
            r = per // 2 + 1 if per > 2 else per - 1
            grids = [("g4", 3 * per + r)]
            if n in BIG_GRID_N:
                grids.append(("g7xx", (530 if n == 32768 else 700) * per + r))
            for tag, b in grids:
                blocks = -(-b // per)
                assert (blocks < 512) if tag == "g4" else (512 < blocks < 1024)
                assert per == 1 or 0 < b % per < per
                runs = [("Forward", ALL_EXTRAS), ("Onlyinverse", ALL_EXTRAS)] + ([("Inverse", ONE_EXTRA)] if tag == "g4" else [])
                specs.append(_spec("%s/%s_x%d" % (cid, tag, b), cid, n, b, tun, path, factors, launches, runs))
        elif path in (1, 2, 7):
            wide = cid in ALL_OFFSET_ROWS
            runs = [("Forward", ALL_EXTRAS if wide else ONE_EXTRA), ("Onlyinverse", ALL_EXTRAS if wide else ONE_EXTRA),
                    ("Inverse", ONE_EXTRA)]
            specs.append(_spec("%s/x%d" % (cid, batch), cid, n, batch, tun, path, factors, launches, runs))
            if path != 2 and batch > 2:
                # ragged last group on both chains: group = 2, streams = 2, odd batch
                b = batch | 1
                t = dict(tun, group=2, streams=2)
                ng = -(-b // 2)
                specs.append(_spec("%s/group2_streams2_x%d" % (cid, b), cid, n, b, t, path, factors, launches * ng,
                                   [("Forward", ONE_EXTRA), ("Onlyinverse", ONE_EXTRA), ("Inverse", ONE_EXTRA)]))
    return specs


SPECS = build_specs()
N_RUNS = sum(len(extras) for s in SPECS for _, extras in s["runs"])


def families_without_cases(cases=None, specs=None):
    have = {s["family"] for s in (SPECS if specs is None else specs)}
    return [c[0] for c in (eb._CASES if cases is None else cases) if c[0] not in have]


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


def _in_arena(fw, dev, queue, kind, n, x, tunables, extra, arena=None, start=None):
    """device_run.run on views inside a guarded arena -> (result, where, facts, guard reports)"""
    G = ga.guard_bytes(n)
    sizes = [x.nbytes, x.nbytes] if kind == "Onlyinverse" else [x.nbytes]
    own = arena is None
    if own:
        start = G + extra
        arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, start, G), G)
    views = arena.layout(sizes, start, names=["src", "src2"][:len(sizes)], whole=own)
    assert all(v.device_ptr % 16 == 0 and v.device_ptr != arena.device_ptr for v in views)
    src, src2 = views[0], (views[1] if len(views) > 1 else None)
    y, where, facts = run(fw, dev, queue, kind, x, n, tunables, buffers=(src, src2))
    reports = arena.check()
    for v in views:
        v.destroy()
    arena.views = []
    if own:
        arena.destroy()
    return y, where, facts, reports


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dft_failures(y, r, n, tol=REL_TOL):
    """the first transforms that miss the parity rule; NaN fails"""
    return [t for t, _, _ in parity_failures(y, r, n, tol)[0][:8]]


def _run_spec(gpu, oracle, spec, runs=None, arena=None, start_of=None):
    """Assertions (a) - (c) for every (kind, start extra) of the spec; the input and its two fp64 DFTs are computed once."""
    fw, dev, queue = gpu
    n, batch, tun = spec["n"], spec["batch"], spec["tunables"]
    want = dict(zip(FACTS, (spec["path"], spec["factors"], spec["launches"])))
    x = oracle.gen_input(n, batch, first_transform=3)
    dft = {}
    bad = []
    for kind, extras in (spec["runs"] if runs is None else runs):
        tag = "%s/%s" % (spec["id"], kind)
        base, base_where, facts = run(fw, dev, queue, kind, x, n, tun)   # as the parity tests: fresh buffers at an allocation base
        if facts != want:
            bad.append("%s: plan took path/factors/launches %s, the case names %s" % (tag, facts, want))
        d = DIRECTION[kind]
        if d not in dft:
            dft[d] = oracle.dft_f64(x, n, d)
        off = _dft_failures(base, dft[d] / n if kind == "Inverse" else dft[d], n)
        if off:
            bad.append("%s: base-buffer result misses the fp64 DFT at transforms %s" % (tag, off[:8]))
        for extra in extras:
            st = None if start_of is None else start_of(kind, extra)
            y, where, facts, reports = _in_arena(fw, dev, queue, kind, n, x, tun, extra, arena, st)
            at = "%s @ %s" % (tag, "G + %d" % extra if start_of is None else "boundary in view %d" % extra)
            bad += ["%s: %s" % (at, m) for m in reports]                                      # (a)
            if not _same_bits(y, base):                                                       # (b)
                k = np.flatnonzero(y.view(np.uint32) != base.view(np.uint32))
                bad.append("%s: result differs from the base-buffer result in %d words, first at sample %d of transform %d "
                           "(NaN there: %s)" % (at, k.size, (k[0] // 2) % n, (k[0] // 2) // n, bool(np.isnan(y.view(np.float32)[k[0]]))))
            if facts != want or where != base_where:                                          # (c)
                bad.append("%s: plan took %s into %s, the case names %s into %s" % (at, facts, where, want, base_where))
    return bad


def test_every_family_has_containment_cases():
    assert not families_without_cases(), families_without_cases()
    for cid in ALL_OFFSET_ROWS:
        assert any(s["family"] == cid for s in SPECS), cid
    for s in SPECS:
        kinds = {k for k, _ in s["runs"]}
        assert {"Forward", "Onlyinverse"} <= kinds and all(16 in e for _, e in s["runs"]), s["id"]
    print("containment: %d plan cases (kind x start offset) in %d specs" % (N_RUNS, len(SPECS)))


@pytest.mark.parametrize("spec", SPECS, ids=[s["id"] for s in SPECS])
def test_plan_stays_inside_its_views(gpu, oracle, spec):
    bad = _run_spec(gpu, oracle, spec)
    assert not bad, "\n".join(bad)


# ---- Normalize (k_scale), out of place, ragged last chunk ----
@pytest.mark.parametrize("n,batch", [(64, 700 * 128 + 3), (512, 16 * 700 + 5)])
def test_normalize_reads_one_view_and_writes_the_other(gpu, oracle, n, batch):
    """n = 64 (even log2): reads buffer1, writes buffer2; n = 512 (odd): reads buffer2, writes buffer1.  701 workgroups, the
    last chunk partial.  Bit-exact against the oracle; the READ view keeps every bit; no guard byte changes."""
    fw, dev, queue = gpu
    x = oracle.gen_input(n, batch, first_transform=5)
    G = ga.guard_bytes(n)
    sizes = [x.nbytes, x.nbytes]
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, G + 16, G), G)
    b1, b2 = arena.layout(sizes, G + 16, names=["buffer1", "buffer2"])
    even = (n.bit_length() - 1) % 2 == 0
    rd, wr = (b1, b2) if even else (b2, b1)
    arena.bait(0 if even else 1)                         # what a surplus lane reads behind the read view is not the sentinel
    queue.write_buffer(rd, 0, x)
    enc = dev.create_command_encoder()
    plan = fw.Normalize(dev, queue, b1, b2, n)
    out = plan.proc(enc)
    assert out is wr
    got = out.map_read(stream=enc)
    reports = arena.check()
    assert not reports, "\n".join(reports)
    assert _same_bits(got, oracle.normalize_ref(x, n))
    assert _same_bits(rd.map_read(), x)
    plan.destroy()
    arena.destroy()


# ---- the entry points that write device memory without a plan ----
@pytest.mark.parametrize("nbytes", [3 * 65536 + 4096 + 16, 700 * 65536 + 1536])
def test_calib_copy_stays_inside_its_views(gpu, oracle, nbytes):
    """fwa_calib_copy out of place (k_copy chunks + k_copy_tail vectors) and in place (k_scale with scale 1)."""
    fw, dev, queue = gpu
    x = oracle.gen_input(nbytes // 8, 1, first_transform=9)
    G = ga.MIN_GUARD
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes([nbytes, nbytes], G + 16, G), G)
    src, dst = arena.layout([nbytes, nbytes], G + 16, names=["src", "dst"])
    arena.bait(0)
    queue.write_buffer(src, 0, x)
    dev.calib_copy(dst, src, nbytes)
    reports = arena.check()
    assert not reports, "\n".join(reports)
    assert _same_bits(dst.map_read(), x) and _same_bits(src.map_read(), x)
    dev.calib_copy(src, src, nbytes)                     # in place
    reports = arena.check()
    assert not reports, "\n".join(reports)
    assert _same_bits(src.map_read(), x) and _same_bits(dst.map_read(), x)
    arena.destroy()


def test_fill_synthetic_stays_inside_its_view(gpu, oracle):
    fw, dev, queue = gpu
    n, batch = 64, 3 * 128 + 5                           # three whole 64-KiB chunks and a partial one
    G = ga.guard_bytes(n)
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes([n * batch * 8], G + 16, G), G)
    (view,) = arena.layout([n * batch * 8], G + 16, names=["dst"])
    dev.fill_synthetic(view, n, first_transform=3)
    reports = arena.check()
    assert not reports, "\n".join(reports)
    assert _same_bits(view.map_read(), oracle.gen_input(n, batch, first_transform=3))
    arena.destroy()


def test_buffer_copies_and_host_transfers_with_offsets_into_views(gpu, oracle):
    """fwa_buf_copy between two views with non-zero offsets on both sides; queue.write_buffer / map_read with offsets into a
    view (bound-checked on the host: a range past the end of the VIEW is refused although the arena goes on)."""
    fw, dev, queue = gpu
    nbytes = 65536 + 4096
    x = oracle.gen_input(nbytes // 8, 1, first_transform=11)
    G = ga.MIN_GUARD
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes([nbytes, nbytes], G + 16, G), G)
    a, b = arena.layout([nbytes, nbytes], G + 16, names=["a", "b"])
    queue.write_buffer(a, 0, x)
    enc = dev.create_command_encoder()
    enc.copy_buffer_to_buffer(a, 4096, b, 1024, nbytes - 4096)           # ends 3072 bytes before the end of b
    enc.synchronize()
    reports = arena.check()
    assert not reports, "\n".join(reports)
    got = b.map_read().view(np.uint32)
    assert np.array_equal(got[256:256 + (nbytes - 4096) // 4], x.view(np.uint32)[1024:])
    assert (got[:256] == ga.SENTINEL).all() and (got[256 + (nbytes - 4096) // 4:] == ga.SENTINEL).all()
    # host transfers with offsets: the last 512 bytes of the view, then one byte range too far
    queue.write_buffer(b, nbytes - 512, x[:64])
    assert _same_bits(b.map_read(offset=nbytes - 512, size=512), x[:64])
    assert not arena.check()
    for call in (lambda: queue.write_buffer(b, nbytes - 504, x[:64]), lambda: b.map_read(offset=nbytes - 504, size=512),
                 lambda: enc.copy_buffer_to_buffer(a, 8, b, nbytes - 504, 512)):
        with pytest.raises(fw.FwaError) as e:
            call()
        assert e.value.status == 1
    assert not arena.check()
    arena.destroy()


def test_rejects_misaligned_and_overlapping_views(gpu):
    fw, dev, queue = gpu
    n, batch = 512, 4
    size = n * batch * 8
    arena = dev.create_buffer(4 * size)
    p = arena.device_ptr
    with pytest.raises(fw.FwaError) as e:
        dev.wrap_buffer(p + 8, size)                     # 16-byte alignment is the one placement rule
    assert e.value.status == 1
    at = 16 + size
    a = dev.wrap_buffer(p + at, size)
    for off in (at + size - n * 8, at - size + n * 8, at + size - 16):   # one transform shared (behind, in front), 16 bytes
        b = dev.wrap_buffer(p + off, size)
        for mk in (fw.Onlyinverse, fw.Normalize):
            with pytest.raises(fw.FwaError) as e:
                mk(dev, queue, a, b, n)
            assert e.value.status == 1 and "overlap" in str(e.value)
            with pytest.raises(fw.FwaError):
                mk(dev, queue, b, a, n)
    with pytest.raises(fw.FwaError) as e:
        fw.Onlyinverse(dev, queue, a, dev.wrap_buffer(p + at, size), n)   # the same memory through two handles
    assert e.value.status == 1 and "distinct" in str(e.value)
    touching = dev.wrap_buffer(p + at + size, size)      # adjacent views share no byte: accepted
    fw.Onlyinverse(dev, queue, a, touching, n).destroy()
    fw.Normalize(dev, queue, touching, a, n).destroy()


# ---- re-exec on poisoned destinations ----
@pytest.mark.parametrize("kind,n,batch,tunables,want", [
    ("Onlyinverse", 512, 2500, {}, (0, 9, 1)),
    ("Forward", 1 << 20, 5, {"group": 2, "streams": 2}, (1, eb._f(10, 10), 6)),
    ("Forward", 1 << 18, 7, {"group": 2, "streams": 2}, (7, eb._f(8, 10), 8)),
])
def test_three_execs_back_to_back_on_poisoned_destinations(gpu, oracle, kind, n, batch, tunables, want):
    """One plan, three execs on one stream with no host synchronisation in between; before each exec the destination view is
    re-poisoned and fresh input uploaded, both stream-ordered; each result is parked by a stream-ordered copy.  Each must be
    bit-identical to a single exec of the same input: an exec that left part of its destination to the previous exec's
    (identical-looking) result shows here and nowhere else."""
    fw, dev, queue = gpu
    xs = [oracle.gen_input(n, batch, first_transform=100 * i) for i in range(3)]
    singles = [run(fw, dev, queue, kind, x, n, tunables)[0] for x in xs]
    bad = _dft_failures(singles[0], oracle.dft_f64(xs[0], n, DIRECTION[kind]), n)
    assert not bad, bad
    G = ga.guard_bytes(n)
    nbytes = xs[0].nbytes
    sizes = [nbytes, nbytes] if kind == "Onlyinverse" else [nbytes]
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, G + 16, G), G)
    views = arena.layout(sizes, G + 16, names=["src", "src2"][:len(sizes)])
    src, src2 = views[0], (views[1] if len(views) > 1 else None)
    plan = fw.plan_of_kind(kind, dev, queue, src, src2, n)
    plan.configure(tunables)
    assert facts_of(plan) == dict(zip(FACTS, want))
    dest = 1 if (kind == "Onlyinverse" and (n.bit_length() - 1) % 2) else 0
    keep = [dev.create_buffer(nbytes) for _ in xs]
    # page-locked staging: the uploads are truly asynchronous, nothing between two execs waits on the host
    n_pinned = len(getattr(dev, "_pinned", []))
    poison = dev.pinned_array(nbytes // 4, dtype=np.uint32)
    poison[:] = ga.SENTINEL
    staged = [dev.pinned_array(x.size) for x in xs]
    for s, x in zip(staged, xs):
        s[:] = x
    enc = dev.create_command_encoder()
    for s, k in zip(staged, keep):
        queue.write_buffer(views[dest], 0, poison, encoder=enc)
        queue.write_buffer(src, 0, s, encoder=enc)
        out = plan.proc(enc)
        assert out is views[dest]
        enc.copy_buffer_to_buffer(out, 0, k, 0, nbytes)
    enc.synchronize()
    del poison, staged
    while len(dev._pinned) > n_pinned:
        dev._L.fwa_host_free(dev._h, dev._pinned.pop())
    for i, (k, one) in enumerate(zip(keep, singles)):
        assert _same_bits(k.map_read(), one), "exec %d differs from a single exec of the same input" % i
    reports = arena.check()
    assert not reports, "\n".join(reports)
    plan.destroy()
    arena.destroy()


# ---- a view that straddles a 4-GiB address boundary ----
_STRADDLE = [
    # id, n, batch, tunables, (path, factors, launches), boundary positions: transforms into the view (x.5 = mid-transform)
    ("chunk_64", 64, 3 * 128 + 65, {}, (0, 6, 1), (130.5, 129.0)),            # inside a workgroup's 128 transforms
    ("small32_512", 512, 3 * 16 + 9, {}, (0, 9, 1), (18.5, 19.0)),            # workgroup 1 holds transforms 16 .. 31
    ("small32_8192", 8192, 3, {}, (0, 13, 1), (1.5,)),
    ("pipeline_2^20x4", 1 << 20, 4, {}, (1, eb._f(10, 10), 2), (1.5,)),
    ("colsw_8_2^17x9", 1 << 17, 9, {}, (7, eb._f(8, 9), 2), (4.5,)),
    ("p1_gen_2^22x2", 1 << 22, 2, {}, (7, eb._f(10, 12), 2), (0.5,)),
]


@pytest.fixture(scope="module")
def big_arena(gpu):
    fw, dev, queue = gpu
    if dev.info()["hbm_bytes"] < 48 * 2 ** 30:
        pytest.skip("needs a 4-GiB arena beside the buffers of the other tests")
    G = ga.guard_bytes(1 << 22)
    arena = ga.GuardedArena(dev, queue, ga.straddle_arena_bytes([8 << 22 << 1, 8 << 22 << 1], G), G)
    yield arena
    arena.destroy()


@pytest.mark.parametrize("case", _STRADDLE, ids=[c[0] for c in _STRADDLE])
def test_view_straddling_a_4gib_address_boundary(gpu, oracle, big_arena, case):
    """The 32-GiB tests cover element offsets above 2^32 from an allocation base; here base + offset carries across a multiple
    of 2^32 in the virtual address (i) in the middle of a transform and (ii) between two transforms of one workgroup, in the
    source view and (Onlyinverse) in the destination view.  Only the guard windows around the views are poisoned and checked."""
    fw, dev, queue = gpu
    cid, n, batch, tun, want, positions = case
    spec = _spec("straddle/" + cid, cid, n, batch, tun, *want, runs=None)
    nbytes = n * batch * 8
    G = big_arena.guard = ga.guard_bytes(n)
    bad = []
    for pos in positions:
        delta = int(pos * n * 8)
        assert delta % 16 == 0 and 0 < delta < nbytes

        def start_of(kind, in_view):
            # the boundary falls `delta` bytes into view `in_view` (0: src, 1: src2 of Onlyinverse)
            second = ga.view_offsets([nbytes, nbytes], G, G)[1] - G
            start = ga.straddle_start(big_arena.device_ptr, delta + (second if in_view else 0), G)
            lo = big_arena.device_ptr + start + (second if in_view else 0)
            assert lo < lo + delta and (lo + delta) % ga.FOUR_GIB == 0 and lo // ga.FOUR_GIB + 1 == (lo + nbytes - 1) // ga.FOUR_GIB
            return start
        runs = [("Forward", (0,)), ("Onlyinverse", (0, 1))]
        bad += ["boundary %.1f transforms into the view: %s" % (pos, m)
                for m in _run_spec(gpu, oracle, spec, runs, big_arena, start_of)]
    assert not bad, "\n".join(bad)


def test_normalize_on_views_straddling_a_4gib_address_boundary(gpu, oracle, big_arena):
    fw, dev, queue = gpu
    n, batch = 64, 3 * 128 + 65
    x = oracle.gen_input(n, batch, first_transform=5)
    nbytes = x.nbytes
    G = big_arena.guard = ga.guard_bytes(n)
    second = ga.view_offsets([nbytes, nbytes], G, G)[1] - G
    for pos in (130.5, 129.0):
        for in_view in (0, 1):                            # the boundary in the view that is read, then in the one written
            start = ga.straddle_start(big_arena.device_ptr, int(pos * n * 8) + (second if in_view else 0), G)
            b1, b2 = big_arena.layout([nbytes, nbytes], start, names=["buffer1", "buffer2"], whole=False)
            big_arena.bait(0)
            queue.write_buffer(b1, 0, x)
            enc = dev.create_command_encoder()
            plan = fw.Normalize(dev, queue, b1, b2, n)
            out = plan.proc(enc)
            assert out is b2
            got = out.map_read(stream=enc)
            reports = big_arena.check()
            assert not reports, "\n".join(reports)
            assert _same_bits(got, oracle.normalize_ref(x, n)) and _same_bits(b1.map_read(), x)
            plan.destroy()
            for v in (b1, b2):
                v.destroy()
            big_arena.views = []
