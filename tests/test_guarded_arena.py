"""not-gpu: the arithmetic and the checker of tests/guarded_arena.py, and the coverage of the containment case list.

A numpy array stands in for device memory, so the helper that the GPU containment tests trust is itself held to account
before it ever runs on a GPU."""
import numpy as np
import pytest

import guarded_arena as ga
import test_gpu_containment as tc
from oracle import error_budget as eb


def test_guard_size_is_the_stated_condition():
    assert ga.guard_bytes(2) == ga.guard_bytes(1 << 16) == 1 << 20           # 2 * 2^16 * 8 = 1 MiB
    assert ga.guard_bytes(1 << 17) == 2 << 20 and ga.guard_bytes(1 << 20) == 16 << 20
    assert ga.guard_bytes(1 << 22) == ga.guard_bytes(1 << 30) == 64 << 20
    for lg in range(1, 31):
        g = ga.guard_bytes(1 << lg)
        # at least sixteen 64-KiB chunks, at least two transforms up to the 64-MiB clamp, above what one workgroup handles
        assert g % 16 == 0 and g >= 16 * 65536 and (g >= 2 * 8 << lg or g == ga.MAX_GUARD) and g > 256 << 10


def test_start_offsets_are_16_byte_aligned_and_nothing_more():
    assert ga.START_EXTRAS == (0, 16, 4096 - 16, 65536 + 48)
    assert all(e % 16 == 0 for e in ga.START_EXTRAS)
    assert [e % 65536 for e in ga.START_EXTRAS[1:]] == [16, 4080, 48] and ga.START_EXTRAS[2] % 4096 and ga.START_EXTRAS[3] % 64


@pytest.mark.parametrize("sizes", [[8 * 64 * 5], [8 * 512 * 7, 8 * 512 * 7], [3 * 65536 + 4096 + 16, 3 * 65536 + 4096 + 16],
                                   [8, 24, 8 * 3]])
@pytest.mark.parametrize("extra", ga.START_EXTRAS)
def test_layout_is_aligned_guarded_and_without_overlap(sizes, extra):
    G = ga.guard_bytes(512)
    offs = ga.view_offsets(sizes, G + extra, G)
    total = ga.arena_bytes(sizes, G + extra, G)
    zones = ga.guard_zones(sizes, offs, G, total)
    assert offs[0] == G + extra and all(o % 16 == 0 for o in offs)
    assert len(zones) == len(sizes) + 1 and all(hi - lo >= G for lo, hi in zones)
    # views and zones tile [0, total) exactly: no overlap, no byte that is neither view nor checked guard
    pieces = sorted(zones + [(o, o + s) for o, s in zip(offs, sizes)])
    assert pieces[0][0] == 0 and pieces[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
    # windows only (the 4-GiB arena): exactly one guard on each outer side
    win = ga.guard_zones(sizes, offs, G, None)
    assert win[0] == (offs[0] - G, offs[0]) and win[-1] == (offs[-1] + sizes[-1], offs[-1] + sizes[-1] + G) and win[1:-1] == zones[1:-1]


@pytest.mark.parametrize("base", [0x7F2A00000000, 0x7F2A00000010, 0x7F29FFF00000, 0x7F2AFFFFFFF0, 0x7F2A80001230, 0x10])
@pytest.mark.parametrize("delta,nbytes", [(64 * 8 * 130 + 256, 64 * 8 * 449), (512 * 8 * 19, 512 * 8 * 57), ((8 << 22) // 2, 8 << 23)])
def test_straddle_placement(base, delta, nbytes):
    G = ga.guard_bytes(1 << 22)
    start = ga.straddle_start(base, delta, G)
    total = ga.straddle_arena_bytes([nbytes, nbytes], G)
    assert start % 16 == 0 and G <= start < G + ga.FOUR_GIB
    lo = base + start
    assert (lo + delta) % ga.FOUR_GIB == 0 and lo // ga.FOUR_GIB + 1 == (lo + nbytes - 1) // ga.FOUR_GIB
    # both views and the guard behind them fit into the arena wherever the allocation landed
    offs = ga.view_offsets([nbytes, nbytes], start, G)
    assert ga.guard_zones([nbytes, nbytes], offs, G, None)[-1][1] <= total
    # the boundary in the SECOND view: shift by the distance of the two views
    second = ga.view_offsets([nbytes, nbytes], G, G)[1] - G
    start2 = ga.straddle_start(base, delta + second, G)
    offs2 = ga.view_offsets([nbytes, nbytes], start2, G)
    assert (base + offs2[1] + delta) % ga.FOUR_GIB == 0 and ga.guard_zones([nbytes, nbytes], offs2, G, None)[-1][1] <= total


class _FakeArena:
    """device memory as a numpy array"""

    def __init__(self, sizes, start, guard):
        self.sizes, self.offs = sizes, ga.view_offsets(sizes, start, guard)
        self.total = ga.arena_bytes(sizes, start, guard)
        self.zones = ga.guard_zones(sizes, self.offs, guard, self.total)
        self.mem = np.full(self.total // 4, ga.SENTINEL, dtype=np.uint32)
        self.reads = 0
        self.baits = []

    def read(self, lo, hi):
        assert lo % 4 == 0 and hi % 4 == 0
        self.reads += hi - lo
        return self.mem[lo // 4:hi // 4]

    def changes(self, limit=8):
        return ga.find_changes(self.read, self.zones, self.sizes, self.offs, ["src", "src2"], limit, self.baits)


def test_checker_reports_single_changed_bytes_with_signed_distance():
    G = ga.MIN_GUARD
    sizes = [8 * 64 * 5 + 8, 8 * 64 * 5 + 8]             # ends 8 mod 16: the next view is rounded up
    a = _FakeArena(sizes, G + 16, G)
    assert a.changes() == []
    assert a.reads == a.total - sum(sizes)                # every guard byte is read, no sampling
    o0, o1 = a.offs
    e0, e1 = o0 + sizes[0], o1 + sizes[1]
    by = a.mem.view(np.uint8)
    cases = [
        (0, 0, -o0),                      # the first guard byte of the arena
        (a.total - 1, 1, a.total - 1 - e1),   # the last one
        (o0 - 1, 0, -1),                  # the last byte before src
        (e0, 0, 0),                       # the first byte past the end of src
        (e0 + 65536, 0, 65536),           # one chunk past the end of src
        (o1 - 3, 1, -3),                  # in the guard between the views, nearer to src2
        (e1 + 8 * 512 + 5, 1, 8 * 512 + 5),
    ]
    for off, view, dist in cases:
        old = by[off]
        by[off] ^= 0x40
        got = a.changes()
        assert len(got) == 1 and got[0][:3] == (off, view, dist), (off, got)
        msg = got[0][3]
        assert ("%d bytes past the end of %s" % (dist, ["src", "src2"][view]) in msg) if dist >= 0 \
            else ("%d bytes before the start of %s" % (-dist, ["src", "src2"][view]) in msg)
        by[off] = old
    assert a.changes() == []


def test_checker_ignores_views_and_limits_its_report():
    G = ga.MIN_GUARD
    sizes = [4096, 4096]
    a = _FakeArena(sizes, G, G)
    by = a.mem.view(np.uint8)
    for o, s in zip(a.offs, sizes):                      # anything may happen inside a view
        by[o:o + s] = 0
    assert a.changes() == []
    e1 = a.offs[1] + sizes[1]
    a.mem[e1 // 4:e1 // 4 + 16384] = 0x3F800000          # a 64-KiB overrun behind src2
    got = a.changes(limit=3)
    assert [g[:3] for g in got] == [(e1, 1, 0), (e1 + 4, 1, 4), (e1 + 8, 1, 8)]
    a.mem[(a.offs[0] - 8) // 4] = 0
    assert a.changes(limit=3)[0][:3] == (a.offs[0] - 8, 0, -8)   # address order: the zone in front of src comes first
    with pytest.raises(AssertionError):
        ga.signed_distance(a.offs[0], sizes, a.offs)


def test_read_bait_makes_a_carried_over_guard_visible():
    """An out-of-place elementwise kernel whose surplus lanes run 64 KiB past both views: with the sentinel on both sides it
    writes what is already there; with the bait behind the read view the guard behind the written view changes."""
    G = ga.MIN_GUARD
    sizes = [8 * 64 * 3, 8 * 64 * 3]
    a = _FakeArena(sizes, G + 16, G)
    e0, e1 = (o + s for o, s in zip(a.offs, sizes))
    over = 65536 // 4
    a.mem[e1 // 4:e1 // 4 + over] = a.mem[e0 // 4:e0 // 4 + over]          # sentinel carried over: invisible
    assert a.changes() == []
    bait = ga.bait_words()
    assert bait.size * 4 == ga.BAIT_BYTES and np.isfinite(bait.view(np.float32)).all() and (bait != ga.SENTINEL).all()
    assert (np.abs(bait.view(np.float32)) >= 2).all() and (bait[1:] != bait[:-1]).all()
    a.mem[e0 // 4:e0 // 4 + bait.size] = bait
    a.baits.append(e0)
    assert a.changes() == []                                               # the bait itself is expected
    a.mem[e1 // 4:e1 // 4 + over] = (a.mem[e0 // 4:e0 // 4 + over].view(np.float32) / 64).view(np.uint32)
    got = a.changes(limit=2)
    assert [g[:3] for g in got] == [(e1, 1, 0), (e1 + 4, 1, 4)]
    a.mem[e1 // 4:e1 // 4 + over] = ga.SENTINEL
    a.mem[e0 // 4 + 5] ^= 0x100                                            # a write into the bait is a guard write too
    assert a.changes()[0][:3] == (e0 + 21, 0, 21)


def test_sentinel_is_a_quiet_nan_in_both_halves():
    w = np.array([ga.SENTINEL, ga.SENTINEL], dtype=np.uint32)
    assert np.isnan(w.view(np.float32)).all() and np.isnan(w.view(np.complex64)).all()
    assert ga.SENTINEL & 0x7FC00000 == 0x7FC00000          # exponent all ones, quiet bit set
    # NaN-propagating: a result fed by a stray read cannot pass the suite's comparisons
    y = np.ones(64, dtype=np.complex64)
    y[7] = w.view(np.complex64)[0]
    rel_l2, max_rel = eb.metrics(y, np.ones(64, dtype=np.complex128), 64)
    assert not rel_l2 <= 1.0 and not max_rel <= 1.0
    assert tc._dft_failures(y, np.ones(64, dtype=np.complex128), 64) == [0]
    assert tc._dft_failures(np.ones(128, dtype=np.complex64), np.ones(128, dtype=np.complex128), 64) == []


def test_every_family_of_the_error_budget_has_containment_cases():
    assert tc.families_without_cases() == []
    # a family added to the error-budget list on a path the containment cases do not know fails, it is not passed over
    new = ("future_family", 1 << 12, 4, {}, (9, 12, 1), "k_future")
    assert tc.families_without_cases(list(eb._CASES) + [new], tc.build_specs(list(eb._CASES) + [new])) == ["future_family"]
    # ... and one on a known path is covered without a change here
    new = ("future_tiled", 1 << 18, 5, {}, (7, eb._f(8, 10), 2), "k_future")
    specs = tc.build_specs([new])
    assert [s["id"] for s in specs] == ["future_tiled/x5", "future_tiled/group2_streams2_x5"] and specs[1]["launches"] == 6


def test_containment_cases_follow_the_issue():
    by_family = {}
    for s in tc.SPECS:
        by_family.setdefault(s["family"], []).append(s)
    for cid, n, batch, tun, (path, factors, launches), _ in eb._CASES:
        specs = by_family[cid]
        for s in specs:
            runs = dict(s["runs"])
            assert {"Forward", "Onlyinverse", "Inverse"} <= set(runs) or "g7xx" in s["id"]
            assert all(16 in e for e in runs.values())
            assert (s["n"], s["path"], s["factors"]) == (n, path, factors)
        if path == 0:
            per = tc.per_wg(n)
            for s in specs:
                assert per == 1 or 0 < s["batch"] % per < per
                assert dict(s["runs"])["Forward"] == dict(s["runs"])["Onlyinverse"] == ga.START_EXTRAS
            grids = sorted(-(-s["batch"] // per) for s in specs)
            assert grids[0] < 512 and ((512 < grids[-1] < 1024) == (n in tc.BIG_GRID_N))
        else:
            assert specs[0]["batch"] == batch and specs[0]["tunables"] == tun
            assert specs[0]["batch"] * n * 8 * 2 + 3 * ga.guard_bytes(n) < 1.5 * 2 ** 30
            if path != 2 and batch > 2:
                g = specs[1]
                assert g["batch"] % 2 == 1 and g["tunables"]["group"] == 2 and g["tunables"]["streams"] == 2
                assert g["launches"] == launches * -(-g["batch"] // 2)
            if cid in tc.ALL_OFFSET_ROWS:
                assert dict(specs[0]["runs"])["Forward"] == ga.START_EXTRAS
    assert set(tc.ALL_OFFSET_ROWS) <= set(by_family)
