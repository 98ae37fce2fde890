"""Guarded arena (TEST INFRASTRUCTURE ONLY): one device allocation that holds views separated and surrounded by guard zones.

The parity tests ask whether the bytes inside a result buffer are right.  This helper lets a test ask the other
question: did the library touch only the bytes it was given?  Every 32-bit word of the arena is first set to SENTINEL, a
quiet NaN with a recognisable payload (in the re and in the im half of every sample).  A stray WRITE changes a guard word
and `check` reports it; a stray READ that feeds a result turns that result into NaN, which every comparison of the suite
rejects; a destination that an exec leaves partly unwritten still holds NaN and cannot pass by luck.

Layout: guard | view 0 | guard | view 1 | ... | guard.  Every view starts on a 16-byte boundary (the ABI's only placement
rule, fwa_buf_wrap) and is wrapped with Device.wrap_buffer, i.e. it does NOT start at an allocation base unless asked to.
The guard size is a condition, not a measurement: guard_bytes(n) = clamp(2 * n * 8, 1 MiB, 64 MiB) -- at least two
transforms and at least sixteen 64-KiB chunks, larger than anything one workgroup of any kernel family handles (a
16 Ki-point first-pass tile = 128 KiB, a 64-KiB chunk, one 2^15 transform = 256 KiB).

Read bait.  A surplus lane of an out-of-place elementwise kernel (k_scale, k_copy) that reads the sentinel behind its source
and writes f(sentinel) behind its destination writes the sentinel again (a NaN keeps its payload through a multiply or a
copy): invisible.  `bait(i)` therefore replaces the first BAIT_BYTES of the guard behind view i by finite, position-dependent
words, which `check` then expects there; carried over behind another view they change its guard.  Only the tests whose
results are compared bit for bit with an independent answer use it (a stray read of the bait gives a finite wrong value,
not a NaN).

The arithmetic (view_offsets, arena_bytes, straddle_start, guard_zones) and the checker (find_changes) are plain numpy /
integers and are tested without a GPU in tests/test_guarded_arena.py.
"""
import numpy as np

SENTINEL = 0x7FC5A5A5
MIN_GUARD = 1 << 20
MAX_GUARD = 64 << 20
ALIGN = 16
FOUR_GIB = 1 << 32
# added to the guard size: the first view then starts at G + 0, G + 16, G + 4096 - 16, G + 65536 + 48 -- 16-byte aligned and
# nothing more ("64-KiB-aligned chunks" in the kernel sources means relative to the buffer, not to the address)
START_EXTRAS = (0, 16, 4096 - 16, 65536 + 48)
BAIT_BYTES = 128 << 10      # two 64-KiB chunks: more than the surplus lanes of one workgroup of an elementwise kernel reach


def bait_words(nbytes=BAIT_BYTES):
    """finite floats in [2, 4), every word different from its neighbours and from SENTINEL"""
    return np.uint32(0x40000000) | (np.arange(nbytes // 4, dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(10))


def guard_bytes(n):
    """Guard size per side and between two views for transforms of n points."""
    return min(max(2 * n * 8, MIN_GUARD), MAX_GUARD)


def _up(v, a=ALIGN):
    return -(-v // a) * a


def view_offsets(sizes, start_offset, guard):
    """Byte offsets of the views: the first at `start_offset`, each next one `guard` bytes (rounded up to 16) behind the
    end of the one before."""
    assert start_offset % ALIGN == 0 and start_offset >= guard and guard % ALIGN == 0 and guard > 0
    offs, off = [], start_offset
    for s in sizes:
        assert s > 0 and s % 4 == 0, "views hold whole 32-bit words"
        offs.append(off)
        off = _up(off + s + guard)
    return offs


def arena_bytes(sizes, start_offset, guard):
    """Smallest arena for this layout: the last view is followed by one more guard."""
    offs = view_offsets(sizes, start_offset, guard)
    return _up(offs[-1] + sizes[-1]) + guard


def guard_zones(sizes, offs, guard, total=None):
    """[lo, hi) of every guard zone.  total given: the zones tile everything of [0, total) that is not a view (every byte
    of the arena is a view byte or a checked guard byte).  total None: windows of `guard` bytes around the views only
    (the 4-GiB arena, whose far ends are not poisoned)."""
    ends = [o + s for o, s in zip(offs, sizes)]
    lo0 = 0 if total is not None else offs[0] - guard
    hi_last = total if total is not None else ends[-1] + guard
    zones = [(lo0, offs[0])]
    zones += [(ends[i], offs[i + 1]) for i in range(len(offs) - 1)]
    zones.append((ends[-1], hi_last))
    assert all(0 <= lo < hi for lo, hi in zones)
    return zones


def straddle_start(base_ptr, delta, guard):
    """Offset of a view inside an arena at `base_ptr` such that the byte `delta` bytes into the view has an address that is a
    multiple of 2^32, with room for a guard in front: the one solution in [guard, guard + 2^32)."""
    assert delta % ALIGN == 0 and base_ptr % ALIGN == 0 and delta >= 0
    start = (-(base_ptr + delta)) % FOUR_GIB
    if start < guard:
        start += FOUR_GIB
    assert (base_ptr + start + delta) % FOUR_GIB == 0 and start % ALIGN == 0 and guard <= start < guard + FOUR_GIB
    return start


def straddle_arena_bytes(sizes, guard):
    """An arena in which straddle_start fits whatever the base address: 4 GiB + guard in front of the views."""
    return FOUR_GIB + arena_bytes(sizes, guard, guard)


def signed_distance(off, sizes, offs):
    """(view index, d): position of arena byte `off` relative to the nearest view edge.  d >= 0: the byte lies d bytes
    past the END of that view (d = 0: the first byte behind it); d < 0: -d bytes in front of its START (d = -1: the last
    byte before it)."""
    best = None
    for i, (o, s) in enumerate(zip(offs, sizes)):
        assert not o <= off < o + s, "the byte lies inside a view"
        d = off - (o + s) if off >= o + s else off - o
        if best is None or abs(d) < abs(best[1]):
            best = (i, d)
    return best


def find_changes(read_words, zones, sizes, offs, names=None, limit=8, baits=()):
    """Compare every word of every guard zone with SENTINEL (with bait_words() from each arena offset in `baits` on).
    `read_words(lo, hi)` returns the uint32 words of arena bytes [lo, hi).  Returns at most `limit` reports (byte offset in the arena, view index, signed distance, message), first
    changed BYTE of each changed word, in address order."""
    names = names or ["view%d" % i for i in range(len(sizes))]
    out = []
    for lo, hi in zones:
        w = np.asarray(read_words(lo, hi), dtype=np.uint32)
        assert w.size * 4 == hi - lo
        want = np.full(w.size, SENTINEL, dtype=np.uint32)
        for b in baits:
            assert lo <= b and b + BAIT_BYTES <= hi or b + BAIT_BYTES <= lo or hi <= b, "a bait lies inside one guard zone"
            if lo <= b < hi:
                want[(b - lo) // 4:(b - lo + BAIT_BYTES) // 4] = bait_words()
        for k in np.flatnonzero(w != want)[:limit - len(out)]:
            x = int(w[k]) ^ int(want[k])
            byte = next(b for b in range(4) if (x >> (8 * b)) & 0xFF)     # little-endian: byte b of the word
            off = lo + 4 * int(k) + byte
            i, d = signed_distance(off, sizes, offs)
            where = ("%d bytes past the end of %s" % (d, names[i]) if d >= 0
                     else "%d bytes before the start of %s" % (-d, names[i]))
            out.append((off, i, d, "guard word changed %s (arena offset %d, word %#010x)" % (where, off, int(w[k]))))
        if len(out) >= limit:
            break
    return out


class GuardedArena:
    """One dev.create_buffer allocation, poisoned with SENTINEL, with views wrapped at `layout`'s offsets."""

    _poison_cache = None

    def __init__(self, dev, queue, nbytes, guard):
        self.dev, self.queue, self.guard, self.nbytes = dev, queue, guard, nbytes
        self.buf = dev.create_buffer(nbytes)
        self.device_ptr = self.buf.device_ptr
        assert self.device_ptr % ALIGN == 0
        self.views, self.sizes, self.offs, self.names, self.zones, self.baits = [], [], [], [], [], []

    @classmethod
    def _poison(cls, nbytes):
        if cls._poison_cache is None or cls._poison_cache.nbytes < nbytes:
            cls._poison_cache = np.full(_up(nbytes, 1 << 20) // 4, SENTINEL, dtype=np.uint32)
        return cls._poison_cache[:nbytes // 4]

    def layout(self, sizes, start_offset, names=None, whole=True):
        """Poison, then wrap one view per size.  whole=False: only the window guard | views | guard is poisoned and
        checked (the 4-GiB arena)."""
        self.sizes = list(sizes)
        self.offs = view_offsets(sizes, start_offset, self.guard)
        self.names = list(names) if names else ["view%d" % i for i in range(len(sizes))]
        self.zones = guard_zones(self.sizes, self.offs, self.guard, self.nbytes if whole else None)
        assert self.zones[-1][1] <= self.nbytes
        lo, hi = self.zones[0][0], self.zones[-1][1]
        self.queue.write_buffer(self.buf, lo, self._poison(hi - lo))
        self.views = [self.dev.wrap_buffer(self.device_ptr + o, s) for o, s in zip(self.offs, self.sizes)]
        self.baits = []
        return self.views

    def bait(self, i):
        """Read bait in the guard behind view i (module docstring)."""
        at = _up(self.offs[i] + self.sizes[i])
        assert self.guard >= 2 * BAIT_BYTES
        self.queue.write_buffer(self.buf, at, bait_words())
        self.baits.append(at)

    def check(self, limit=8):
        """Read back EVERY guard byte (waits for all submitted work) -> list of messages, empty when no guard word changed."""
        self.dev.poll()
        read = lambda lo, hi: self.buf.map_read(offset=lo, size=hi - lo, dtype=np.uint32)
        return [m for _, _, _, m in find_changes(read, self.zones, self.sizes, self.offs, self.names, limit, self.baits)]

    def destroy(self):
        for v in self.views:
            v.destroy()
        self.views = []
        self.buf.destroy()
