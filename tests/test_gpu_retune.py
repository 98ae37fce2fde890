"""Re-tuning a pipelined plan before its first exec: what the plan and its context report after every step follows from a
few rules (the model below), and a re-tuned plan computes what a fresh plan of the same final choice computes.

The shape is the smallest with a ring: n = 2^16 (tiled path), 9 transforms (4.5 MiB).  Every test makes a context of
its own, so the ring pool starts empty and the counters start at zero.
"""
import numpy as np
import pytest

from conftest import REL_TOL
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu

LG, N, BATCH = 16, 1 << 16, 9
POOL_CAP = 1 << 30


@pytest.fixture(scope="module")
def fw():
    import fft_wgpu_amd as fw
    return fw


@pytest.fixture(scope="module")
def signal(oracle):
    x = oracle.gen_input(N, BATCH, first_transform=5)
    x.setflags(write=False)
    r = oracle.dft_f64(x, N, -1)
    r.setflags(write=False)
    return x, r


def _own_context(fw):
    return open_gpu()[1:]


def _second_factorisation(plan):
    """a valid factorisation of 2^16 other than the plan's own"""
    return next(f for f in (8 | (8 << 8), 10 | (6 << 8)) if f != plan.get("factors"))


class Model:
    """The rules a re-tune follows: ring bytes = min(group, batch) x min(streams, groups) x n x 8; a build first takes the
    newest pooled ring of exactly that size, else allocates, then pools the old ring; the pool keeps at most 1 GiB (oldest
    entries go first); "factors" restores the default group (128 MiB of transforms) and chains (2 from 4 groups on, else
    1); "path" = 2 pools the ring and, on even log2 n, adds a second buffer of the source's size."""

    def __init__(self, factors):
        self.pool, self.allocs, self.reuses = [], 0, 0     # pool: ring sizes, oldest first
        self.ring, self.second, self.path, self.factors = 0, 0, 7, factors
        self.set_factors(factors)

    def _to_pool(self, size):
        if not size:
            return
        if size > POOL_CAP:
            return
        self.pool.append(size)
        while sum(self.pool) > POOL_CAP:
            self.pool.pop(0)

    def build(self, group, streams):
        self.group = min(max(group, 1), BATCH)
        groups = -(-BATCH // self.group)
        self.streams = min(max(streams, 1), groups)
        new = self.group * self.streams * N * 8
        if new in self.pool:
            self.pool.reverse(); self.pool.remove(new); self.pool.reverse()   # the newest of that size
            self.reuses += 1
        else:
            self.allocs += 1
        self._to_pool(self.ring)
        self.ring = new

    def set_factors(self, factors):
        group = max((128 << 20) // (N * 8), 1)
        self.factors, self.path = factors, 7
        self.build(group, 2 if -(-BATCH // group) >= 4 else 1)

    def set_path_2(self):
        self._to_pool(self.ring)
        self.ring, self.path = 0, 2
        if LG % 2 == 0:
            self.second = N * BATCH * 8

    def expected(self):
        passes = 3 if self.factors >> 16 else 2
        launches = LG if self.path == 2 else passes * -(-BATCH // self.group)
        return {"scratch_bytes": self.ring + self.second, "group": self.group, "streams": self.streams,
                "launches_per_exec": launches, "factors": self.factors, "path": self.path,
                "ring_allocs": self.allocs, "ring_reuses": self.reuses, "pooled_ring_bytes": sum(self.pool)}


def _observed(plan, dev):
    got = {k: plan.get(k) for k in ("scratch_bytes", "group", "streams", "launches_per_exec", "factors", "path")}
    stats = dev.stats()
    got.update({k: stats[k] for k in ("ring_allocs", "ring_reuses", "pooled_ring_bytes")})
    return got


def test_retune_ledger_follows_the_rules(fw):
    """group = 2, streams = 2, group = 2 again, a second factorisation, path = 2: after every step the plan's scratch,
    geometry, launches, factors and path and the context's ring counters are what the rules give; destroying the plan
    pools its last ring."""
    dev, queue = _own_context(fw)
    src = dev.create_buffer(N * BATCH * 8)
    plan = fw.Forward(dev, queue, src, N)
    model = Model(plan.get("factors"))
    other = _second_factorisation(plan)
    steps = [("create", None, lambda: None),
             ("group", 2, lambda: model.build(2, model.streams)),
             ("streams", 2, lambda: model.build(model.group, 2)),
             ("group", 2, lambda: model.build(2, model.streams)),
             ("factors", other, lambda: model.set_factors(other)),
             ("path", 2, model.set_path_2)]
    for i, (key, value, rule) in enumerate(steps):
        if value is not None:
            plan.set(key, value)
        rule()
        got, want = _observed(plan, dev), model.expected()
        print(i, key, value, got)
        assert got == want, (i, key, value, got, want)
    assert model.allocs > 1 and model.reuses > 0        # the sequence reaches both branches of the build order
    pooled, last_ring = dev.stats()["pooled_ring_bytes"], model.ring
    plan.destroy()
    assert dev.stats()["pooled_ring_bytes"] == pooled + last_ring
    src.destroy()
    dev.destroy()


def test_retuned_plan_computes_what_a_fresh_plan_does(fw, oracle, signal):
    """A plan re-tuned through group = 2, streams = 2, group = 2, factors = F and a fresh plan with only factors = F: the
    same bits, both within REL_TOL of the fp64 DFT; the re-tuned plan's ring goes to the pool when it is destroyed."""
    x, r = signal
    dev, queue = _own_context(fw)
    enc = dev.create_command_encoder()
    outs, plans, bufs, f = [], [], [], None
    for steps in ((("group", 2), ("streams", 2), ("group", 2)), ()):
        src = dev.create_buffer(x.nbytes)
        queue.write_buffer(src, 0, x)
        plan = fw.Forward(dev, queue, src, N)
        f = f or _second_factorisation(plan)
        for key, value in steps + (("factors", f),):
            plan.set(key, value)
        outs.append(plan.proc(enc).map_read(stream=enc))
        plans.append(plan)
        bufs.append(src)
    assert all(p.get(k) == plans[1].get(k) for p in plans for k in ("factors", "group", "streams", "scratch_bytes"))
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    for y in outs:
        for t in range(BATCH):
            mx, l2 = oracle.compare(y[t * N:(t + 1) * N], r[t * N:(t + 1) * N])
            assert mx <= REL_TOL and l2 <= REL_TOL, (t, mx, l2)
    pooled, ring = dev.stats()["pooled_ring_bytes"], plans[0].get("scratch_bytes")
    assert ring == BATCH * N * 8
    plans[0].destroy()
    assert dev.stats()["pooled_ring_bytes"] == pooled + ring
    plans[1].destroy()
    for b in bufs + [enc]:
        b.destroy()
    dev.destroy()
