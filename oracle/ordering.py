"""Host-side ordering of fwa_plan_exec / fwa_plan_destroy (TEST INFRASTRUCTURE ONLY): the scenarios.

The kernels are held by the parity, containment and error-budget tests.  What stitches them together on the host is
held here: the fork from the caller's stream to the context's chain streams and the join back (plan.cpp run_groups),
the chain streams shared by every plan of a context, the pooled ring and the wait in fwa_plan_destroy, and the promise
that an exec only enqueues, so that a caller can capture it into a graph.  A missing edge there gives wrong spectra,
not an error code.

SCENARIOS is a list of (id, callable); `callable(fw, dev, queue, oracle)` returns a list of failure messages, empty =
pass.  tests/test_gpu_ordering.py runs every one on the product library; tools/ordering_mutants.py runs the same code
on laboratory builds that each lack one ordering edge.

Reference of every comparison: the bits of a *solo* exec -- fresh buffers, a plan of the same geometry, input uploaded
with a host wait, one exec, a device-wide host wait -- which is itself checked against oracle.dft_f64 at REL_TOL on its
first, last and group-boundary transforms.  GPU results are bit-deterministic for a fixed input (error_budget.py), so
every comparison with a solo exec is bit-identity; no new tolerance.  A solo exec waits on the host on both sides, so
it is right also on a build that lacks a device-side edge.

Every plan is held to the geometry its tag names (path, factors, launches_per_exec, group, streams): a shape that
quietly took one chain raises GeometryDrift; it never passes vacuously.

Shapes: the smallest that reach each mechanism (tag -> SHAPES).  Even log2 n wherever a plan is destroyed before its
result is read: the result buffer is then the caller's src.
"""
import ctypes

import numpy as np

from .device_run import hip_runtime, parity_failures, upload
from .error_budget import _f

REL_TOL = 1e-5            # the parity bound of the suite (tests/conftest.py REL_TOL; tests/test_ordering.py compares them)
POISON = 0x7FC0DEAD       # a quiet NaN as f32: a destination nobody wrote stays recognisable
DIRECTION = {"Forward": -1, "Inverse": 1, "Onlyinverse": 1, "Onlyinverse+Normalize": 1}

# tag -> n, batch, keys set before the first exec, and what the plan must then report
SHAPES = {
    # 2^20 two-pass pipeline: the smallest batch it accepts with both chains busy; 3 groups on 2 chains, last one ragged
    "P1": dict(n=1 << 20, batch=5, tunables={"group": 2, "streams": 2},
               want=dict(path=1, factors=_f(10, 10), launches_per_exec=6, group=2, streams=2)),
    # the smallest tiled size, two passes, 4 groups on 2 chains
    "T2": dict(n=1 << 16, batch=7, tunables={"group": 2, "streams": 2},
               want=dict(path=7, factors=_f(8, 8), launches_per_exec=8, group=2, streams=2)),
    # three passes: pass B runs in place in the slab between fork and join
    "T3": dict(n=1 << 18, batch=5, tunables={"factors": _f(6, 6, 6), "group": 2, "streams": 2},
               want=dict(path=7, factors=_f(6, 6, 6), launches_per_exec=9, group=2, streams=2)),
    # defaults with ONE chain: the groups run on the caller's stream, the ring is 128 MiB
    "S1": dict(n=1 << 20, batch=48, tunables={},
               want=dict(path=1, factors=_f(10, 10), launches_per_exec=6, group=16, streams=1)),
    "S2": dict(n=1 << 16, batch=512, tunables={},
               want=dict(path=7, factors=_f(8, 8), launches_per_exec=4, group=256, streams=1)),
    # the default two-chain geometry of a tiled plan: 4 groups without any key
    "D2": dict(n=1 << 22, batch=13, tunables={},
               want=dict(path=7, factors=_f(10, 12), launches_per_exec=8, group=4, streams=2)),
    # one launch, no pipeline (the reference's own benchmark shape); result in the plan's second buffer (odd log2 n)
    "Z0": dict(n=512, batch=2500, tunables={}, want=dict(path=0, factors=9, launches_per_exec=1)),
}
MECHANISM_TAGS = ("P1", "T2", "T3", "S1", "S2", "D2")


class GeometryDrift(AssertionError):
    pass


# ---- shared helpers -------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def gen(oracle, tag, k):
    """Input number k of a shape: disjoint runs of the seeded generator."""
    s = SHAPES[tag]
    return oracle.gen_input(s["n"], s["batch"], first_transform=1000 * k + s["n"] % 89)


def make_plan(fw, dev, queue, tag, kind, src, src2=None, tunables=None, want=None):
    """A plan of the shape `tag` with its keys set, held to the geometry the tag names."""
    s = SHAPES[tag]
    tunables = s["tunables"] if tunables is None else tunables
    want = s["want"] if want is None else want
    plan = fw.plan_of_kind(kind, dev, queue, src, src2, s["n"])
    try:
        plan.configure(tunables)
        took = {k: int(plan.get(k)) for k in want}
        if took != want:
            raise GeometryDrift("%s/%s: the plan took %s, the scenario names %s" % (tag, kind, took, want))
    except Exception:
        plan.destroy()
        raise
    return plan


def expected(oracle, tag, kind, x, transforms):
    """fp64 DFT of the listed transforms of x, scaled as `kind` scales."""
    n = SHAPES[tag]["n"]
    transforms = list(transforms)
    scale = 1.0 / n if kind in ("Inverse", "Onlyinverse+Normalize") else 1.0
    if len(transforms) == x.size // n:     # the whole batch: one threaded call
        r = oracle.dft_f64(x, n, DIRECTION[kind]) * scale
        return {t: r[t * n:(t + 1) * n] for t in transforms}
    return {t: oracle.dft_f64(x[t * n:(t + 1) * n], n, DIRECTION[kind]) * scale for t in transforms}


def dft_failures(oracle, tag, kind, x, y, transforms, what):
    n = SHAPES[tag]["n"]
    bad = []
    for t, r in expected(oracle, tag, kind, x, transforms).items():
        for _, mx, l2 in parity_failures(y[t * n:(t + 1) * n], r, n, REL_TOL)[0]:
            bad.append("%s: transform %d against the fp64 DFT: max_rel %.3g rel_l2 %.3g (bound %g)" % (what, t, mx, l2, REL_TOL))
    return bad


def _edge_transforms(tag):
    s = SHAPES[tag]
    g = s["want"].get("group", s["batch"])
    return sorted({0, min(g, s["batch"] - 1), max(0, min(g, s["batch"]) - 1), s["batch"] - 1})


_SOLO = {}


def solo(fw, dev, queue, oracle, tag, kind, k, x=None, steps=1):
    """The bits of `steps` solo execs of input k (each exec followed by a device-wide host wait; for even log2 n exec
    i + 1 transforms the output of exec i) -> list of read-only complex64 arrays, one per step.  Computed once per
    (device, shape, kind, input) and shared.  kind "Onlyinverse+Normalize": the two plans of the reference's
    basic_inverse2 sequence, one step."""
    key = (id(dev), tag, kind, k, steps)
    if key in _SOLO:
        return _SOLO[key]
    x = gen(oracle, tag, k) if x is None else x
    src = upload(dev, queue, x)
    src2 = dev.create_buffer(x.nbytes) if kind.startswith("Onlyinverse") else None
    plan = make_plan(fw, dev, queue, tag, kind.split("+")[0], src, src2)
    norm = fw.Normalize(dev, queue, src, src2, SHAPES[tag]["n"]) if kind.endswith("+Normalize") else None
    enc = dev.create_command_encoder()
    outs = []
    for _ in range(steps):
        out = plan.proc(enc)
        if norm is not None:
            out = norm.proc(enc)
        dev.poll()
        y = out.map_read()
        y.setflags(write=False)
        outs.append(y)
    bad = dft_failures(oracle, tag, kind, x, outs[0], _edge_transforms(tag), "solo %s/%s" % (tag, kind))
    for p in (norm, plan):
        if p is not None:
            p.destroy()
    enc.destroy()
    for b in (src, src2):
        if b is not None:
            b.destroy()
    assert not bad, "\n".join(bad)     # the reference itself is wrong: nothing below means anything
    if steps * x.nbytes <= 512 << 20:  # the large multi-step sequences are used once
        _SOLO[key] = outs
    return outs


class Pinned:
    """Page-locked staging for truly asynchronous, stream-ordered uploads (dev.pinned_array), freed on exit."""

    def __init__(self, dev):
        self.dev = dev

    def __enter__(self):
        self.mark = len(getattr(self.dev, "_pinned", []))
        return self

    def array(self, x):
        a = self.dev.pinned_array(x.size, dtype=x.dtype)
        a[:] = x
        return a

    def poison(self, nbytes):
        a = self.dev.pinned_array(nbytes // 4, dtype=np.uint32)
        a[:] = POISON
        return a

    def __exit__(self, *exc):
        self.dev.poll()
        while len(getattr(self.dev, "_pinned", [])) > self.mark:
            self.dev._L.fwa_host_free(self.dev._h, self.dev._pinned.pop())


def hip_stream(hip):
    s = ctypes.c_void_p()
    rc = hip.hipStreamCreateWithFlags(ctypes.byref(s), 1)      # hipStreamNonBlocking
    assert rc == 0 and s.value, "hipStreamCreateWithFlags: %d" % rc
    return s


def kernel_nodes(hip, graph):
    count = ctypes.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * max(1, count.value))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(count)) == 0
    kernels = 0
    for i in range(count.value):
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(nodes[i], ctypes.byref(kind)) == 0
        kernels += kind.value == 0                                # hipGraphNodeTypeKernel
    return kernels, count.value


# ---- graph capture of an exec that forks to the chain streams and joins back ---------------------------------------------
def graph_forked(tag, kind):
    def scenario(fw, dev, queue, oracle):
        hip = hip_runtime()
        if hip is None:
            return ["no libamdhip64 mapped in this process"]
        bad = []
        s = SHAPES[tag]
        xs = [gen(oracle, tag, k) for k in (0, 1)]
        want = [solo(fw, dev, queue, oracle, tag, kind, k, x)[0] for k, x in zip((0, 1), xs)]
        nbytes = xs[0].nbytes
        src = upload(dev, queue, xs[0])
        two = kind == "Onlyinverse+Normalize"
        src2 = dev.create_buffer(nbytes) if two else None
        plans = [make_plan(fw, dev, queue, tag, kind.split("+")[0], src, src2)]
        if two:
            plans.append(fw.Normalize(dev, queue, src, src2, s["n"]))
        launches = sum(int(p.get("launches_per_exec")) for p in plans)
        stream = hip_stream(hip)
        enc = dev.create_command_encoder(hip_stream=stream)
        graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
        with Pinned(dev) as pin:
            staged = [pin.array(x) for x in xs]
            poison = pin.poison(nbytes) if two else None
            # first use outside the capture: the chain streams are created (and checked to overlap) here, never while a
            # stream captures
            for p in plans:
                out = p.proc(enc)
            enc.synchronize()
            chains = dev.stats()["chain_streams"]
            if int(plans[0].get("streams")) != 2 or chains < 2:
                bad.append("the plan does not fork: streams %d, chain streams of the context %d" % (plans[0].get("streams"), chains))
            queue.write_buffer(src, 0, staged[0], encoder=enc)
            if two:
                queue.write_buffer(src2, 0, poison, encoder=enc)
            enc.synchronize()
            rc = hip.hipStreamBeginCapture(stream, 0)             # hipStreamCaptureModeGlobal
            assert rc == 0, "hipStreamBeginCapture: %d" % rc
            try:
                for p in plans:
                    out = p.proc(enc)
            finally:
                rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
            assert rc == 0 and graph.value, "hipStreamEndCapture: %d (a chain stream was not joined back?)" % rc
            # (a) a captured exec enqueued nothing real
            enc.synchronize()
            if not same_bits(src.map_read(stream=enc), xs[0]):
                bad.append("(a) the source changed during the capture: the captured exec ran something")
            if two and not np.all(bits(src2.map_read(stream=enc)) == POISON):
                bad.append("(a) the result buffer lost its poison during the capture")
            # (b) one kernel node per launch the plans report
            kernels, nodes = kernel_nodes(hip, graph)
            if kernels != launches:
                bad.append("(b) the graph holds %d kernel nodes (of %d nodes), the plans report %d launches per exec" % (kernels, nodes, launches))
            rc = hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0)
            assert rc == 0, "hipGraphInstantiate: %d" % rc
            # (c) two replays on two different inputs
            for k in (0, 1):
                queue.write_buffer(src, 0, staged[k], encoder=enc)
                if two:
                    queue.write_buffer(src2, 0, poison, encoder=enc)
                rc = hip.hipGraphLaunch(gexec, stream)
                assert rc == 0, "hipGraphLaunch: %d" % rc
                if not same_bits(out.map_read(stream=enc), want[k]):
                    bad.append("(c) replay %d differs from a solo exec of its input" % k)
            rc = (hip.hipGraphExecDestroy(gexec), hip.hipGraphDestroy(graph))
            assert rc == (0, 0), "hipGraphExecDestroy / hipGraphDestroy: %s" % (rc,)
            # (d) the plan outlived the graph
            queue.write_buffer(src, 0, staged[1], encoder=enc)
            for p in plans:
                out = p.proc(enc)
            if not same_bits(out.map_read(stream=enc), want[1]):
                bad.append("(d) a direct exec after hipGraphExecDestroy differs from a solo exec")
        for p in reversed(plans):
            p.destroy()
        enc.destroy()
        assert hip.hipStreamDestroy(stream) == 0
        for b in (src, src2):
            if b is not None:
                b.destroy()
        return bad
    return scenario


# ---- two (three) plans of one context, each on its own caller stream -------------------------------------------------------
def two_plans_two_streams(tags):
    rounds = 3

    def scenario(fw, dev, queue, oracle):
        bad = []
        want = [solo(fw, dev, queue, oracle, tag, "Forward", 2 + i, steps=rounds) for i, tag in enumerate(tags)]
        srcs = [upload(dev, queue, gen(oracle, tag, 2 + i)) for i, tag in enumerate(tags)]
        plans = [make_plan(fw, dev, queue, tag, "Forward", src) for tag, src in zip(tags, srcs)]
        encs = [dev.create_command_encoder() for _ in tags]
        keep = [[dev.create_buffer(src.size) for _ in range(rounds)] for src in srcs]
        dev.poll()
        for r in range(rounds):                       # nothing in here waits on the host
            for p, enc, src, k in zip(plans, encs, srcs, keep):
                out = p.proc(enc)
                enc.copy_buffer_to_buffer(out, 0, k[r], 0, src.size)
        for enc in encs:
            enc.synchronize()
        for tag, k, w in zip(tags, keep, want):
            for r in range(rounds):
                if not same_bits(k[r].map_read(), w[r]):
                    bad.append("%s, round %d: differs from the same sequence of this plan run alone" % (tag, r))
        for p in plans:
            p.destroy()
        for o in encs + srcs + [b for k in keep for b in k]:
            o.destroy()
        return bad
    return scenario


# ---- fwa_plan_destroy while the plan's last exec is in flight, its ring handed to the next plan -----------------------------
def destroy_in_flight(tag, variant):
    """Plan A's exec is queued on stream 1 behind the stream-ordered upload of its own input (milliseconds over the host
    link), and stream 2 waits on the device for the end of that upload: whatever the host does in between, A's exec and B's
    exec become runnable at the same moment.  If fwa_plan_destroy(A) returned before A's exec had finished, the two would
    run side by side on the one ring B took over from A."""
    def scenario(fw, dev, queue, oracle):
        bad = []
        xa, xb = gen(oracle, tag, 5), gen(oracle, tag, 6)
        want_a = solo(fw, dev, queue, oracle, tag, "Forward", 5, xa)[0]
        want_b = solo(fw, dev, queue, oracle, tag, "Forward", 6, xb)[0]
        src_a, src_b = dev.create_buffer(xa.nbytes), upload(dev, queue, xb)
        hip = stream = None
        if variant == "wrapped":
            hip = hip_runtime()
            if hip is None:
                return ["no libamdhip64 mapped in this process"]
            stream = hip_stream(hip)
            enc1 = dev.create_command_encoder(hip_stream=stream)
        else:
            enc1 = dev._default if variant == "null" else dev.create_command_encoder()
        enc2 = dev.create_command_encoder()
        uploaded = fw.Event(dev)
        a = make_plan(fw, dev, queue, tag, "Forward", src_a)
        with Pinned(dev) as pin:
            staged = pin.array(xa)
            dev.poll()
            before = (dev.get("ring_reuses"), dev.get("ring_allocs"))
            # from here to the last exec nothing waits on the host except fwa_plan_destroy itself (and, in the variant
            # "destroyed", whatever fwa_stream_destroy waits for)
            queue.write_buffer(src_a, 0, staged, encoder=enc1)
            uploaded.record(enc1)
            enc2.wait_event(uploaded)
            a.proc(enc1)
            if variant == "destroyed":
                enc1.destroy()
            a.destroy()
            b = make_plan(fw, dev, queue, tag, "Forward", src_b)
            b.proc(enc2)
            after = (dev.get("ring_reuses"), dev.get("ring_allocs"))
            dev.poll()
        if after != (before[0] + 1, before[1]):
            bad.append("plan B did not take plan A's pooled ring: (ring_reuses, ring_allocs) %s -> %s" % (before, after))
        if not same_bits(src_a.map_read(), want_a):
            bad.append("plan A (destroyed with its exec in flight) differs from a solo exec")
        if not same_bits(src_b.map_read(), want_b):
            bad.append("plan B (on the ring plan A gave back) differs from a solo exec")
        b.destroy()
        del uploaded
        for o in (enc1, enc2, src_a, src_b):
            if o is not dev._default:
                o.destroy()
        if stream is not None:
            assert hip.hipStreamDestroy(stream) == 0
        return bad
    return scenario


# ---- one plan, execs on alternating caller streams ordered only on the device -----------------------------------------------
def alternating_streams(tag):
    execs = 4

    def scenario(fw, dev, queue, oracle):
        bad = []
        xs = [gen(oracle, tag, 10 + i) for i in range(execs)]
        want = [solo(fw, dev, queue, oracle, tag, "Forward", 10 + i, x)[0] for i, x in enumerate(xs)]
        nbytes = xs[0].nbytes
        src = dev.create_buffer(nbytes)
        plan = make_plan(fw, dev, queue, tag, "Forward", src)
        encs = [dev.create_command_encoder(), dev.create_command_encoder()]
        keep = [dev.create_buffer(nbytes) for _ in xs]
        with Pinned(dev) as pin:
            staged = [pin.array(x) for x in xs]
            dev.poll()
            for i in range(execs):                    # nothing in here waits on the host
                enc, other = encs[i % 2], encs[(i + 1) % 2]
                enc.wait_for(other)
                queue.write_buffer(src, 0, staged[i], encoder=enc)
                out = plan.proc(enc)
                enc.copy_buffer_to_buffer(out, 0, keep[i], 0, nbytes)
            for enc in encs:
                enc.synchronize()
        for i in range(execs):
            if not same_bits(keep[i].map_read(), want[i]):
                bad.append("exec %d (encoder %d) differs from a solo exec of its input" % (i, i % 2))
        plan.destroy()
        for o in encs + keep + [src]:
            o.destroy()
        return bad
    return scenario


# ---- HostPipeline over a pipelined plan: one plan per slot, back to back on one stream ---------------------------------------
def host_pipeline(tag):
    iters, slots = 5, 2

    def scenario(fw, dev, queue, oracle):
        bad = []
        s = SHAPES[tag]
        xs = [gen(oracle, tag, 20 + i) for i in range(iters)]
        want3 = solo(fw, dev, queue, oracle, tag, "Forward", 23, xs[3])[0]
        mark = len(getattr(dev, "_pinned", []))
        pipe = fw.HostPipeline(dev, queue, lambda d, q, b: make_plan(fw, d, q, tag, "Forward", b), s["n"] * s["batch"], slots=slots)
        results, pending = {}, []
        for it in range(iters):
            pending.append((it, pipe.submit(xs[it])))
            if len(pending) == slots:                 # read a slot back before it is reused
                j, sj = pending.pop(0)
                results[j] = pipe.result(sj).copy()
        for j, sj in pending:
            results[j] = pipe.result(sj).copy()
        pipe.drain()
        for it in range(iters):
            bad += dft_failures(oracle, tag, "Forward", xs[it], results[it], range(s["batch"]), "iteration %d" % it)
        if not same_bits(results[3], want3):
            bad.append("iteration 3 differs from a solo exec of its input")
        for p in pipe.plans:
            p.destroy()
        for o in [pipe.ex, pipe.down] + pipe.src + pipe.staging:
            o.destroy()
        del pipe
        dev.poll()
        while len(dev._pinned) > mark:
            dev._L.fwa_host_free(dev._h, dev._pinned.pop())
        return bad
    return scenario


# ---- the default two-chain geometry of a tiled plan ---------------------------------------------------------------------------
def default_two_chains(tag):
    def scenario(fw, dev, queue, oracle):
        s = SHAPES[tag]
        x = gen(oracle, tag, 30)
        outs = []
        # no key set: 4 groups of 4 on two chains; then the same plan as 7 groups of 2 on the caller's stream
        for tunables, want in (({}, s["want"]),
                               ({"group": 2, "streams": 1}, dict(s["want"], group=2, streams=1, launches_per_exec=14))):
            src = upload(dev, queue, x)
            keep = dev.create_buffer(x.nbytes)
            plan = make_plan(fw, dev, queue, tag, "Forward", src, tunables=tunables, want=want)
            enc = dev.create_command_encoder()
            out = plan.proc(enc)
            enc.copy_buffer_to_buffer(out, 0, keep, 0, x.nbytes)
            outs.append(keep.map_read(stream=enc))    # waits for the caller's stream only: the join is what orders it
            plan.destroy()
            for o in (enc, src, keep):
                o.destroy()
        bad = dft_failures(oracle, tag, "Forward", x, outs[0], (0, 3, 4, 12), "default geometry")
        if not same_bits(outs[0], outs[1]):
            bad.append("the default two-chain plan differs from the same plan with group = 2 on one chain")
        return bad
    return scenario


SCENARIOS = (
    [("graph_forked/%s/%s" % (t, k), graph_forked(t, k)) for t in ("P1", "T2", "T3") for k in ("Forward", "Inverse")]
    + [("graph_forked/T2/Onlyinverse+Normalize", graph_forked("T2", "Onlyinverse+Normalize"))]
    + [("two_plans_two_streams/%s" % "+".join(t).replace("Z0", "path0"), two_plans_two_streams(t))
       for t in (("S1", "S2"), ("P1", "T2"), ("P1", "T2", "Z0"))]
    + [("destroy_in_flight/%s/%s" % (t, v), destroy_in_flight(t, v))
       for t in ("S1", "S2") for v in ("library", "null", "wrapped", "destroyed")]
    + [("alternating_streams/%s" % t, alternating_streams(t)) for t in ("P1", "T2")]
    + [("host_pipeline/%s" % t, host_pipeline(t)) for t in ("T2", "P1")]
    + [("default_two_chains/D2", default_two_chains("D2"))]
)
