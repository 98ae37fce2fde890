"""GPU tests of the multi-GPU part of the boundary, on however many devices the box shows --
one on this pool, so the N-device forms run in their degenerate shapes: `ShardedBatch` over `device_count()` devices, and
several contexts on device 0 acting as the shards of one batch, with the slab-movement legs (peer-copy `fwa_buf_copy`
across contexts; `fwa_comm_*` over RCCL in a fresh child process).  Everything must be BIT-identical to the unsharded
transform of the same samples: sharding only chooses where a transform runs.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle.device_run import open_gpu
from parity_cases import hip_runtime, run as _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


def test_enumerate_adapters_lists_every_ordinal(gpu):
    """instance.enumerate_adapters (src/lib.rs:33-35): one entry per fwa_device_count ordinal, no context needed."""
    fw, dev, _ = gpu
    ads = fw.enumerate_adapters()
    assert len(ads) == fw.device_count() >= 1
    assert [a["ordinal"] for a in ads] == list(range(len(ads)))
    for a in ads:
        assert a["usable"] and a["name"].startswith("gfx950") and a["compute_units"] == 256 and a["hbm_bytes"] > (200 << 30)
    assert ads[0]["name"] == dev.info()["name"]
    ok = ctypes.c_int32()
    assert dev._L.fwa_device_info(len(ads), None, 0, None, None, ctypes.byref(ok)) == 1      # ordinal out of range


@pytest.mark.parametrize("kind,n,batch", [("Forward", 1024, 37), ("Forward", 512, 5), ("Inverse", 1 << 16, 9), ("Forward", 1 << 20, 9),
                                          ("Onlyinverse", 2048, 11)])
def test_sharded_batch_over_visible_devices_is_bit_identical(gpu, oracle, kind, n, batch):
    """`ShardedBatch` with its default ordinals = every visible device (one here): slabs tile the batch, results equal
    the plain plan bit for bit, odd log2 n (result in the plan's second buffer) included."""
    fw, dev, queue = gpu
    x = oracle.gen_input(n, batch, first_transform=3)
    ref, _, _ = _run(fw, dev, queue, kind, x, n)
    sb = fw.ShardedBatch(getattr(fw, kind), n, batch)
    assert len(sb) == fw.device_count() and sb.slabs[0][0] == 0 and sb.slabs[-1][1] == batch
    sb.write(x)
    sb.proc()
    y = sb.read()
    assert np.array_equal(y.view(np.uint64), ref.view(np.uint64))
    sb.destroy()


@pytest.mark.parametrize("n,batch,shards", [(1024, 37, 2), (512, 7, 3), (1 << 20, 9, 2), (1 << 16, 2, 3), (4096, 0, 2)])
def test_contexts_on_device_0_as_shards_of_one_batch_with_scatter_and_gather(gpu, oracle, n, batch, shards):
    """Several contexts on device 0 stand in for the GPUs of a node: the batch starts in one buffer of the first context,
    is scattered slab by slab into the shards' buffers (fwa_buf_copy ACROSS contexts), transformed by every shard on its own
    stream, and gathered into one buffer again -- bit-identical to the unsharded transform; ragged slabs, a shard with
    no transform at all (batch 2 over 3 shards), the empty batch, the 2^20 pipeline (each shard forks to its context's chains)."""
    fw, dev, queue = gpu
    x = oracle.gen_input(n, batch, first_transform=11)
    ref = _run(fw, dev, queue, "Forward", x, n)[0] if batch else x
    sb = fw.ShardedBatch(fw.Forward, n, batch, ordinals=[0] * shards)
    assert [b - a for a, b in sb.slabs] == [batch // shards + (1 if r < batch % shards else 0) for r in range(shards)]
    for other in sb.devices[1:]:
        assert sb.devices[0].peer_access(other) == 1                    # same device
    root = sb.devices[0]
    full = root.create_buffer(x.nbytes)
    back = root.create_buffer(x.nbytes)
    if batch:
        fw.Queue(root).write_buffer(full, 0, x, encoder=sb.encoders[0])
    sb.scatter(full)
    res = sb.proc()
    assert all((r.device_ptr == b.device_ptr) == (int(np.log2(n)) % 2 == 0) for r, b, (a, z) in zip(res, sb.buffers, sb.slabs) if z > a)
    sb.gather(back)
    y = back.map_read(stream=sb.encoders[0]) if batch else x
    assert np.array_equal(y.view(np.uint64), ref.view(np.uint64))
    # and straight from / to host memory
    sb.write(x)
    sb.proc()
    assert np.array_equal(sb.read().view(np.uint64), ref.view(np.uint64))
    # both enqueue forms of proc(): one host thread per shard (what a process driving 8 GPUs needs: VERDICT round 4, item 2;
    # profiles/round5/enqueue_cost.jsonl) and one shard after another
    for threads in (True, False):
        sb.threads = threads
        assert sb._threaded() == (threads and shards > 1)
        sb.write(x)
        sb.proc()
        assert np.array_equal(sb.read().view(np.uint64), ref.view(np.uint64))
    sb.destroy()
    assert all(d._h is None for d in sb.devices)     # the contexts this object created are gone
    full.destroy()                                    # handles may outlive their context
    back.destroy()


def test_sharded_batch_leaves_the_callers_devices_alone(gpu, oracle):
    """`devices=`: the caller's Device objects are used as they are and survive destroy(); an exec of many launches is
    enqueued from one thread per shard by default."""
    fw, dev, queue = gpu
    n, batch = 1 << 20, 2 * 160
    mine = [fw.Device(0), fw.Device(0)]
    sb = fw.ShardedBatch(fw.Forward, n, batch, devices=mine)
    assert sb.devices == mine and sb.plans[0].get("launches_per_exec") == 20 and sb._threaded()
    for d, b, e, (a, z) in zip(sb.devices, sb.buffers, sb.encoders, sb.slabs):
        d.fill_synthetic(b, n, first_transform=a, encoder=e)
    res = sb.proc()
    sb.poll()
    x = oracle.gen_input(n, 1, first_transform=161)       # one transform of the second shard, checked against the fp64 DFT
    y = res[1].map_read(offset=n * 8, size=n * 8, stream=sb.encoders[1])
    mx, l2 = oracle.compare(y, oracle.dft_f64(x, n, -1))
    assert mx <= 1e-5 and l2 <= 1e-5, (mx, l2)
    sb.destroy()
    assert all(d._h is not None for d in mine)
    assert mine[0].create_buffer(1024).size == 1024      # still usable
    for d in mine:
        d.destroy()


def test_buf_copy_across_contexts_is_explicit(gpu, oracle):
    """fwa_buf_copy between buffers of two contexts: the stream must belong to one of them; same device = plain device copy."""
    fw, dev, queue = gpu
    a, b, c = fw.Device(0), fw.Device(0), fw.Device(0)
    x = oracle.gen_input(256, 4)
    ba, bb = a.create_buffer(x.nbytes), b.create_buffer(x.nbytes)
    ea, eb, ec = a.create_command_encoder(), b.create_command_encoder(), c.create_command_encoder()
    fw.Queue(a).write_buffer(ba, 0, x, encoder=ea)
    ea.synchronize()
    L = a._L
    assert L.fwa_buf_copy(bb._h, 0, ba._h, 0, x.nbytes, ec._h) == 1                          # a third context's stream
    assert b"neither" in L.fwa_last_error_string(b._h)
    assert L.fwa_buf_copy(bb._h, 0, ba._h, 0, x.nbytes, eb._h) == 0                          # dst's stream
    assert np.array_equal(bb.map_read(stream=eb).view(np.uint64), x.view(np.uint64))
    assert L.fwa_buf_copy(bb._h, 8, ba._h, 0, x.nbytes, ea._h) == 1                          # range check
    k = ctypes.c_int32(-1)
    assert L.fwa_ctx_peer_access(a._h, b._h, ctypes.byref(k)) == 0 and k.value == 1


def _build(tmp_path, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", name + ".cpp"),
                           "-L" + os.path.join(ROOT, "fft_wgpu_amd"), "-lfft_wgpu_amd", "-pthread", "-o", str(exe)])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "fft_wgpu_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    return str(exe), env


def test_cpp_sharded_batch_is_bit_identical_to_the_unsharded_transform(gpu, tmp_path):
    """fft_wgpu::ShardedBatch (include/fft_wgpu.hpp) from a compiled C++ host (tools/example_sharded.cpp): enumerate_devices,
    one Device + encoder + plan per ordinal in ONE process, host -> slabs -> proc -> host and scatter -> proc -> gather, both
    compared with memcmp against the unsharded transform; Onlyinverse + Normalize shards undo it.  Over the visible devices
    (shards = 0) and over 2 / 3 contexts on device 0; small, odd-log2, two-pass 2^16 and the 2^20 pipeline."""
    exe, env = _build(tmp_path, "example_sharded")
    for lg, batch, shards in ((10, 37, 0), (10, 37, 2), (9, 5, 3), (16, 9, 2), (20, 9, 2), (11, 1, 2)):
        r = subprocess.run([exe, str(lg), str(batch), str(shards)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (lg, batch, shards, r.stdout, r.stderr)
        m = re.search(r"sharded ok: n=2\^(\d+) batch=(\d+) shards=(\d+) devices=(\d+)", r.stdout)
        assert "adapter 0: gfx950" in r.stdout and m, r.stdout
        assert (int(m.group(1)), int(m.group(2))) == (lg, batch) and int(m.group(3)) == (shards or int(m.group(4)))


_RCCL_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import fft_wgpu_amd as fw
import oracle
dev, queue = fw.prepare_gpu(0)
enc = dev.create_command_encoder()
n, batch = 4096, 13
x = oracle.gen_input(n, batch, first_transform=5)
uid = fw.Comm.unique_id()
assert len(uid) == 128 and any(uid)
comm = fw.Comm(dev, uid, 1, 0)
assert (comm.get("rank"), comm.get("world"), comm.get("device")) == (0, 1, 0)
full, slab, back = dev.create_buffer(x.nbytes), dev.create_buffer(x.nbytes), dev.create_buffer(x.nbytes)
queue.write_buffer(full, 0, x, encoder=enc)
comm.scatter(full, slab, n, batch, root=0, encoder=enc)                    # world 1: the root's own slab
out = fw.Forward(dev, queue, slab, n).proc(enc)
comm.gather(out, back, n, batch, root=0, encoder=enc)
y = back.map_read(stream=enc)
ref_buf = dev.create_buffer(x.nbytes)
queue.write_buffer(ref_buf, 0, x, encoder=enc)
ref = fw.Forward(dev, queue, ref_buf, n).proc(enc).map_read(stream=enc)
assert np.array_equal(y.view(np.uint64), ref.view(np.uint64))
# the RCCL data path itself: a grouped ncclSend + ncclRecv (to / from the own rank: the one peer a one-GPU box has)
ring = dev.create_buffer(x.nbytes)
half = x.nbytes // 2 // 8 * 8
comm.sendrecv(back, 0, half, 0, ring, x.nbytes - half, half, 0, encoder=enc)
z = ring.map_read(stream=enc)
assert np.array_equal(z[(x.nbytes - half) // 8:].view(np.uint64), ref[:half // 8].view(np.uint64))
# argument checks
for bad in (lambda: comm.sendrecv(back, 0, 16, 0, None, 0, 0, -1, encoder=enc),        # send to self without the receive
            lambda: comm.sendrecv(back, 0, 16, 1, ring, 0, 16, 1, encoder=enc),         # rank out of range
            lambda: comm.scatter(None, slab, n, batch, root=0, encoder=enc),           # root without the full buffer
            lambda: comm.scatter(full, slab, n, batch + 1, root=0, encoder=enc)):      # slab buffer too small
    try:
        bad()
    except fw.FwaError as e:
        assert e.status == 1, e
    else:
        raise AssertionError("accepted")
comm.destroy()
print("rccl leg ok")
"""


def test_comm_scatter_gather_over_rccl_in_a_child_process(gpu, tmp_path):
    """fwa_comm_* (RCCL loaded by the library with dlopen, ncclCommInitRank, grouped ncclSend / ncclRecv) on the one GPU of
    the box: a world of one rank -- scatter, transform, gather bit-identical to the plain transform, and one real grouped
    send + receive through RCCL (to the own rank).  Fresh child process with a timeout: RCCL initialises its own
    transport state and must not share a process with this test session's contexts."""
    script = tmp_path / "rccl_child.py"
    script.write_text(_RCCL_CHILD)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl leg ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_cpp_comm_rank_scatters_transforms_gathers(gpu, tmp_path):
    """fft_wgpu::Comm (include/fft_wgpu.hpp) from a compiled C++ host, the one-process-per-GPU form: tools/example_comm.cpp as the
    single rank this box can host (unique id -> communicator -> scatter -> Forward on the slab -> gather -> memcmp against the
    unsharded transform; one grouped send + receive).  A fresh process with a timeout, as every RCCL call of the test suite."""
    exe, env = _build(tmp_path, "example_comm")
    env = dict(env, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), FWA_COMM_ID_FILE=str(tmp_path / "comm_id"))
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    for lg, batch in ((12, 13), (9, 5), (16, 3)):
        r = subprocess.run([exe, str(lg), str(batch)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"comm ok: rank 0 of 1 on device 0, n=2^{lg} batch={batch}, slab [0, +{batch})" in r.stdout, (r.stdout, r.stderr[-3000:])
    assert len(open(tmp_path / "comm_id", "rb").read()) == 128


def test_stream_overlap_check_is_refused_during_capture_and_can_be_turned_off(gpu):
    """VERDICT round 3, item 5(b).  The overlap check behind fwa_stream_create / the chain streams launches spin kernels:
    it runs only when there is a peer to overlap with, never while a stream of the context captures a graph
    (FWA_ERR_UNSUPPORTED), and fwa_ctx_set_i64("chain_check", 0) turns it off."""
    fw, _, _ = gpu
    hip = hip_runtime()
    d = fw.Device(0)
    base = d.get("chain_checks")
    first = d.create_command_encoder()
    assert d.get("chain_checks") == base                                  # no peer yet: nothing launched
    second = d.create_command_encoder()
    assert d.get("chain_checks") > base                                   # checked against `first`
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0
    wrapped = d.create_command_encoder(hip_stream=stream)
    assert d.get("live_streams") == 4                                     # the null-stream encoder of Device + three
    graph = ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 2) == 0                      # hipStreamCaptureModeRelaxed
    with pytest.raises(fw.FwaError) as e:
        d.create_command_encoder()
    assert e.value.status == 6 and "capturing" in e.value.detail
    n_before = d.get("chain_checks")
    d.set("chain_check", 0)
    third = d.create_command_encoder()                                    # accepted as the runtime hands it out
    assert d.get("chain_checks") == n_before and d.get("chain_check") == 0
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    d.set("chain_check", 1)
    with pytest.raises(fw.FwaError):
        d.set("chain_check", 2)
    for enc in (first, second, third, wrapped):
        enc.destroy()
    assert d.get("live_streams") == 1
    assert hip.hipStreamDestroy(stream) == 0


def test_stream_and_buffer_handles_may_outlive_their_context(gpu, oracle):
    """A host with garbage collection frees in any order: destroying a stream or a buffer handle after its context is legal
    (using the stream is an error, not a crash), and the next launch on another context is unaffected."""
    fw, dev, queue = gpu
    d = fw.Device(0)
    enc = d.create_command_encoder()
    buf = d.create_buffer(1 << 20)
    L = d._L
    eh, bh = enc._h, buf._h
    enc._h = buf._h = None                       # keep the Python wrappers from freeing them first
    d._default.destroy()
    d.destroy()
    assert L.fwa_stream_synchronize(eh) == 1
    assert L.fwa_stream_destroy(eh) == 0 and L.fwa_buf_free(bh) == 0
    x = oracle.gen_input(1024, 3)
    y, _, _ = _run(fw, dev, queue, "Forward", x, 1024)
    mx, _ = oracle.compare(y[:1024], oracle.dft_f64(x[:1024], 1024, -1))
    assert mx <= 1e-5


def test_handles_freed_on_other_threads_while_their_context_is_destroyed(gpu, oracle):
    """Finalizers of a garbage-collected host run on other threads (ctypes releases the GIL during a call): four threads free
    64 buffer / event / stream handles through the raw ABI at the moment the main thread destroys their context.  Every call
    answers 0 -- the registry of fft_wgpu_amd/csrc/handles.h orders them, tests/test_handles.py races it under sanitizers on
    a CPU -- and the next launch on another context is unaffected.  Wrapped null streams only: a created stream would start
    the spin kernels of the overlap check."""
    import threading
    fw, dev, queue = gpu
    d = fw.Device(0)
    L = d._L
    owned = [d.create_buffer(4096) for _ in range(16)]
    backing = d.create_buffer(4096)
    views = [d.wrap_buffer(backing.device_ptr, 4096) for _ in range(16)]
    events = [fw.Event(d) for _ in range(16)]
    streams = []
    for _ in range(16):
        h = ctypes.c_void_p()
        assert L.fwa_stream_wrap(d._h, None, ctypes.byref(h)) == 0
        streams.append(h)
    assert d.get("live_streams") == 17 and d.get("live_buffers") == 33
    jobs = [(L.fwa_buf_free, b._h) for b in owned + views] + [(L.fwa_event_destroy, e._h) for e in events] \
        + [(L.fwa_stream_destroy, s) for s in streams]
    last, ctx = backing._h, d._h
    for w in owned + views + events + [backing, d]:
        w._h = None                              # keep the Python wrappers from freeing them first
    d._default.destroy()
    gate = threading.Barrier(5)
    status = [[] for _ in range(4)]

    def free_share(k):
        gate.wait()
        status[k] += [f(h) for f, h in jobs[k::4]]

    threads = [threading.Thread(target=free_share, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    gate.wait()
    destroyed = L.fwa_ctx_destroy(ctx)
    for t in threads:
        t.join()
    assert destroyed == 0 and [len(s) for s in status] == [16] * 4 and not any(sum(status, []))
    assert L.fwa_buf_free(last) == 0
    x = oracle.gen_input(1024, 3)
    y, _, _ = _run(fw, dev, queue, "Forward", x, 1024)
    mx, _ = oracle.compare(y[:1024], oracle.dft_f64(x[:1024], 1024, -1))
    assert mx <= 1e-5


def test_using_a_handle_after_its_context_is_an_error_code_not_a_dangling_pointer(gpu, oracle):
    """ShardedBatch.destroy() destroys the contexts it created while the caller may still hold
    buffers, events and encoders on `sb.devices[i]`.  fwa_ctx_destroy detaches every live buffer / event / stream handle of the
    context, so each later USE answers FWA_ERR_INVALID_ARG (status 1) with a message -- it must not dereference the freed
    context (`USE_DEVICE(buf->ctx)`) -- and the handles stay destroyable."""
    fw, dev, queue = gpu
    n, batch = 4096, 6
    x = oracle.gen_input(n, batch)
    sb = fw.ShardedBatch(fw.Forward, n, batch, ordinals=[0, 0])        # two contexts on device 0, created by the object
    sb.write(x)
    sb.proc()
    got = sb.read()
    d0 = sb.devices[0]
    L = d0._L
    mine = d0.create_buffer(n * 8)                 # the caller's own objects on a context the ShardedBatch owns
    wrapped = d0.wrap_buffer(mine.device_ptr, n * 8)
    other = dev.create_buffer(n * 8)               # a buffer of a context that stays alive
    enc = d0.create_command_encoder()
    ev = fw.Event(d0)
    ev.record(enc)
    assert d0.get("live_buffers") >= 3             # slab + mine + wrapped (+ second buffers)
    sb.destroy()                                   # destroys d0's context underneath `mine`, `wrapped`, `enc`, `ev`
    assert d0._h is None
    host = np.zeros(n, dtype=np.complex64)
    hp = host.ctypes.data_as(ctypes.c_void_p)
    INVALID = 1
    calls = {
        "upload": lambda: L.fwa_buf_upload(mine._h, 0, hp, host.nbytes, None),
        "download": lambda: L.fwa_buf_download(hp, mine._h, 0, host.nbytes, None),
        "download_async": lambda: L.fwa_buf_download_async(hp, wrapped._h, 0, host.nbytes, None),
        "copy_from": lambda: L.fwa_buf_copy(other._h, 0, mine._h, 0, host.nbytes, None),
        "copy_to": lambda: L.fwa_buf_copy(mine._h, 0, other._h, 0, host.nbytes, None),
        "fill": lambda: L.fwa_fill_synthetic(mine._h, 1, 0, n, 1.0, None),
        "calib_copy": lambda: L.fwa_calib_copy(mine._h, other._h, 4096, None),
        "event_record": lambda: L.fwa_event_record(ev._h, None),
        "event_sync": lambda: L.fwa_event_synchronize(ev._h),
        "stream_sync": lambda: L.fwa_stream_synchronize(enc._h),
    }
    for name, call in calls.items():
        assert call() == INVALID, name
        assert b"context has been destroyed" in L.fwa_last_error_string(None) or \
            b"context that has been destroyed" in L.fwa_last_error_string(None), name
    # a plan on a LIVE context refuses a buffer of the dead one
    h = ctypes.c_void_p()
    assert L.fwa_plan_create(dev._h, 0, n, mine._h, None, ctypes.byref(h)) == INVALID and not h.value
    assert b"destroyed" in L.fwa_last_error_string(dev._h)
    # size and pointer are still answered (plain reads of the handle), and every handle can still be freed
    assert mine.size == n * 8 and wrapped.device_ptr == mine.device_ptr
    for o in (wrapped, mine, enc):
        o.destroy()
    assert L.fwa_event_destroy(ev._h) == 0
    ev._h = None
    other.destroy()
    # the result read before the destroy is the unsharded transform; the surviving context still works
    y, _, _ = _run(fw, dev, queue, "Forward", x, n)
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32))
