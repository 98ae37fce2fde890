"""One plan on the device from a kind name to its result, and the parity metric (TEST INFRASTRUCTURE ONLY).

Every GPU test layer and every tool that runs a case does the same steps: open a context, allocate the buffers the kind
takes, build the plan (fft_wgpu_amd.plan_of_kind), set its tuning keys and read them back (_Plan.configure: a key the
plan ignored or clamped would run another kernel under the case's name), fill the source, exec, read the result, collect
the plan facts and tear everything down.  They are written here once:

  open_gpu      the context of a `gpu` fixture, with the no-GPU assertion
  upload        a fresh buffer holding `x`
  planned       context manager: the configured plan on its buffers and encoder, torn down on exit, also on an exception
  execute       one exec of it -> the buffer that holds the result and where that is ("src", "src2" or "plan")
  facts_of      path, factors, launches_per_exec and any further keys, as one dict
  run           all of it for one input -> (result, where, facts)

and the parity rule of the suite, per transform, with fwo_compare's definition (oracle/ref_fft.c; the C
function stays the cross-check, tests/test_device_run.py):

  blocks        y - r and r in complex128, at most 2^22 samples at a time (error_budget.metrics walks the same blocks)
  parity        (max_rel, rel_l2) of every transform
  parity_failures   the transforms that miss a tolerance; NaN fails

Importable from tests/ and tools/; nothing under fft_wgpu_amd/ imports it.
"""
import contextlib
import ctypes
import types

import numpy as np

FACTS = ("path", "factors", "launches_per_exec")
BLOCK = 1 << 22           # samples per block of the metric


def open_gpu(lab=False):
    """(fw, dev, queue) on device 0; lab: the laboratory build."""
    import fft_wgpu_amd as fw
    got = fw.prepare_gpu(0, lab=lab)
    assert got is not None, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    dev, queue = got
    return fw, dev, queue


def upload(dev, queue, x):
    buf = dev.create_buffer(x.nbytes)
    queue.write_buffer(buf, 0, x)          # no encoder: waits on the host
    return buf


@contextlib.contextmanager
def planned(fw, dev, queue, kind, n, nbytes=None, tunables=None, buffers=None):
    """The plan of `kind` with `tunables` set and read back, on fresh buffers of `nbytes` or on the caller's `buffers`
    (src, src2 or None: arena views, which stay the caller's) -> namespace(plan, enc, src, src2, queue, held).  The plan,
    the encoder and the buffers made here are destroyed on exit."""
    made = []
    try:
        if buffers is None:
            made += [dev.create_buffer(nbytes) for _ in range(2 if kind in fw.SECOND_BUFFER_KINDS else 1)]
            buffers = (made + [None])[:2]
        src, src2 = buffers
        enc = dev.create_command_encoder()
        made.append(enc)
        plan = fw.plan_of_kind(kind, dev, queue, src, src2, n)
        made.append(plan)
        held = plan.configure(tunables or {})
        yield types.SimpleNamespace(plan=plan, enc=enc, src=src, src2=src2, queue=queue, held=held)
    finally:
        for o in reversed(made):
            o.destroy()


def execute(p):
    """One exec of a `planned` plan, submitted (examples/basic.rs:84-104) -> (the buffer that holds the result, where)."""
    out = p.plan.proc(p.enc)
    p.queue.submit(p.enc.finish())
    return out, "src" if out is p.src else ("src2" if out is p.src2 else "plan")


def facts_of(plan, extra=()):
    return {k: int(plan.get(k)) for k in FACTS + tuple(extra)}


def run(fw, dev, queue, kind, x, n, tunables=None, facts=(), buffers=None, fill=None):
    """The reference call sequence (examples/basic.rs:73-122): write_buffer -> proc -> read back, on a plan of `kind` with
    `tunables` -> (result, where it landed, plan facts).  fill(src, src2) replaces the upload of `x` into src."""
    with planned(fw, dev, queue, kind, n, x.nbytes, tunables, buffers) as p:
        if fill is None:
            queue.write_buffer(p.src, 0, x)
        else:
            fill(p.src, p.src2)
        out, where = execute(p)
        return out.map_read(stream=p.enc), where, facts_of(p.plan, facts)


def hip_runtime():
    """The HIP runtime image this process already runs (the one the library resolved its libamdhip64 to -- torch's bundled
    copy if torch was imported first, else the system one; found in /proc/self/maps: no second runtime is loaded), with
    the signatures of the few calls the graph tests make themselves.  None where none is mapped."""
    with open("/proc/self/maps") as f:
        paths = [line.split()[-1] for line in f if "libamdhip64" in line]
    if not paths:
        return None
    hip = ctypes.CDLL(paths[0])
    P, PP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
    for name, args in (("hipStreamCreateWithFlags", [PP, ctypes.c_uint]), ("hipStreamDestroy", [P]),
                       ("hipStreamBeginCapture", [P, ctypes.c_int]), ("hipStreamEndCapture", [P, PP]),
                       ("hipGraphInstantiate", [PP, P, P, P, ctypes.c_size_t]), ("hipGraphLaunch", [P, P]),
                       ("hipGraphGetNodes", [P, PP, ctypes.POINTER(ctypes.c_size_t)]),
                       ("hipGraphNodeGetType", [P, ctypes.POINTER(ctypes.c_int)]),
                       ("hipGraphExecDestroy", [P]), ("hipGraphDestroy", [P])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, ctypes.c_int
    return hip


# ---- the parity metric ----------------------------------------------------------------------------------------------
def blocks(y, r, n):
    """(first transform, y - r, r) over `y` (complex64) against `r` (complex128), both n x batch, in complex128 blocks of at
    most BLOCK samples: whole transforms, or pieces of one where n > BLOCK."""
    y = np.asarray(y).reshape(-1, n)
    r = np.asarray(r).reshape(-1, n)
    rows = max(1, BLOCK // n)
    cols = min(n, BLOCK)
    for t0 in range(0, y.shape[0], rows):
        for k0 in range(0, n, cols):
            rb = r[t0:t0 + rows, k0:k0 + cols]
            yield t0, y[t0:t0 + rows, k0:k0 + cols].astype(np.complex128) - rb, rb


def _modulus(z):
    """sqrt(re^2 + im^2) of a complex block, as fwo_compare forms it (a new array)"""
    f = np.square(np.asarray(z, dtype=np.complex128).view(np.float64))
    s = f[:, 0::2] + f[:, 1::2]
    return np.sqrt(s, out=s)


def _sums_of_squares(a):
    """per row, added sample by sample as fwo_compare adds them; `a` is used up"""
    np.multiply(a, a, out=a)
    return np.add.accumulate(a, axis=1, out=a)[:, -1].copy()


def parity(y, r, n):
    """Per transform (max_k |y - r| / max_k |r|, rel-L2): two float64 arrays.  fwo_compare's definition, operation by
    operation: a modulus is sqrt(re^2 + im^2), the maximum of the differences propagates a NaN, that of the reference
    skips one, the sums run sample by sample, and where a reference transform is all zero the numerators stand alone."""
    batch = np.size(y) // n
    maxd, maxr, sd, sr = (np.zeros(batch) for _ in range(4))
    for t0, diff, rb in blocks(y, r, n):
        t = slice(t0, t0 + diff.shape[0])
        d, m = _modulus(diff), _modulus(rb)
        maxd[t] = np.maximum(maxd[t], d.max(axis=1))
        maxr[t] = np.fmax(maxr[t], np.fmax.reduce(m, axis=1))
        sd[t] += _sums_of_squares(d)
        sr[t] += _sums_of_squares(m)
    return maxd / np.where(maxr > 0, maxr, 1.0), np.sqrt(sd / np.where(sr > 0, sr, 1.0))


def parity_failures(y, r, n, tol):
    """-> ([(transform, max_rel, rel_l2)] of the transforms that miss `tol` in either figure (a NaN misses it), and the
    worst (max_rel, rel_l2) of the batch)."""
    mx, l2 = parity(y, r, n)
    bad = [(int(t), float(mx[t]), float(l2[t])) for t in np.flatnonzero(~((mx <= tol) & (l2 <= tol)))]
    return bad, (float(mx.max(initial=0.0)), float(l2.max(initial=0.0)))
