"""GPU: the framed real-input plans (include/fft_wgpu_amd_stft.h) -- rfft, or its squared modulus, of overlapping windowed
frames of long real signals, out of place, one launch.

Shapes, inputs, the float64 reference, the bounds and the checks themselves are tests/stft_cases.py's (tests/test_stft.py
applies the same checks to a numpy model and to its mutants on the CPU).  What only a GPU can show is here: the bits of a
rectangular plan against real.Forward over the materialised frames, containment inside guarded views, buffers past 4 GiB,
stream order and the status codes.  With STFT_RECORD=<path> in the environment the budget tests also write the measured
figures there (tests/golden/stft_error.json is such a record; no test pins to it).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # before the library: one HIP runtime in the process, the one torch brings (as in bench.py)

import guarded_arena as ga
import side_sweeps as ss
import stft_cases as sc
from oracle.device_run import open_gpu
import side_libs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 6


@pytest.fixture(scope="session")
def stft():
    return side_libs.load("stft")


@pytest.fixture(scope="session")
def real():
    return side_libs.load("real")


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


def out_spec(output, n, frames):
    """(bytes, dtype) of a plan's destination"""
    return (frames * (n // 2 + 1) * 8, np.complex64) if output == "Spectrum" else (frames * (n // 2 + 1) * 4, np.float32)


def run_on(stft, gpu, output, x, n, hop, w, views=None, keep=False):
    """upload -> one exec -> read back; on the (src, window, dst) views the caller owns or on fresh buffers at allocation
    bases.  keep: also return what src and the window hold after the exec."""
    fw, dev, queue = gpu
    signals, L = x.shape
    frames = signals * sc.frames_per_signal(n, hop, L)
    nbytes, dtype = out_spec(output, n, frames)
    own = views is None
    if own:
        src, win, dst = dev.create_buffer(x.nbytes), dev.create_buffer(4 * n) if w is not None else None, dev.create_buffer(nbytes)
    else:
        src, win, dst = views
    queue.write_buffer(src, 0, x)
    if w is not None:
        queue.write_buffer(win, 0, w)
    enc = dev.create_command_encoder()
    plan = getattr(stft, output)(dev, queue, src, dst, n, hop, L, window=win if w is not None else None)
    assert plan.get("launches_per_exec") == 1 and plan.get("frames") == frames and plan.get("fft_len") == n
    assert plan.get("windowed") == (w is not None) and plan.get("output") == (output == "Power")
    assert plan.proc(enc) is dst
    y = dst.map_read(stream=enc, dtype=dtype).reshape(frames, n // 2 + 1)
    after = None
    if keep:
        after = (src.map_read(stream=enc, dtype=np.float32).reshape(x.shape), win.map_read(stream=enc, dtype=np.float32) if w is not None else None)
    plan.destroy()
    enc.destroy()
    if own:
        for b in (src, win, dst):
            if b is not None:
                b.destroy()
    return (y, after) if keep else y


@pytest.fixture(scope="module")
def run(stft, gpu):
    return lambda output, x, n, hop, w: run_on(stft, gpu, output, x, n, hop, w)


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_parity(run, oracle, n):
    """per frame: the default shape windowed and rectangular, one frame of one signal, an odd L at an even hop, and
    hop = 1, 3, n / 2, n, n + 5 at n = 2, 64, 128, 4096"""
    bad = []
    for hop, signals, L, windowed in sc.parity_shapes(n):
        bad += sc.check_parity(run, oracle, n, hop, signals, L, sc.hann(n) if windowed else None)
    assert not bad, "\n".join(bad)


# ---- bit-identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_a_rectangular_plan_has_the_bits_of_real_forward_over_the_frames(stft, real, gpu, run, n):
    """at an even hop and an even L (the 8-byte load form), at an odd hop and at an odd L (the 4-byte form), and at hop = n"""
    fw, dev, queue = gpu
    F = 5 if n >= 128 else 300
    even = max(2, n // 4)
    shapes = [(even, 3, sc.signal_len(n, even, F, 2 if (n + (F - 1) * even) % 2 == 0 else 1)), (3, 3, sc.signal_len(n, 3, F, 0)),
              (even, 3, sc.signal_len(n, even, F, 1 if (n + (F - 1) * even) % 2 == 0 else 2)), (n, 2, sc.signal_len(n, n, F, 0))]
    assert shapes[0][2] % 2 == 0 and shapes[2][2] % 2 == 1
    for hop, signals, L in shapes:
        x = sc.signals_input(n, hop, signals, L)
        fr = sc.frames_of(x, n, hop)
        assert not np.isnan(fr).any()
        src, dst = dev.create_buffer(fr.nbytes), dev.create_buffer(fr.shape[0] * (n // 2 + 1) * 8)
        queue.write_buffer(src, 0, fr)
        enc = dev.create_command_encoder()
        plan = real.Forward(dev, queue, src, dst, n)
        plan.proc(enc)
        want = dst.map_read(stream=enc, dtype=np.complex64).reshape(fr.shape[0], n // 2 + 1)
        for h in (plan, enc, src, dst):
            h.destroy()
        got = run("Spectrum", x, n, hop, None)
        assert sc.same_bits(got, want), "n %d hop %d L %d: %d words differ" % (n, hop, L, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        p1, p2 = run("Power", x, n, hop, sc.hann(n)), run("Power", x, n, hop, sc.hann(n))
        assert sc.same_bits(p1, p2) and not np.isnan(p1).any()


# ---- budget ---------------------------------------------------------------------------------------------------------
_measured = {}
_budget_runs = {}
WINDOWS = {"hann": sc.hann, "random": sc.random_window}


def budget_run(run, n, name):
    if (n, name) not in _budget_runs:
        rel_l2, bad, spread = sc.check_budget(run, n, WINDOWS[name](n), name)
        hop, signals, L = sc.budget_shape(n)
        _measured["%d/%s" % (n, name)] = dict({"n": n, "window": name, "hop": hop, "signals": signals, "signal_len": L, "rel_l2": rel_l2,
                                               "cap": sc.cap(n)}, **ss.spread_record(spread))
        path = os.environ.get("STFT_RECORD")
        if path:
            with open(path, "w") as f:
                json.dump({"metric": "whole-buffer rel-L2 against numpy.fft.rfft of the windowed frames in float64; per class "
                                     "(tests/side_sweeps.py) as a fraction of the cap, oracle.error_budget.cap(2 n)",
                           "cases": _measured}, f, indent=1, sort_keys=True)
        _budget_runs[(n, name)] = (rel_l2, bad)
    return _budget_runs[(n, name)]


@pytest.mark.parametrize("name", sorted(WINDOWS))
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_budget(run, n, name):
    """windowed, >= 2^18 samples per length: whole-buffer rel-L2 under cap(2 n)"""
    rel_l2, _ = budget_run(run, n, name)
    assert rel_l2 <= sc.cap(n)


@pytest.mark.parametrize("name", sorted(WINDOWS))
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_budget_per_class(run, n, name):
    """the same exec: every class of frames and of bins under the same cap"""
    _, bad = budget_run(run, n, name)
    assert not bad, "\n".join(bad)


# ---- power, the DFT matrix, special values --------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_power_is_the_squared_modulus_of_the_spectrum_plans_bits(run, n):
    hop, signals, L = sc.default_shape(n)
    bad = sc.check_power(run, n, hop, signals, L, sc.hann(n)) + sc.check_power(run, n, 3, signals, sc.signal_len(n, 3, 40), None)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", sc.LENGTHS)
def test_dft_matrix_sweep(run, n):
    bad = sc.check_sweep(run, n)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("output", ("Spectrum", "Power"))
@pytest.mark.parametrize("n", [2, 16, 128, 4096])
def test_nan_stays_in_its_frames_and_powers_of_two_scale_exactly(run, n, output):
    bad = sc.check_special_values(run, n, output)
    assert not bad, "\n".join(bad)


# ---- containment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output", ("Spectrum", "Power"))
@pytest.mark.parametrize("n,signals,F", [(2, 3, 200), (64, 7, 100), (128, 7, 5), (4096, 1, 3)])
def test_plan_stays_inside_its_views(stft, gpu, run, oracle, n, signals, F, output):
    """src, window and dst as views inside one poisoned arena at the four START_EXTRAS offsets: no guard word changes, src and
    the window keep their bits, and dst has the bits of the same plan on buffers at allocation bases.  The last frame of the
    last signal ends exactly at the end of src.  600 and 700 frames: full workgroups of 256 and a partial one; 35 frames:
    16-frame tiles across signal boundaries; 3 frames: one partial tile."""
    fw, dev, queue = gpu
    hop = max(1, n // 4)
    L = sc.signal_len(n, hop, F, 0)
    assert (sc.frames_per_signal(n, hop, L) - 1) * hop + n == L
    x = sc.signals_input(n, hop, signals, L)
    w = sc.hann(n) if n >= 4 else sc.sweep_window(n)
    assert not sc.check_parity(run, oracle, n, hop, signals, L, w)             # identical, and not identically wrong
    base = run(output, x, n, hop, w)
    sizes = [x.nbytes, w.nbytes, out_spec(output, n, signals * F)[0]]
    G = ga.guard_bytes(n)
    bad = []
    arena = ga.GuardedArena(dev, queue, ga.arena_bytes(sizes, G + max(ga.START_EXTRAS), G), G)
    for e in ga.START_EXTRAS:
        views = arena.layout(sizes, G + e, names=["src", "window", "dst"])
        assert all(v.device_ptr % 16 == 0 for v in views) and views[0].device_ptr != arena.device_ptr
        y, (x_after, w_after) = run_on(stft, gpu, output, x, n, hop, w, views=views, keep=True)
        bad += ["G + %d: %s" % (e, m) for m in arena.check()]
        if not sc.same_bits(x_after, x):
            bad.append("G + %d: src changed" % e)
        if not sc.same_bits(w_after, w):
            bad.append("G + %d: the window changed" % e)
        if not sc.same_bits(y, base):
            bad.append("G + %d: the result differs from the base-buffer result in %d words" %
                       (e, int((y.view(np.uint32) != base.view(np.uint32)).sum())))
        for v in views:
            v.destroy()
        arena.views = []
    arena.destroy()
    assert not bad, "\n".join(bad)


# ---- past 4 GiB -----------------------------------------------------------------------------------------------------
def impulse_errors(y, p, n):
    k = np.arange(n // 2 + 1)
    want = np.exp(-2j * np.pi * ((p * k) % n) / n)
    y = y.astype(np.complex128)
    return float(np.abs(np.angle(y * np.conj(want))).max()), float(np.abs(np.abs(y) - 1.0).max())


def test_dst_past_4gib(stft, gpu):
    """n = 4096, hop = 1, one signal with F = 2^18 + 16 frames: 4 GiB + 2.25 MiB of spectra, zeroed on the device.  Unit
    impulses at sample 0 (frame 0 alone holds it), 100 samples into the frame whose row straddles byte 2^32 of dst, and at the
    last sample (the last frame alone holds it): those rows are held to the impulse bounds, sampled other rows stay zero."""
    fw, dev, queue = gpu
    n, M = 4096, 2048
    F = (1 << 18) + 16
    L = F - 1 + n
    row = (M + 1) * 8
    assert F * row > 1 << 32
    t_dst = torch.zeros(F * (M + 1), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    dst = dev.wrap_buffer(t_dst.data_ptr(), F * row)
    src = dev.create_buffer(L * 4)
    queue.write_buffer(src, 0, np.zeros(L, dtype=np.float32))
    straddle = ((1 << 32) - 1) // row
    assert straddle * row < 1 << 32 < (straddle + 1) * row
    for q in (0, straddle + 100, L - 1):
        queue.write_buffer(src, q * 4, np.array([1], dtype=np.float32))
    hot = {0: 0, straddle: 100, straddle + 1: 99, straddle + 100: 0, F - 1: n - 1}         # frame -> impulse position
    zero = [1, 16, 5000, straddle - n, straddle + 101, F - 17, F - 2]
    enc = dev.create_command_encoder()
    plan = stft.Spectrum(dev, queue, src, dst, n, 1, L)
    assert plan.get("frames") == F and plan.get("blocks") == F // 16 and plan.get("launches_per_exec") == 1
    plan.proc(enc)
    bad = []
    for f in sorted(set(hot) | set(zero)):
        y = dst.map_read(offset=f * row, size=row, stream=enc)
        if f in hot:
            angle, modulus = impulse_errors(y, hot[f], n)
            if not (angle <= ss.ANGLE and modulus <= ss.MODULUS):
                bad.append("frame %d: angle error %.3g, modulus error %.3g" % (f, angle, modulus))
        elif np.count_nonzero(y):
            bad.append("frame %d: %d outputs are not zero" % (f, np.count_nonzero(y)))
    for h in (plan, enc, src, dst):
        h.destroy()
    del t_dst
    torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


def test_src_past_4gib(stft, gpu):
    """n = 4096, two signals of L = 2^29 + 4097 samples, hop = 2^25: 17 frames per signal, 4 GiB + 32 KiB of signal, zeroed on
    the device.  Impulses in frame 0, in the last frame of signal 0, in the first frame of signal 1 (past byte 2^31) and in the
    last frame of all (past byte 2^32); sampled other frames stay exactly zero."""
    fw, dev, queue = gpu
    n, M = 4096, 2048
    L, hop, signals = (1 << 29) + 4097, 1 << 25, 2
    F = sc.frames_per_signal(n, hop, L)
    assert F == 17 and signals * L * 4 > 1 << 32 and L * 4 > 1 << 31
    t_src = torch.zeros(signals * L, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    src = dev.wrap_buffer(t_src.data_ptr(), signals * L * 4)
    row = (M + 1) * 8
    dst = dev.create_buffer(signals * F * row)
    hot = {0: 1, F - 1: 5, F: 2047, 2 * F - 1: n - 1}                            # frame -> impulse position
    for g, p in hot.items():
        at = (g // F) * L + (g % F) * hop + p
        assert at < signals * L
        queue.write_buffer(src, at * 4, np.array([1], dtype=np.float32))
    assert (L + 2047) * 4 > 1 << 31 and (L + (F - 1) * hop + n - 1) * 4 > 1 << 32
    enc = dev.create_command_encoder()
    plan = stft.Spectrum(dev, queue, src, dst, n, hop, L)
    assert plan.get("signals") == signals and plan.get("frames_per_signal") == F and plan.get("blocks") == 3
    plan.proc(enc)
    y = dst.map_read(stream=enc).reshape(signals * F, M + 1)
    bad = []
    for g in range(signals * F):
        if g in hot:
            angle, modulus = impulse_errors(y[g], hot[g], n)
            if not (angle <= ss.ANGLE and modulus <= ss.MODULUS):
                bad.append("frame %d: angle error %.3g, modulus error %.3g" % (g, angle, modulus))
        elif np.count_nonzero(y[g]):
            bad.append("frame %d: %d outputs are not zero" % (g, np.count_nonzero(y[g])))
    for h in (plan, enc, src, dst):
        h.destroy()
    del t_src
    torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ---- ordering -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 256, 4096])
def test_execs_are_stream_ordered_and_allocate_nothing(stft, gpu, run, n):
    """two windows: exec, copy the result away, copy the second window over the first, exec -- all on one stream with no
    host synchronisation in between.  The kept copy has the bits of a synchronised exec with the first window, dst those of
    one with the second."""
    fw, dev, queue = gpu
    hop, signals, L = sc.default_shape(n)
    x = sc.signals_input(n, hop, signals, L)
    w1, w2 = sc.hann(n), sc.random_window(n)
    want1, want2 = run("Spectrum", x, n, hop, w1), run("Spectrum", x, n, hop, w2)
    assert not sc.same_bits(want1, want2)
    src, win, other, dst, kept = (dev.create_buffer(b) for b in (x.nbytes, 4 * n, 4 * n, want1.nbytes, want1.nbytes))
    queue.write_buffer(src, 0, x)
    queue.write_buffer(win, 0, w1)
    queue.write_buffer(other, 0, w2)
    enc = dev.create_command_encoder()
    plan = stft.Spectrum(dev, queue, src, dst, n, hop, L, window=win)
    dev.poll()
    plan.proc(enc)
    enc.copy_buffer_to_buffer(dst, 0, kept, 0, want1.nbytes)
    enc.copy_buffer_to_buffer(other, 0, win, 0, 4 * n)
    plan.proc(enc)
    assert sc.same_bits(dst.map_read(stream=enc).reshape(want2.shape), want2)
    assert sc.same_bits(kept.map_read(stream=enc).reshape(want1.shape), want1)
    dev.poll()
    before = dev.stats()["mem_free_bytes"]
    for _ in range(10):
        plan.proc(enc)
    dev.poll()
    assert dev.stats()["mem_free_bytes"] == before
    plan.destroy()                                                           # the buffers outlive the plan
    assert sc.same_bits(dst.map_read(stream=enc).reshape(want2.shape), want2)
    for h in (enc, src, win, other, dst, kept):
        h.destroy()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_status_codes_and_lifetimes(stft, gpu):
    fw, dev, queue = gpu
    Lb = stft.lib()
    n, hop, L, signals = 64, 16, 64 + 16 * 5 + 3, 6
    F = sc.frames_per_signal(n, hop, L)
    assert F == 6
    xb, wb = dev.create_buffer(signals * L * 4), dev.create_buffer(n * 4)
    sb, pb = dev.create_buffer(signals * F * (n // 2 + 1) * 8), dev.create_buffer(signals * F * (n // 2 + 1) * 4)
    out = ctypes.c_void_p()

    def create(ctx, output, length, h, sig, src, win, dst):
        st = Lb.fwt_plan_create(ctx, output, length, h, sig, src, win, dst, ctypes.byref(out))
        if st == 0:
            Lb.fwt_plan_destroy(out)
        else:
            assert not out.value
        return st
    ok = (dev._h, 0, n, hop, L, xb._h, wb._h, sb._h)
    assert create(*ok) == 0 and create(dev._h, 1, n, hop, L, xb._h, wb._h, pb._h) == 0
    assert create(dev._h, 0, n, hop, L, xb._h, None, sb._h) == 0                # rectangular
    assert create(None, *ok[1:]) == INVALID_ARG
    assert create(dev._h, 0, n, hop, L, None, wb._h, sb._h) == INVALID_ARG and create(dev._h, 0, n, hop, L, xb._h, wb._h, None) == INVALID_ARG
    assert Lb.fwt_plan_create(*ok, None) == INVALID_ARG
    assert Lb.fwt_plan_exec(None, None) == INVALID_ARG
    for bad_len in (0, 48, 3):
        assert create(dev._h, 0, bad_len, hop, L, xb._h, wb._h, sb._h) == INVALID_ARG
    for output in (2, -1):
        assert create(dev._h, output, n, hop, L, xb._h, wb._h, sb._h) == INVALID_ARG
    for length, word in ((1, "2 .. 4096"), (8192, "4096")):
        with pytest.raises(fw.FwaError) as e:
            stft.Spectrum(dev, queue, xb, sb, length, hop, max(L, length))
        assert e.value.status == UNSUPPORTED and word in e.value.detail
    assert create(dev._h, 0, n, 0, L, xb._h, wb._h, sb._h) == INVALID_ARG       # hop = 0
    assert create(dev._h, 0, n, hop, n - 1, xb._h, wb._h, sb._h) == INVALID_ARG  # L < n
    assert create(dev._h, 0, n, hop, L + 1, xb._h, wb._h, sb._h) == INVALID_ARG  # src is not a whole number of signals
    assert create(dev._h, 0, n, hop, L, xb._h, wb._h, pb._h) == INVALID_ARG      # dst holds power rows
    assert create(dev._h, 1, n, hop, L, xb._h, wb._h, sb._h) == INVALID_ARG      # dst holds spectrum rows
    assert create(dev._h, 0, n, hop // 2, L, xb._h, wb._h, sb._h) == INVALID_ARG  # another hop: another F
    with pytest.raises(fw.FwaError) as e:
        stft.Spectrum(dev, queue, xb, sb, n, hop, L, window=sb)                # a window of another size
    assert e.value.status == INVALID_ARG and "window" in e.value.detail
    half = dev.wrap_buffer(wb.device_ptr, n * 2)
    assert create(dev._h, 0, n, hop, L, xb._h, half._h, sb._h) == INVALID_ARG
    # overlap: src with dst, window with dst; adjacent views are fine
    arena = dev.create_buffer(xb.size + sb.size + n * 4 + 64)
    v_src = dev.wrap_buffer(arena.device_ptr, xb.size)
    at = -(-xb.size // 16) * 16
    v_dst = dev.wrap_buffer(arena.device_ptr + at, sb.size)
    v_over = dev.wrap_buffer(arena.device_ptr + at - 16, sb.size)
    v_win_in = dev.wrap_buffer(arena.device_ptr + at + 16, n * 4)
    v_win = dev.wrap_buffer(arena.device_ptr + at + -(-sb.size // 16) * 16, n * 4)
    assert create(dev._h, 0, n, hop, L, v_src._h, v_win._h, v_dst._h) == 0
    with pytest.raises(fw.FwaError) as e:
        stft.Spectrum(dev, queue, v_src, v_over, n, hop, L)
    assert e.value.status == INVALID_ARG and "overlap" in e.value.detail
    assert create(dev._h, 0, n, hop, L, v_src._h, v_win_in._h, v_dst._h) == INVALID_ARG
    assert create(dev._h, 0, n, hop, L, xb._h, wb._h, xb._h) == INVALID_ARG      # dst == src
    # a buffer and a stream of another context; a buffer whose context was destroyed
    other = fw.Device(0)
    foreign, foreign_win = other.create_buffer(signals * L * 4), other.create_buffer(n * 4)
    assert create(dev._h, 0, n, hop, L, foreign._h, wb._h, sb._h) == INVALID_ARG
    assert create(dev._h, 0, n, hop, L, xb._h, foreign_win._h, sb._h) == INVALID_ARG
    plan = stft.Power(dev, queue, xb, pb, n, hop, L, window=wb)
    foreign_stream = other.create_command_encoder()
    assert Lb.fwt_plan_exec(plan._h, foreign_stream._h) == INVALID_ARG
    stale_stream = other.create_command_encoder()
    other.destroy()
    assert create(dev._h, 0, n, hop, L, foreign._h, wb._h, sb._h) == INVALID_ARG
    assert Lb.fwt_plan_exec(plan._h, stale_stream._h) == INVALID_ARG
    v = ctypes.c_int64()
    assert Lb.fwt_plan_get_i64(plan._h, b"no_such_key", ctypes.byref(v)) == INVALID_ARG
    g = stft.describe(n, hop, L, signals)
    assert {k: plan.get(k) for k in g} == g
    assert [plan.get(k) for k in ("fft_len", "hop", "signal_len", "signals", "frames", "output", "windowed", "launches_per_exec")] == \
        [n, hop, L, signals, signals * F, 1, 1, 1]
    plan.destroy()
    for h in (foreign, foreign_win, foreign_stream, stale_stream, half, v_src, v_dst, v_over, v_win_in, v_win, arena, xb, wb, sb, pb):
        h.destroy()
