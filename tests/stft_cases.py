"""The numeric checks of the framed real-input plans (TEST INFRASTRUCTURE ONLY): shapes, inputs, windows, the float64
reference, the bounds and a numpy complex64 model of the algorithm, shared by tests/test_gpu_stft.py (which applies the checks
to the GPU's results) and tests/test_stft.py (which applies them to the model and to its mutants, on the CPU).

Every check takes `run(output, x, n, hop, w)`: x (signals, L) float32, w (n,) float32 or None, output "Spectrum" or "Power";
it returns the (signals F, n / 2 + 1) complex64 or float32 rows of one exec.  A check returns its failures as strings and
prints every figure it measured.

Reference: numpy.fft.rfft(w64 * frames64, axis=-1) in float64 on the float32 inputs, frames64 =
sliding_window_view(x, n, axis=-1)[:, ::hop], computed once per shape and left unchanged.  Bounds:
  parity    per frame, oracle.compare's max_rel and rel-L2 <= REL_TOL (tests/conftest.py)
  budget    whole-buffer rel-L2 <= oracle.error_budget.cap(2 n), and the same cap on every class of
            side_sweeps.real_classes(n, "Forward", frames): an n-point real transform is log2 n rounding levels (cap(n), the
            bound of the real plans) and the f32 window product is one more, log2(2 n) in all
  power     |P - (re^2 + im^2)| <= 2.0001 * 2^-24 * (re^2 + im^2) against the Spectrum plan's own bits, in float64: two
            roundings of positive terms in any evaluation order or FMA contraction; NaN positions identical
  sweep     side_sweeps.real_failures: pi / 2^20 in angle and 1e-6 in modulus per output of every impulse position
Everything else is bit for bit.
"""
import numpy as np

import side_sweeps as ss
from conftest import REL_TOL
from oracle import error_budget as eb

LENGTHS = [1 << lg for lg in range(1, 13)]
HOP_LENGTHS = [2, 64, 128, 4096]                     # one butterfly; the last small length; the first network; the largest
POWER_BOUND = 2.0001 * 2.0 ** -24
MUTANTS = ("hop", "window_shift", "w_even_both", "no_signal_reset", "tail_frame", "power_mirror")


def hops(n):
    return sorted({1, 3, max(1, n // 2), n, n + 5})


def frames_per_signal(n, hop, L):
    assert hop >= 1 and L >= n
    return 1 + (L - n) // hop


def signal_len(n, hop, F, extra=1):
    """F frames and `extra` more samples, which fill no frame where extra < hop"""
    return (F - 1) * hop + n + extra


def default_shape(n):
    """(hop, signals, L).  n >= 128: 7 signals of 5 frames -- 35 frames, so 16-frame tiles straddle signal boundaries and the
    last tile is partial; n <= 64: 7 signals of 100 frames -- two full workgroups of 256 and a partial one.  One more sample
    than the frames need sits between two signals (at hop = 1 it makes one more frame)."""
    hop = max(1, n // 4)
    return hop, 7, signal_len(n, hop, 5 if n >= 128 else 100)


def hann(n):
    """the periodic Hann window in f32"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def random_window(n):
    return np.random.default_rng(0x57F7 + n).uniform(-1, 1, n).astype(np.float32)


def sweep_window(n):
    """exact in fp32, no zeros"""
    return (1 + (np.arange(n) % 8) / 8).astype(np.float32)


_inputs, _refs = {}, {}


def signals_input(n, hop, signals, L):
    """(signals, L) float32, uniform in (-1, 1), seeded by the shape, read-only; the samples of a signal's tail that fill no
    frame hold NaN"""
    key = (n, hop, signals, L)
    if key not in _inputs:
        x = np.random.default_rng([n, hop, signals, L % (1 << 31)]).uniform(-1, 1, (signals, L)).astype(np.float32)
        used = (frames_per_signal(n, hop, L) - 1) * hop + n
        x[:, used:] = np.nan
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def frames_of(x, n, hop):
    """(signals F, n): the frames, materialised"""
    v = np.lib.stride_tricks.sliding_window_view(x, n, axis=-1)[:, ::hop]
    assert v.shape[1] == frames_per_signal(n, hop, x.shape[1])
    return np.ascontiguousarray(v).reshape(-1, n)


def reference(x, n, hop, w, key=None):
    """float64 on the float32 inputs; cached under `key` when one is given"""
    if key is not None and key in _refs:
        return _refs[key]
    fr = frames_of(x, n, hop).astype(np.float64)
    if w is not None:
        fr = fr * w.astype(np.float64)
    r = np.fft.rfft(fr, axis=-1)
    if key is not None:
        r.setflags(write=False)
        _refs[key] = r
    return r


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the model ------------------------------------------------------------------------------------------------------
TABLE = (np.cos(2 * np.pi * np.arange(2048) / 4096).astype(np.float32)
         - 1j * np.sin(2 * np.pi * np.arange(2048) / 4096).astype(np.float32)).astype(np.complex64)


def model(output, x, n, hop, w, mutant=None):
    """kernels_stft.hip in numpy, complex64 / float32 throughout: frame addressing, the f32 window product, the half-length
    FFT, split_fwd, power.  mutant: one of MUTANTS, a deliberate mistake."""
    assert x.dtype == np.float32 and (w is None or w.dtype == np.float32) and mutant in (None,) + MUTANTS
    signals, L = x.shape
    M = n // 2
    F = frames_per_signal(n, hop, L)
    g = np.arange(signals * F)
    h = hop + 1 if mutant == "hop" else hop
    Fa = F + 1 if mutant == "tail_frame" else F                    # the tail of a signal taken for one more frame
    start = (g // Fa) * L + (g % Fa) * h
    if mutant == "no_signal_reset":
        start = g * h
    flat = np.concatenate([x.ravel(), np.zeros(int(start.max()) + n, dtype=np.float32)])
    fr = flat[start[:, None] + np.arange(n)[None, :]]
    if w is not None:
        if mutant == "window_shift":
            w = np.roll(w, 1)
        if mutant == "w_even_both":
            w = np.repeat(w[0::2], 2)
        fr = fr * w
    assert fr.dtype == np.float32
    z = (fr[:, 0::2] + 1j * fr[:, 1::2]).astype(np.complex64)
    Z = np.fft.fft(z, axis=-1) if M > 1 else z
    assert Z.dtype == np.complex64                                   # numpy transforms complex64 in fp32
    k = np.arange(M)
    i = k * (4096 // n)
    W = np.where((i & 2048) != 0, -TABLE[i & 2047], TABLE[i & 2047])
    Zr = np.conj(Z[:, (M - k) % M])
    X = (Z + Zr) * np.float32(0.5) + W * ((Z - Zr) * np.complex64(-0.5j))
    last = (Z[:, :1].real - Z[:, :1].imag).astype(np.complex64)
    X = np.concatenate([X, last], axis=1).astype(np.complex64)
    X.imag[:, 0] = np.where(np.isnan(X.real[:, 0]), np.nan, 0.0)   # Im X[0]: Im Z[0] - Im Z[0] in the kernel
    if output == "Spectrum":
        return X
    if mutant == "power_mirror":
        X = X[:, M - np.arange(M + 1)]
    return (X.real * X.real + X.imag * X.imag).astype(np.float32)


# ---- the checks -----------------------------------------------------------------------------------------------------
def check_parity(run, oracle, n, hop, signals, L, w, cached=True):
    x = signals_input(n, hop, signals, L)
    y = run("Spectrum", x, n, hop, w)
    ref = reference(x, n, hop, w, key=(n, hop, signals, L, None if w is None else w.tobytes()) if cached else None)
    frames = signals * frames_per_signal(n, hop, L)
    if y.shape != ref.shape:
        return ["n %d hop %d: %r rows, not %r" % (n, hop, y.shape, ref.shape)]
    worst = (0.0, 0.0)
    bad = []
    for f in range(frames):
        mx, l2 = oracle.compare(y[f], ref[f])
        if not (mx <= REL_TOL and l2 <= REL_TOL) and len(bad) < 8:
            bad.append("n %d hop %d signals %d L %d %s, frame %d: max_rel %.3g rel_l2 %.3g" %
                       (n, hop, signals, L, "windowed" if w is not None else "rectangular", f, mx, l2))
        worst = (max(worst[0], mx) if mx == mx else mx, max(worst[1], l2) if l2 == l2 else l2)
    print("parity n %d hop %d signals %d L %d %s: %d frames, worst max_rel %.3g rel_l2 %.3g" %
          (n, hop, signals, L, "windowed" if w is not None else "rectangular", frames, worst[0], worst[1]))
    return bad


def parity_shapes(n):
    """(hop, signals, L, windowed) of test_parity: the default shape windowed and rectangular, one frame of one signal,
    an odd L at an even hop (n >= 4), and every hop of hops(n) at the lengths of HOP_LENGTHS"""
    hop, signals, L = default_shape(n)
    out = [(hop, signals, L, True), (hop, signals, L, False), (hop, 1, n, True), (hop, 1, n, False)]
    if n >= 4:
        even = max(2, n // 4)
        odd_L = signal_len(n, even, 5, 1)
        out.append((even, 3, odd_L if odd_L % 2 else odd_L + 1, True))
        out.append((even, 3, odd_L if odd_L % 2 else odd_L + 1, False))
    if n in HOP_LENGTHS:
        for h in hops(n):
            F = 5 if n >= 128 else 100
            out.append((h, 3, signal_len(n, h, F), True))
            out.append((h, 2, signal_len(n, h, F, 0), False))
    return list(dict.fromkeys(out))


def budget_shape(n):
    """(hop, signals, L): 2^18 / n frames, at least 2^18 samples, four signals"""
    frames = -(-eb.MIN_SAMPLES // n)
    signals = 4
    hop = max(1, n // 4)
    return hop, signals, signal_len(n, hop, frames // signals, 0)


def cap(n):
    return float(eb.cap(2 * n))


def check_budget(run, n, w, name):
    """(whole-buffer rel-L2, per-class failures, spread) of one windowed exec"""
    hop, signals, L = budget_shape(n)
    x = signals_input(n, hop, signals, L)
    y = run("Spectrum", x, n, hop, w).astype(np.complex128)
    r = reference(x, n, hop, w)
    assert y.size >= eb.MIN_SAMPLES // 2 and x.size >= 0
    rel_l2 = float(np.sqrt((np.abs(y - r) ** 2).sum() / (np.abs(r) ** 2).sum()))
    print("budget n %d %s window, %d frames: rel_l2 %.4g = %.3f of the cap %.4g" % (n, name, y.shape[0], rel_l2, rel_l2 / cap(n), cap(n)))
    bad, spread = ss.class_failures(y, r, ss.real_classes(n, "Forward", y.shape[0]), cap(n), "stft %s n %d" % (name, n))
    return rel_l2, bad, spread


def check_power(run, n, hop, signals, L, w):
    x = signals_input(n, hop, signals, L).copy()
    x[0, min(L - 1, n // 2)] = np.nan                               # NaN positions must agree too
    S = run("Spectrum", x, n, hop, w)
    P = run("Power", x, n, hop, w)
    if P.dtype != np.float32 or P.shape != S.shape:
        return ["n %d: power rows %r %s against spectrum rows %r" % (n, P.shape, P.dtype, S.shape)]
    want = S.real.astype(np.float64) ** 2 + S.imag.astype(np.float64) ** 2
    bad = []
    if not np.array_equal(np.isnan(P), np.isnan(want)):
        bad.append("n %d hop %d: %d NaN positions differ" % (n, hop, int((np.isnan(P) != np.isnan(want)).sum())))
    if not np.isnan(want).any() or np.isnan(want).all():
        bad.append("n %d hop %d: the input's NaN reaches %d of %d values" % (n, hop, int(np.isnan(want).sum()), want.size))
    ok = ~np.isnan(want)
    err = np.abs(P.astype(np.float64)[ok] - want[ok])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(want[ok] > 0, err / want[ok], np.where(err > 0, np.inf, 0.0))))
    print("power n %d hop %d: worst |P - (re^2 + im^2)| / (re^2 + im^2) = %.4g = %.3f of the bound" % (n, hop, worst, worst / POWER_BOUND))
    wrong = np.flatnonzero(~(err <= POWER_BOUND * want[ok]))
    for i in wrong[:8]:
        bad.append("n %d hop %d, value %d: power %.9g against %.17g" % (n, hop, i, P[ok][i], want[ok][i]))
    return bad


def check_sweep(run, n):
    """hop = 1, one signal of 2 n - 1 samples with a unit at sample n - 1: frame f sees the unit at position n - 1 - f, times
    the window sample there.  Rows reversed and divided by the window in float64: the DFT matrix."""
    x = np.zeros((1, 2 * n - 1), dtype=np.float32)
    x[0, n - 1] = 1
    w = sweep_window(n)
    y = run("Spectrum", x, n, 1, w)
    if y.shape != (n, n // 2 + 1):
        return ["n %d: %r rows" % (n, y.shape)]
    rows = y[::-1].astype(np.complex128) / w.astype(np.float64)[:, None]
    return ss.real_failures(rows, n, "Forward")


def frames_holding(n, hop, L, s, p):
    """the frames g that contain sample p of signal s"""
    F = frames_per_signal(n, hop, L)
    return [s * F + f for f in range(F) if f * hop <= p < f * hop + n]


def check_special_values(run, n, output):
    hop, signals, L = default_shape(n)
    w = hann(n) if n >= 4 else sweep_window(n)                      # Hann of 2 points is {0, 1}
    x = signals_input(n, hop, signals, L)
    F = frames_per_signal(n, hop, L)
    used = (F - 1) * hop + n
    clean = run(output, x, n, hop, w)
    bad = []
    if np.isnan(clean).any():
        return ["n %d %s: the clean exec holds NaN" % (n, output)]
    for s, p in ((0, 0), (signals // 2, used // 2), (signals - 1, used - 1), (1, n - 1), (2, min(used - 1, n))):
        q = x.copy()
        q[s, p] = np.nan
        hit = frames_holding(n, hop, L, s, p)
        assert 1 <= len(hit) <= -(-n // hop)
        y = run(output, q, n, hop, w)
        nan_rows = np.isnan(y).any(axis=1)
        if not (np.isnan(y[hit]).all() and sorted(np.flatnonzero(nan_rows)) == hit):
            bad.append("n %d %s, NaN at sample %d of signal %d: NaN in frames %r, not exactly in all of %r" %
                       (n, output, p, s, list(np.flatnonzero(nan_rows)[:12]), hit))
        others = np.flatnonzero(~nan_rows)
        if not same_bits(y[others], clean[others]):
            bad.append("n %d %s, NaN at sample %d of signal %d: another frame changed" % (n, output, p, s))
    for j in (0, n - 1, n // 2):
        q = w.copy()
        q[j] = np.nan
        if not np.isnan(run(output, x, n, hop, q)).all():
            bad.append("n %d %s: a NaN at window sample %d does not reach every output" % (n, output, j))
    for e in (-40, 40):
        f = np.float32(2.0) ** np.float32(e)
        want = clean * (f if output == "Spectrum" else f * f)
        assert np.isfinite(want).all()
        for what, y in (("signal", run(output, x * f, n, hop, w)), ("window", run(output, x, n, hop, w * f))):
            if not same_bits(y, want):
                bad.append("n %d %s: %s times 2^%d does not scale the result exactly" % (n, output, what, e))
    return bad
