"""The numeric checks of the fused FFT-convolution plans (TEST INFRASTRUCTURE ONLY): inputs, the float64 reference, the
bounds and the one-hot sweep, shared by tests/test_gpu_conv.py (which applies them to the GPU's results) and
tests/test_conv.py (which applies them to a numpy complex64 model of the algorithm and to doctored results, on the CPU).

Reference: numpy.fft.ifft(numpy.fft.fft(x128, axis=-1) * h(H128[b % F]), axis=-1), h = conj for the correlating plans, times
n for the unscaled kind.  Bounds:
  parity    per row, oracle.compare's max_rel and rel-L2 <= REL_TOL (tests/conftest.py)
  cap       whole-buffer rel-L2 <= oracle.error_budget.cap(2 n n) = C 2^-24 sqrt(2 log2 n + 1): log2 n butterfly levels each
            way plus the multiply, the rule that gives cap(n) for one transform
  one-hot   per output, angle within 2 pi / 2^20 of the expected tone and modulus within 2e-6 of it, RELATIVE to 1 / n
            (|n |y| - 1| <= 2e-6, which is tighter than 2e-6 absolute around 1 / n): two unit-modulus twiddle chains, each
            at the bound tests/test_gpu_real.py uses for one
"""
import numpy as np

from conftest import REL_TOL
from oracle import error_budget as eb

LENGTHS = [1 << lg for lg in range(1, 13)]
SHAPES = [2, 32, 64, 512, 1024, 2048, 4096]          # one butterfly; last chunk-shape length; first network (8 x 8); 32-point
#                                                      stages (512, 1024); three stages (2048); RT = 8 (4096)
ONEHOT_LENGTHS = LENGTHS                             # the one-hot sweep runs at every length ...
ONEHOT_CONJ = (False, True)                          # ... through both conj_filter forms of the kernel (a one-hot 1 + 0i is its own conjugate)
KINDS = ("Convolve", "OnlyConvolve")
ONEHOT_ANGLE, ONEHOT_MODULUS = 2 * np.pi / 2 ** 20, 2e-6


def rows_per_block(n):
    """the geometry rule, written out here independently of conv_geom.h"""
    return 8192 // n if n <= 32 else (8 if n == 4096 else 16)


def default_batch(n):
    """one full workgroup and three more rows"""
    return rows_per_block(n) + 3


def cap(n):
    return float(eb.cap(2 * n * n))


_inputs, _refs = {}, {}


def inputs(oracle, n, batch, filters):
    """(x, H): (batch, n) and (filters, n) complex64 from the seeded generator, computed once per shape, read-only"""
    key = (n, batch, filters)
    if key not in _inputs:
        x = oracle.gen_input(n, batch, first_transform=5).reshape(batch, n)
        H = oracle.gen_input(n, filters, first_transform=1 << 20).reshape(filters, n)
        x.setflags(write=False)
        H.setflags(write=False)
        _inputs[key] = (x, H)
    return _inputs[key]


def cap_filters(oracle, n):
    """(3, n) complex64, read-only: a flat random spectrum, the spectrum of an exponentially decaying random impulse response
    (time constant n / 8 samples) and a low-pass with a 60-dB stop band (bins n / 4 .. 3 n / 4)"""
    key = ("cap", n)
    if key not in _inputs:
        flat = oracle.gen_input(n, 1, first_transform=(1 << 21) + 1).astype(np.complex128)
        taps = oracle.gen_input(n, 1, first_transform=(1 << 21) + 2).astype(np.complex128) * np.exp(-np.arange(n) / max(n / 8.0, 1.0))
        k = np.arange(n)
        low = np.where((k < n // 4) | (k > n - n // 4), 1.0, 1e-3).astype(np.complex128)
        H = np.stack([flat, np.fft.fft(taps), low]).astype(np.complex64)
        H.setflags(write=False)
        _inputs[key] = H
    return _inputs[key]


def cap_batch(n):
    """at least 2^18 samples, as every row of oracle.error_budget"""
    return -(-eb.MIN_SAMPLES // n)


def reference(x, H, kind, conj):
    """the float64 reference of one (inputs, kind, conj): complex128 (batch, n)"""
    batch, n = x.shape
    Hb = H.astype(np.complex128)[np.arange(batch) % H.shape[0]]
    r = np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * (np.conj(Hb) if conj else Hb), axis=-1)
    return r * n if kind == "OnlyConvolve" else r


def cached_reference(oracle, n, batch, filters, kind, conj):
    key = (n, batch, filters, kind, conj)
    if key not in _refs:
        x, H = inputs(oracle, n, batch, filters)
        _refs[key] = reference(x, H, kind, conj)
        _refs[key].setflags(write=False)
    return _refs[key]


def model(x, H, kind, conj, row_of=None, use_conj=None):
    """The algorithm in numpy complex64 (numpy.fft on complex64 runs in fp32): forward, times the filter row of the row,
    unscaled inverse, times 2^-log2 n for the scaled kind.  row_of / use_conj: what a doctored implementation would do."""
    batch, n = x.shape
    assert x.dtype == np.complex64 and H.dtype == np.complex64
    rows = np.arange(batch) % H.shape[0] if row_of is None else row_of(np.arange(batch))
    Hb = H[rows]
    if conj if use_conj is None else use_conj:
        Hb = np.conj(Hb)
    X = np.fft.fft(x, axis=-1)
    assert X.dtype == np.complex64
    y = np.fft.ifft(X * Hb, axis=-1)
    if kind == "OnlyConvolve":
        y = y * np.float32(n)
    assert y.dtype == np.complex64
    return y


# ---- parity and cap -------------------------------------------------------------------------------------------------
def row_errors(oracle, y, ref):
    """worst (max_rel, rel_l2) over the rows, NaN-propagating"""
    worst = (0.0, 0.0)
    for b in range(y.shape[0]):
        mx, l2 = oracle.compare(y[b], ref[b])
        worst = (max(worst[0], mx) if mx == mx else mx, max(worst[1], l2) if l2 == l2 else l2)
    return worst


def parity_failures(oracle, y, ref, what=""):
    mx, l2 = row_errors(oracle, y, ref)
    print("parity %s: worst max_rel %.3g rel_l2 %.3g" % (what, mx, l2))
    return [] if mx <= REL_TOL and l2 <= REL_TOL else ["%s: max_rel %.3g rel_l2 %.3g" % (what, mx, l2)]


def whole_rel_l2(y, ref):
    d = y.astype(np.complex128) - ref
    return float(np.sqrt((np.abs(d) ** 2).sum() / (np.abs(ref) ** 2).sum()))


def cap_failures(y, ref, n, what=""):
    v = whole_rel_l2(y, ref)
    print("cap %s: rel_l2 %.4g = %.3f of the cap %.4g" % (what, v, v / cap(n), cap(n)))
    return [] if v <= cap(n) else ["%s: whole-buffer rel_l2 %.4g above the cap %.4g" % (what, v, cap(n))]


# ---- every bin meets its own filter sample ----------------------------------------------------------------------------
def onehot_spot(n, b):
    return (7 * b + 3) % n


def onehot_inputs(n):
    """batch = F = n: filter row b is one-hot at bin b (1 + 0i), src row b is a unit impulse at p_b = (7 b + 3) mod n"""
    b = np.arange(n)
    x = np.zeros((n, n), dtype=np.complex64)
    H = np.zeros((n, n), dtype=np.complex64)
    x[b, onehot_spot(n, b)] = 1
    H[b, b] = 1
    return x, H


def onehot_failures(y, n, limit=8):
    """scaled kind: dst[b][j] = exp(2 pi i b (j - p_b) / n) / n; a filter sample applied to the wrong bin gives another
    tone or a zero row"""
    bad = []
    worst_angle = worst_modulus = 0.0
    j = np.arange(n)
    for b0 in range(0, n, 256):
        b = np.arange(b0, min(b0 + 256, n))[:, None]
        want = np.exp(2j * np.pi * ((b * (j[None, :] - onehot_spot(n, b))) % n) / n)
        got = y[b0:b0 + b.shape[0]].astype(np.complex128) * n
        with np.errstate(invalid="ignore"):
            angle = np.abs(np.angle(got * np.conj(want)))
            modulus = np.abs(np.abs(got) - 1.0)
        angle[np.isnan(angle)] = np.inf
        modulus[np.isnan(modulus)] = np.inf
        worst_angle, worst_modulus = max(worst_angle, float(angle.max())), max(worst_modulus, float(modulus.max()))
        for r in np.flatnonzero(~((angle <= ONEHOT_ANGLE) & (modulus <= ONEHOT_MODULUS)).all(axis=1)):
            if len(bad) < limit:
                bad.append("row %d: angle error %.3g, modulus error %.3g (relative to 1 / n)" % (b0 + r, angle[r].max(), modulus[r].max()))
    print("one-hot n %d: worst angle error %.3g (bound %.3g), worst modulus error %.3g (bound %.3g)"
          % (n, worst_angle, ONEHOT_ANGLE, worst_modulus, ONEHOT_MODULUS))
    return bad


# ---- shifts -------------------------------------------------------------------------------------------------------------
def shift_filter(n, q):
    """the f32-rounded spectrum of a unit impulse at q: convolving with it rotates a row by q"""
    k = np.arange(n)
    return np.exp(-2j * np.pi * ((q * k) % n) / n).astype(np.complex64).reshape(1, n)


def shifts(n):
    return sorted({1, n // 2, n - 1})
