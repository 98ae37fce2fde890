"""The complete impulse sweeps and the per-class error check of the four side libraries -- strided/, fft2d/, real/, conv/
(TEST INFRASTRUCTURE ONLY): inputs, float64 expectations, bounds and class maps, shared by the four GPU modules (which
apply them to the GPU's results) and by tests/test_side_sweeps.py (which applies them to a numpy complex64 model of the
shared register network and to doctored results, on the CPU).  Pure numpy.

Sweeps.  Every input holds one unit per line, at every position of the length in turn, so the outputs are the DFT matrix of
the kernel: entry (p, k) is exp(-+2 pi i ((p k) mod n) / n), the integer residue taken before the division and the value
read from a float64 table of the n roots.  EVERY output is compared, in blocks of at most 256 lines.  Bounds, the
project's own:
  strided, 2-D, real forward   pi / 2^20 in angle and 1e-6 in modulus, after the exact power-of-two scale is taken off
  real inverse                 2 (pi / 2^20 + 1e-6) absolute on the unscaled output (IMPULSE_ABS of test_gpu_real.py; the
                               scaled kind times n, an exact power of two, is held to the same figure)
  convolution                  conv_cases.onehot_failures, unchanged, now at every length
A failure names library, kind, n, impulse position, output index and both errors; the first 8 are kept.

Classes.  All these kernels give one thread a fixed set of elements and one lane group a fixed line of the tile, so a
precision loss confined to one such class is diluted 8- to 256-fold in the whole-buffer rel-L2.  class_errors() takes the
rel-L2 per class; the maps below are written out from the prose of the geometry headers (not from their code):
  strided            column mod 16 (mod 8 at n = 4096); n <= 32: column mod 256, the thread of k_strided_small
  row / real / conv  line mod RT (16; 8 at the 4096-point network)
  chunk shapes       the thread that owns the line: (line mod (8192 / cols)) * cols div 32, at most 256 classes; the fused
                     form also by the thread of its column phase
  k_real_small       line mod 256, the thread; mod 128 for the forward kind, whose n / 2 + 1 bins per row would leave a
                     class of 256 with 512 .. 1024 samples
  n >= 64            within a line, element index mod T (the thread) and div T (the register), T = n / points
Every class must hold >= MIN_CLASS_SAMPLES samples, which class_errors asserts: that caps what a map could hide.
"""
import numpy as np

LENGTHS = [1 << lg for lg in range(1, 13)]
SMALL = [n for n in LENGTHS if n <= 32]
KINDS = ("Forward", "Inverse", "Onlyinverse")
ANGLE, MODULUS = np.pi / 2 ** 20, 1e-6
REAL_INVERSE_ABS = 2 * (ANGLE + MODULUS)
MIN_CLASS_SAMPLES = 1024
ZERO_COLUMNS = 5
BLOCK = 256

# the register networks of 64 .. 4096 points: log2 n -> (r0, r1, r2, points per thread, lines per tile)
NETS = {6: (8, 8, 1, 8, 16), 7: (16, 8, 1, 16, 16), 8: (16, 16, 1, 16, 16), 9: (32, 16, 1, 32, 16), 10: (32, 32, 1, 32, 16),
        11: (32, 32, 2, 32, 16), 12: (32, 32, 4, 32, 8)}

# the cases of the sweeps, as the GPU modules parametrise them
STRIDED_CASES = [(n, kind) for n in LENGTHS for kind in KINDS]
REAL_CASES = [(n, kind) for n in LENGTHS for kind in KINDS]
FFT2D_KINDS = ("Forward", "Onlyinverse")
FFT2D_SHAPES = [(r, c) for r in SMALL for c in SMALL] + [(2, c) for c in LENGTHS if c > 32] + [(64, c) for c in SMALL]
FFT2D_CASES = [(r, c, kind) for r, c in FFT2D_SHAPES for kind in FFT2D_KINDS]


def lg2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def sign_of(kind):
    return -1.0 if kind == "Forward" else 1.0


def roots(n, sign):
    """exp(sign 2 pi i r / n), r < n, in float64: want[p, k] = roots[(p k) mod n]"""
    return np.exp(sign * 2j * np.pi * np.arange(n) / n)


class Worst:
    """the largest angle and modulus error a sweep met, as fractions of their bounds"""
    def __init__(self):
        self.angle = self.modulus = 0.0

    def fractions(self):
        return self.angle / ANGLE, self.modulus / MODULUS


def _unit_failures(got, want, where, what, bad, worst, limit):
    """got, want: complex128 blocks of one shape; want has modulus 1.  where(index tuple) names the impulse and the output."""
    with np.errstate(invalid="ignore"):
        angle = np.abs(np.angle(got * np.conj(want)))
        modulus = np.abs(np.abs(got) - 1.0)
    angle[np.isnan(angle)] = np.inf
    modulus[np.isnan(modulus)] = np.inf
    worst.angle, worst.modulus = max(worst.angle, float(angle.max())), max(worst.modulus, float(modulus.max()))
    wrong = ~((angle <= ANGLE) & (modulus <= MODULUS))
    if wrong.any():
        for idx in np.argwhere(wrong)[:max(0, limit - len(bad))]:
            idx = tuple(int(i) for i in idx)
            bad.append("%s, %s: angle error %.3g (bound %.3g), modulus error %.3g (bound %.3g)"
                       % (what, where(idx), angle[idx], ANGLE, modulus[idx], MODULUS))


# ---- strided: the columns of one n x (n + 5) matrix -------------------------------------------------------------------
def strided_input(n):
    """column c < n holds a unit at row c; the last five columns are zero and form a partial last tile at every n"""
    x = np.zeros((1, n, n + ZERO_COLUMNS), dtype=np.complex64)
    c = np.arange(n)
    x[0, c, c] = 1
    return x


def strided_failures(y, n, kind, worst=None, limit=8):
    """y[0, k, c] = exp(-+2 pi i c k / n) (/ n for Inverse) for c < n; the five zero columns come back exactly zero"""
    worst = worst or Worst()
    what = "strided %s n %d" % (kind, n)
    bad = []
    y = y.reshape(n, n + ZERO_COLUMNS)
    w, scale = roots(n, sign_of(kind)), float(n) if kind == "Inverse" else 1.0
    c = np.arange(n)
    for k0 in range(0, n, BLOCK):
        k = np.arange(k0, min(k0 + BLOCK, n))
        got = y[k0:k0 + k.size, :n].astype(np.complex128) * scale
        _unit_failures(got, w[(k[:, None] * c[None, :]) % n], lambda i: "impulse at row %d (column %d), output row %d" % (i[1], i[1], k0 + i[0]),
                       what, bad, worst, limit)
    rest = y[:, n:]
    for row, z in np.argwhere(rest != 0)[:max(0, limit - len(bad))]:
        bad.append("%s, zero column %d, output row %d: holds %r, not zero" % (what, n + z, row, complex(rest[row, z])))
    print("sweep %s: worst angle error %.3f of its bound, worst modulus error %.3f of its bound" % ((what,) + worst.fractions()))
    return bad


# ---- real ---------------------------------------------------------------------------------------------------------------
def real_input(n, kind):
    """Forward: batch n, row b a unit at b.  The inverse kinds: batch (n / 2 + 1) + (n / 2 - 1): a real unit at every bin,
    then an imaginary unit at every interior bin."""
    if kind == "Forward":
        return np.eye(n, dtype=np.float32)
    M = n // 2
    X = np.zeros((2 * M, M + 1), dtype=np.complex64)
    X[np.arange(M + 1), np.arange(M + 1)] = 1
    X[M + 1 + np.arange(M - 1), 1 + np.arange(M - 1)] = 1j
    return X


def real_failures(y, n, kind, worst=None, limit=8):
    """Forward: bin k of row b is exp(-2 pi i b k / n), k = 0 .. n / 2.  Inverse kinds, unscaled: a unit at bin q gives
    2 cos(2 pi q j / n) (1 at q = 0, (-1)^j at q = n / 2), a unit imaginary at an interior q gives -2 sin(2 pi q j / n)."""
    what = "real %s n %d" % (kind, n)
    bad = []
    M = n // 2
    if kind == "Forward":
        worst = worst or Worst()
        w = roots(n, -1.0)
        k = np.arange(M + 1)
        for b0 in range(0, n, BLOCK):
            b = np.arange(b0, min(b0 + BLOCK, n))
            _unit_failures(y[b0:b0 + b.size].astype(np.complex128), w[(b[:, None] * k[None, :]) % n],
                           lambda i: "impulse at %d, output bin %d" % (b0 + i[0], i[1]), what, bad, worst, limit)
        print("sweep %s: worst angle error %.3f of its bound, worst modulus error %.3f of its bound" % ((what,) + worst.fractions()))
        return bad
    w = roots(n, 1.0)
    j = np.arange(n)
    scale = float(n) if kind == "Inverse" else 1.0
    top = 0.0
    for b0 in range(0, 2 * M, BLOCK):
        b = np.arange(b0, min(b0 + BLOCK, 2 * M))
        imag = b > M
        q = np.where(imag, b - M, b)
        tone = w[(q[:, None] * j[None, :]) % n]
        weight = np.where((q == 0) | (q == M), 1.0, 2.0)[:, None]
        want = np.where(imag[:, None], -2.0 * tone.imag, weight * tone.real)
        err = np.abs(y[b0:b0 + b.size].astype(np.float64) * scale - want)
        err[np.isnan(err)] = np.inf
        top = max(top, float(err.max()))
        for r, s in np.argwhere(~(err <= REAL_INVERSE_ABS))[:max(0, limit - len(bad))]:
            bad.append("%s, unit %s at bin %d, output sample %d: error %.3g (bound %.3g)"
                       % (what, "1j" if imag[r] else "1", q[r], s, err[r, s], REAL_INVERSE_ABS))
    print("sweep %s: worst error %.3f of its bound" % (what, top / REAL_INVERSE_ABS))
    return bad


# ---- 2-D ----------------------------------------------------------------------------------------------------------------
def fft2d_batch(rows, cols):
    """the fused pairs take the full 2-D matrix; the row kernels one image per column position"""
    return rows * cols if rows <= 32 and cols <= 32 else cols


def fft2d_spot(rows, cols, b):
    """the impulse of image b"""
    b = np.asarray(b)
    return (b // cols, b % cols) if rows <= 32 and cols <= 32 else (b % rows, b)


def fft2d_input(rows, cols):
    batch = fft2d_batch(rows, cols)
    b = np.arange(batch)
    p, q = fft2d_spot(rows, cols, b)
    x = np.zeros((batch, rows, cols), dtype=np.complex64)
    x[b, p, q] = 1
    return x


def fft2d_failures(y, rows, cols, kind, worst=None, limit=8):
    """y[b, k, l] = exp(-+2 pi i (p k / rows + q l / cols)), (p, q) the impulse of image b"""
    worst = worst or Worst()
    what = "fft2d %s %d x %d" % (kind, rows, cols)
    bad = []
    batch = fft2d_batch(rows, cols)
    wr, wc = roots(rows, sign_of(kind)), roots(cols, sign_of(kind))
    k, l = np.arange(rows), np.arange(cols)
    step = max(1, min(BLOCK, (BLOCK * 4096) // (rows * cols)))              # at most 256 lines of 4096 samples
    for b0 in range(0, batch, step):
        b = np.arange(b0, min(b0 + step, batch))
        p, q = fft2d_spot(rows, cols, b)
        want = wr[(p[:, None] * k[None, :]) % rows][:, :, None] * wc[(q[:, None] * l[None, :]) % cols][:, None, :]
        _unit_failures(y[b0:b0 + b.size].astype(np.complex128), want,
                       lambda i: "impulse at (%d, %d), output (%d, %d)" % (p[i[0]], q[i[0]], i[1], i[2]), what, bad, worst, limit)
    print("sweep %s: worst angle error %.3f of its bound, worst modulus error %.3f of its bound" % ((what,) + worst.fractions()))
    return bad


# ---- classes ------------------------------------------------------------------------------------------------------------
def class_errors(y, ref, classes):
    """{map name: rel-L2 per class} of y against the float64 reference; classes: {name: integer array that broadcasts to
    y's shape}.  Asserts that every class of every map holds at least MIN_CLASS_SAMPLES samples."""
    d2 = np.abs(y.astype(ref.dtype) - ref) ** 2
    r2 = np.abs(ref) ** 2
    out = {}
    for name, ids in classes.items():
        flat = np.broadcast_to(ids, y.shape).ravel()
        count = np.bincount(flat)
        assert count.min() >= MIN_CLASS_SAMPLES, "%s: a class of %d samples, fewer than %d" % (name, count.min(), MIN_CLASS_SAMPLES)
        num, den = np.bincount(flat, weights=d2.ravel()), np.bincount(flat, weights=r2.ravel())
        with np.errstate(invalid="ignore", divide="ignore"):
            out[name] = np.sqrt(num / den)
    return out


def class_failures(y, ref, classes, cap, what):
    """(failures, {map: (min, max) as fractions of the cap}): every class of every map has rel-L2 <= cap"""
    bad, spread = [], {}
    for name, e in class_errors(y, ref, classes).items():
        spread[name] = (float(np.nanmin(e)) / cap, float(np.nanmax(e)) / cap)
        for c in np.flatnonzero(~(e <= cap))[:8]:
            bad.append("%s, class %d of '%s': rel_l2 %.4g above the cap %.4g" % (what, c, name, e[c], cap))
    lo, hi = min(v[0] for v in spread.values()), max(v[1] for v in spread.values())
    print("classes %s: %d maps, rel_l2 %.3f .. %.3f of the cap %.4g" % (what, len(spread), lo, hi, cap))
    return bad, spread


def spread_record(spread):
    """what the *_RECORD files keep of a case: per map and overall, min / max as a fraction of the cap"""
    return {"per_class_min_of_cap": min(v[0] for v in spread.values()), "per_class_max_of_cap": max(v[1] for v in spread.values()),
            "class_maps": {k: [v[0], v[1]] for k, v in sorted(spread.items())}}


def _in_line(n, element, axis_shape):
    """element index mod T and div T of an n-point network line; element: integer array already shaped for broadcast"""
    if n < 64:
        return {}
    points = NETS[lg2(n)][3]
    T = n // points
    return {"element mod %d" % T: (element % T).reshape(axis_shape), "element div %d" % T: np.minimum(element // T, points - 1).reshape(axis_shape)}


def _chunk_thread(cols, line):
    """the thread of the 256 that owns a line of cols <= 32 samples: 32 / cols whole lines each, 8192 / cols per chunk"""
    return ((line % (8192 // cols)) * cols) // 32


def strided_classes(n, howmany):
    """for (batch, n, howmany): the columns of each matrix"""
    col = np.arange(howmany)
    width = 256 if n <= 32 else NETS[lg2(n)][4]
    out = {"column mod %d" % width: (col % width).reshape(1, 1, howmany)}
    out.update({"row " + k: v for k, v in _in_line(n, np.arange(n), (1, n, 1)).items()})
    return out


def lines_classes(n, lines):
    """for (lines, n) complex rows of the row, real-network and convolution kernels: n >= 64 by line mod RT and by element;
    n <= 32 (the chunk shapes) by owning thread"""
    line = np.arange(lines)
    if n <= 32:
        return {"chunk thread": _chunk_thread(n, line).reshape(lines, 1)}
    RT = NETS[lg2(n)][4]
    out = {"line mod %d" % RT: (line % RT).reshape(lines, 1)}
    out.update(_in_line(n, np.arange(n), (1, n)))
    return out


def fft2d_classes(rows, cols, batch):
    """for (batch, rows, cols): the row pass over the batch * rows lines, then the column pass inside every image"""
    line = np.arange(batch * rows).reshape(batch, rows, 1)
    if cols <= 32:
        out = {"row pass: chunk thread": _chunk_thread(cols, line)}
    else:
        RT = NETS[lg2(cols)][4]
        out = {"row pass: line mod %d" % RT: line % RT}
        out.update({"row pass: " + k: v for k, v in _in_line(cols, np.arange(cols), (1, 1, cols)).items()})
    if rows <= 32 and cols <= 32:
        # column phase of the fused kernel: thread g * cols + c, g the run of 32 cols samples of the chunk
        flat = line * cols + np.arange(cols).reshape(1, 1, cols)
        out["column phase: thread"] = ((flat % 8192) // (32 * cols)) * cols + flat % cols
    else:
        out.update({"column pass: " + k: v for k, v in strided_classes(rows, cols).items()})
    return out


def real_classes(n, kind, batch):
    """Forward: (batch, n / 2 + 1) bins; the inverse kinds: (batch, n) real samples, sample j being part of element j div 2"""
    line = np.arange(batch).reshape(batch, 1)
    width = n // 2 + 1 if kind == "Forward" else n
    element = np.arange(width) if kind == "Forward" else np.arange(width) // 2
    if n <= 64:
        lanes = 128 if kind == "Forward" else 256
        return {"line mod %d" % lanes: line % lanes}
    M = n // 2
    RT = NETS[lg2(M)][4]
    out = {"line mod %d" % RT: line % RT}
    out.update(_in_line(M, element, (1, width)))
    return out
