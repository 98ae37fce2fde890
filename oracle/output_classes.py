"""Output classes of the main library's kernels (TEST INFRASTRUCTURE ONLY, pure numpy): the class maps, the per-class
metric and the complex64 model that CLASS_FACTOR comes from.

Every kernel of fft_wgpu_amd/csrc gives one thread a fixed set of outputs, so a precision loss confined to one thread,
register, wave or tile line is diluted 8- to 256-fold in the whole-buffer rel-L2 that oracle/error_budget.py holds.  The
maps below assign every output sample of a row of error_budget.MATRIX a class id below 256; ClassSums takes |y - r|^2 and
|r|^2 per class inside the loop error_budget.metrics already walks, and error_budget.check_classes holds every class.
The maps are written out from the prose of the kernel headers, not from their code (tests/test_output_classes.py proves
them against that prose):

  digit windows  every row.  The output index k splits into the digits the plan's factors give: one digit of log2 n bits
                 for the one-launch kernels and the literal recurrence (paths 0, 2); K1 = k mod N1, then K2, then K3 for
                 the 2^20 pipeline and the tiled plans (paths 1, 7: k = K1 + N1 K2 [+ N1 N2 K3]; pass A's thread and
                 register and the row inside pass C's tile are functions of K1, pass C's thread and register of the last
                 digit).  A digit of at most 8 bits is one map; a wider one gives two, its low 8 bits and its high 8 bits.
                 A class defined by up to 8 contiguous bits at either end of a digit -- thread k mod T and register k div T
                 of k_small32, wave, row in tile -- is then a union of whole classes of one map.
  chunk thread   k_chunk, n = 2 .. 256 (kernels_chunk.hip lines 8-16, 48-53, 72-87): with s the sample index mod 8192,
                 wave w = s div 2048 parks its samples at P = 1024 w + s mod 1024 of the half's LDS space; the arithmetic
                 thread is P div 16 for n <= 16 (whole transforms) and (P div n) (n / 16) + (k mod n / 16) from n = 32 on
                 (the last stage writes output q of thread t at t + b n / 16 + 16 q).
  chunk half     (s mod 2048) div 1024: which of the two halves the workgroup transforms the sample in.
  workgroup slot k_small32<9 .. 13>: transform b runs in slot b mod (256 / T), T = n / 32, of its workgroup; none at 2^14
                 and 2^15, where a workgroup holds one transform.

Every class of every map holds at least MIN_CLASS_SAMPLES samples (asserted: that caps what a map could hide); the matrix
runs at least 2^18 samples per case, so 256 classes always fit.

CLASS_FACTOR.  Every class must sit at or below CLASS_FACTOR x cap(n).  The factor is not taken from the GPU: it is the
largest (worst class / whole-buffer rel-L2) of a numpy complex64 model of the same arithmetic class on the same
oracle.gen_input data through the same maps, times 1.1 (the model's stage order is not the kernels', and a 1024-sample
class carries 2-3 % sampling noise), rounded up to the next 0.05.  The model (model_fft) is a mixed-radix
decimation-in-time FFT whose outer radices are the row's digits; inside a digit the radix is 32 (then the rest), and a
butterfly of up to 32 points is a radix-2 network; every level multiplies by W^(j K) from a float64 table rounded to
float32.  Its table (tests/test_output_classes.py recomputes it and holds every ratio at or below CLASS_FACTOR / 1.1):

  row                      whole / cap(n)   best class / whole   worst class / whole   worst class's map
  chunk_2                  exact            -                    -                     -
  chunk_4                  0.238            0.872                1.109                 chunk thread
  chunk_8                  0.363            0.848                1.131                 k
  chunk_16                 0.443            0.769                1.222                 k
  chunk_32                 0.496            0.728                1.284                 k
  chunk_64                 0.521            0.714                1.279                 k
  chunk_128                0.518            0.744                1.239                 chunk thread
  chunk_256                0.528            0.736                1.247                 k
  small32_9                0.552            0.720                1.297                 k low 8 bits
  small32_10               0.577            0.701                1.357                 k low 8 bits
  small32_11               0.586            0.715                1.337                 k low 8 bits
  small32_12               0.580            0.725                1.299                 k low 8 bits
  small32_13               0.584            0.744                1.274                 k low 8 bits
  small32_14               0.599            0.780                1.224                 k low 8 bits
  small32_15               0.615            0.762                1.233                 k low 8 bits
  tile_2^16x4              0.589            0.810                1.187                 K2
  factors_6_6_6_2^18x1     0.634            0.861                1.140                 K3
  mid_tile_9_2^21x2        0.639            0.838                1.160                 K2 low 8 bits

The worst ratio is 1.357 (1024 points, 'k low 8 bits': a class there is 4 outputs of 256 transforms, and the outputs of
one transform differ by the twiddles they met, beyond the sampling noise), so CLASS_FACTOR = ceil(1.1 x 1.357 / 0.05)
x 0.05 = 1.50.  The model's whole-buffer figure sits at 0.24-0.64 of cap(n), so its worst class sits at 0.79 of cap(n) at
the most; a class at twice its error does not pass the pin (error_budget.PIN_REL_L2 x the recorded worst class of its
map), which is the sharp layer, and the cap is the backstop against re-recording a bad class.
"""
import numpy as np

MIN_CLASS_SAMPLES = 1024
MAX_CLASSES = 256
PATH_ONE_LAUNCH, PATH_LITERAL = 0, 2          # one digit; the 2^20 pipeline (1) and the tiled plans (7) have their factors'

# The rows of error_budget.MATRIX the model runs: every one-launch length, and one row per tiled digit shape (two passes,
# three passes, and 64 x 512 x 64, the shape of the record's worst row).
MODEL_ROWS = (["chunk_%d" % (1 << lg) for lg in range(1, 9)] + ["small32_%d" % lg for lg in range(9, 16)]
              + ["tile_2^16x4", "factors_6_6_6_2^18x1", "mid_tile_9_2^21x2"])

CLASS_FACTOR = 1.50


def lg2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


# ---- the maps ---------------------------------------------------------------------------------------------------------
def digits(case):
    """log2 of the digits of the output index, least significant first"""
    if case["path"] in (PATH_ONE_LAUNCH, PATH_LITERAL):
        return [lg2(case["n"])]
    lgs = [case["factors"] >> s & 255 for s in (0, 8, 16)]
    lgs = [v for v in lgs if v]
    assert sum(lgs) == lg2(case["n"]), case
    return lgs


def digit_spans(case):
    """[(digit name, shift, bits)]: digit = k >> shift & (2^bits - 1)"""
    lgs = digits(case)
    return [("k" if len(lgs) == 1 else "K%d" % (i + 1), sum(lgs[:i]), lg) for i, lg in enumerate(lgs)]


def windows_of_digit(name, shift, lg):
    """{map name: (shift, bits)} of one digit: the digit itself up to 8 bits, else its low and its high 8 bits"""
    if lg <= 8:
        return {name: (shift, lg)}
    return {name + " low 8 bits": (shift, 8), name + " high 8 bits": (shift + lg - 8, 8)}


def digit_windows(case):
    """{map name: (shift, bits)}: class id = k >> shift & (2^bits - 1)"""
    out = {}
    for span in digit_spans(case):
        out.update(windows_of_digit(*span))
    return out


def window_ids(n, window):
    """the class id of every k < n, shape (1, n)"""
    shift, bits = window
    return (np.arange(n, dtype=np.int64) >> shift & ((1 << bits) - 1)).reshape(1, n)


def window_sums(v, window):
    """sum of the length-n vector v per class of a window: what bincount(window_ids, weights=v) gives, without the ids"""
    shift, bits = window
    return v.reshape(-1, 1 << bits, 1 << shift).sum(axis=(0, 2))


def all_window_sums(v, case):
    """{map name: window_sums(v, window)} of every digit window of the case: v is reduced to one vector per digit first (one
    pass over v per digit), the windows of a digit are taken from that"""
    out = {}
    for name, shift, lg in digit_spans(case):
        digit = window_sums(v, (shift, lg))
        out.update({m: window_sums(digit, (s - shift, b)) for m, (s, b) in windows_of_digit(name, shift, lg).items()})
    return out


def chunk_maps(n, batch):
    """{map name: ids of shape (batch, n)} of k_chunk, n <= 256"""
    s = np.arange(batch * n, dtype=np.int64).reshape(batch, n) % 8192
    P = 1024 * (s // 2048) + s % 1024
    thread = P // 16 if n <= 16 else (P // n) * (n // 16) + (s % n) % (n // 16)
    return {"chunk thread": thread, "chunk half": (s % 2048) // 1024}


def slot_map(n, batch):
    """{map name: ids of shape (batch, 1)} of k_small32<9 .. 13>"""
    T = n // 32
    return {"workgroup slot": (np.arange(batch, dtype=np.int64) % (256 // T)).reshape(batch, 1)}


def kernel_maps(case):
    """{map name: ids of shape (batch, n) or (batch, 1)}: the maps beyond the digit windows"""
    n, batch = case["n"], case["batch"]
    if case["path"] != PATH_ONE_LAUNCH or n > 1 << 13:
        return {}
    return chunk_maps(n, batch) if n <= 256 else slot_map(n, batch)


def maps_of(case):
    """{map name: integer array that broadcasts to (batch, n)} of a row of error_budget.MATRIX, every map written out"""
    out = {name: window_ids(case["n"], w) for name, w in digit_windows(case).items()}
    out.update(kernel_maps(case))
    return out


def class_counts(case):
    """{map name: samples per class}, from the maps alone"""
    n, batch = case["n"], case["batch"]
    out = {name: count.astype(np.int64) * batch for name, count in all_window_sums(np.ones(n, dtype=np.uint8), case).items()}
    for name, ids in kernel_maps(case).items():
        assert ids.min() >= 0, name
        out[name] = np.bincount(ids.ravel()) * ((batch * n) // ids.size)
    assert all(len(c) <= MAX_CLASSES for c in out.values())
    return out


# ---- the metric -------------------------------------------------------------------------------------------------------
class ClassSums:
    """sum |y - r|^2 and sum |r|^2 per class of every map of `case`, block by block (error_budget.metrics feeds it).  The
    digit windows depend on k alone: a block is first summed over its transforms, that vector is reduced to one vector
    per digit (a block is 2^l consecutive k starting at a multiple of 2^l, so the bits of a digit above l are the same for
    the whole block), and the windows of a digit are taken from the digit's vector at the end: the 2^24 .. 2^26 rows cost
    one pass per digit and no buffer of their size."""
    def __init__(self, case):
        for name, count in class_counts(case).items():
            assert count.min() >= MIN_CLASS_SAMPLES, "%s, '%s': a class of %d samples, fewer than %d" % (
                case.get("id", case.get("case")), name, count.min(), MIN_CLASS_SAMPLES)
        self.maps = kernel_maps(case)
        self.digits = {span: np.zeros((2, 1 << span[2])) for span in digit_spans(case)}
        self.sums = {name: np.zeros((2, int(ids.max()) + 1)) for name, ids in self.maps.items()}

    def add(self, t0, k0, d2, r2):
        """d2 = |y - r|^2 and r2 = |r|^2 of transforms t0 .., outputs k0 .. (float64, one shape)"""
        rows, cols = d2.shape
        l = lg2(cols)
        assert k0 % cols == 0
        for i, v in enumerate((d2, r2)):
            v = v[0] if rows == 1 else v.sum(axis=0)
            for (_, shift, lg), acc in self.digits.items():
                inside = max(0, min(lg, l - shift))                       # the bits of the digit that vary inside the block
                first = k0 >> shift & ((1 << lg) - 1)
                acc[i, first:first + (1 << inside)] += v.reshape(-1, 1 << inside, 1 << min(shift, l)).sum(axis=(0, 2))
        for name, acc in self.sums.items():
            ids = self.maps[name][t0:t0 + rows]
            ids = np.broadcast_to(ids[:, k0:k0 + cols] if ids.shape[1] != 1 else ids, d2.shape).ravel()
            acc[0] += np.bincount(ids, weights=d2.ravel(), minlength=acc.shape[1])
            acc[1] += np.bincount(ids, weights=r2.ravel(), minlength=acc.shape[1])

    def errors(self):
        """{map name: rel-L2 per class}, as side_sweeps.class_errors defines it"""
        pairs = {}
        for (name, shift, lg), acc in self.digits.items():
            for m, (s, b) in windows_of_digit(name, shift, lg).items():
                pairs[m] = (window_sums(acc[0], (s - shift, b)), window_sums(acc[1], (s - shift, b)))
        pairs.update({name: (acc[0], acc[1]) for name, acc in self.sums.items()})
        out = {}
        for name, (num, den) in pairs.items():
            with np.errstate(invalid="ignore", divide="ignore"):
                out[name] = np.sqrt(num / den)
        return out


def spread(errors, cap):
    """{map name: (min, max) as fractions of the cap}; a NaN class makes the max NaN"""
    return {name: (float(np.min(e)) / cap, float(np.max(e)) / cap) for name, e in errors.items()}


def spread_record(sp):
    """what the record keeps of a case, in the shape of side_sweeps.spread_record"""
    return {"per_class_min_of_cap": min(v[0] for v in sp.values()), "per_class_max_of_cap": max(v[1] for v in sp.values()),
            "class_maps": {k: [v[0], v[1]] for k, v in sorted(sp.items())}}


# ---- the model --------------------------------------------------------------------------------------------------------
def _table(n, sign):
    """W_n^e = exp(sign 2 pi i e / n), e < n: float64 values rounded to float32"""
    return np.exp(sign * 2j * np.pi * np.arange(n) / n).astype(np.complex64)


def _butterfly2(a, sign):
    return np.stack([a[..., 0] + a[..., 1], a[..., 0] - a[..., 1]], axis=-1)


def _dit(a, radices, sign, inner):
    """The transform of the last axis of `a` (complex64), n = prod(radices): input j = j1 n / r + j2 and output
    k = K1 + r k2 with r = radices[0]; `inner` transforms r points, W_n^(j2 K1) follows, the rest recurses over j2."""
    n, r = a.shape[-1], radices[0]
    if len(radices) == 1:
        return inner(a, sign)
    M = n // r
    lead = a.shape[:-1]
    v = inner(np.ascontiguousarray(np.swapaxes(a.reshape(lead + (r, M)), -1, -2)), sign)        # [j2, K1]
    v = v * _table(n, sign)[np.arange(M)[:, None] * np.arange(r)[None, :]]
    v = _dit(np.ascontiguousarray(np.swapaxes(v, -1, -2)), radices[1:], sign, inner)            # [K1, k2]
    assert v.dtype == np.complex64
    return np.ascontiguousarray(np.swapaxes(v, -1, -2)).reshape(lead + (n,))                    # [k2, K1]


def _radix2_network(a, sign):
    """up to 32 points: radix-2 stages"""
    return _dit(a, [2] * lg2(a.shape[-1]), sign, _butterfly2) if a.shape[-1] > 1 else a


def _digit(a, sign):
    """one digit: radix 32, then the rest"""
    lg = lg2(a.shape[-1])
    return _dit(a, [32] * (lg // 5) + ([1 << lg % 5] if lg % 5 else []), sign, _radix2_network)


def model_fft(x, n, digit_lgs, sign=-1):
    """complex64 mixed-radix FFT of the rows of x (unscaled): outer radices 2^digit_lgs, least significant output digit
    first, radix 32 inside a digit, float32-rounded float64 twiddles"""
    a = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1, n)
    assert sum(digit_lgs) == lg2(n)
    return _dit(a, [1 << lg for lg in digit_lgs], float(sign), _digit).reshape(-1)


def class_factor(worst_ratio):
    """the worst (class / whole-buffer) ratio of the model, times 1.1, rounded up to the next 0.05"""
    return float(np.ceil(1.1 * worst_ratio / 0.05 - 1e-9) * 0.05)


def model_row(case, x, ref, sign=-1):
    """(whole-buffer rel-L2, {map: rel-L2 per class}) of the model on a row's input against its float64 reference"""
    n = case["n"]
    y = model_fft(x, n, digits(case), sign)
    sums = ClassSums(case)
    rows = max(1, (1 << 22) // n)
    y2, r2 = y.reshape(-1, n), np.asarray(ref).reshape(-1, n)
    for t0 in range(0, y2.shape[0], rows):
        rb = r2[t0:t0 + rows]
        sums.add(t0, 0, np.abs(y2[t0:t0 + rows].astype(np.complex128) - rb) ** 2, np.abs(rb) ** 2)
    total = next(iter(sums.digits.values())).sum(axis=1)
    whole = float(np.sqrt(total[0] / total[1]))
    return whole, sums.errors(), y


def model_table(gen_input, rows):
    """[(row, whole-buffer rel-L2, best class / whole, worst class / whole, the worst class's map)] of the model over
    `rows` (case dicts), on gen_input(n, batch) against numpy's float64 FFT.  Where the model is exact on this input
    (n = 2: one addition per output) there is no ratio and the row reads 0, 0, 0."""
    out = []
    for case in rows:
        n, batch = case["n"], case["batch"]
        x = gen_input(n, batch)
        ref = np.fft.fft(x.astype(np.complex128).reshape(batch, n), axis=1)
        whole, errors, _ = model_row(case, x, ref)
        if whole == 0.0:
            out.append((case["case"], 0.0, 0.0, 0.0, "-"))
            continue
        worst = max(errors, key=lambda name: errors[name].max())
        out.append((case["case"], whole, float(min(e.min() for e in errors.values())) / whole,
                    float(errors[worst].max()) / whole, worst))
    return out
