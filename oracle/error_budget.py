"""Error budget of every kernel family (TEST INFRASTRUCTURE ONLY): the case matrix, the metric and the rule.

The north-star bound of the parity tests (1e-5, tests/conftest.py REL_TOL) is 30-60x looser than what the kernels
reach, so a twiddle bug that makes a family 2-3x less accurate passes it.  This module holds each family to its own
measured fp32 error instead.  tools/record_error_budget.py runs MATRIX on the GPU and writes RECORD_PATH;
tests/test_gpu_error_budget.py runs it again and applies `check`; tests/test_error_budget.py checks the record on
the CPU.

Metric, per case (one plan kind at one (n, batch) with its tunables), against oracle.dft_f64 (divided by n for
Inverse), on the seeded generator input oracle.gen_input:
  * rel_l2  = sqrt(sum |y - r|^2 / sum |r|^2) over the whole batch;
  * max_rel = the worst per-transform max_k |y - r| / max_k |r| (oracle.compare's definition).
Every case with n <= 2^18 runs at least 2^18 samples, so that rel_l2 averages over many roundings.

Rule, per case:
  (a) pin: rel_l2 <= PIN_REL_L2 x the recorded rel_l2 and max_rel <= PIN_MAX_REL x the recorded max_rel.  GPU results
      are bit-deterministic for a fixed input, so this is the sharp layer: an accuracy regression has to be
      re-recorded on purpose.
  (b) cap: rel_l2 <= cap(n) = C * 2^-24 * sqrt(log2 n), one C for every family: the backstop against re-recording
      a bad number.  The cap bounds rel_l2, the averaged metric; max_rel, an extreme-value statistic of one
      transform, is held by the pin and by MAX_REL_CAP_FACTOR x cap(n).
C = 1.05, chosen from the record so that the worst family sits at <= 0.8 of its cap: the three-pass tiled plans, whose
k_tile passes multiply two-level twiddles (hi[e >> 10] * lo[e & 1023], tables.cpp upload_level) into one more rounded
product, with rel_l2 / cap = 0.784 at 2^24 (rel_l2 2.40e-7; 2^20 x 1, 64 x 64 x 256: 0.775).  C was chosen from the
hand-picked rows and has not moved for the cell rows added since (below), all of which sit under the cap: the two-pass
ones at 0.71-0.73, the three-pass ones at 0.74 (64 x 64 x 128), 0.79 (64 x 64 x 1024), 0.80 (64 x 1024 x 64) and 0.851
(64 x 512 x 64, rel_l2 2.44e-7: the worst of the record).  k_tile at 512 and 1024 points has two twiddled radix-16 stages
where 64 .. 256 points have one, and three such passes stack them; the error of those rows is the same to three digits
in every transform and in all three plan kinds.

Per output class.  Every kernel gives one thread a fixed set of outputs, so a loss confined to one thread, register, wave
or tile line is diluted 8- to 256-fold in rel_l2 (one thread of 32 at twice the error: + 4.6 %) and max_rel sees it no
better.  measure therefore also reduces every result per class of every map of oracle/output_classes.py -- the digits of the
output index (one for paths 0 and 2; K1, K2, K3 for paths 1 and 7) in windows of 8 bits, the arithmetic thread and the half
of k_chunk, the workgroup slot of k_small32 -- each class of >= 1024 samples, and check_classes holds every class to
  (a) pin: rel_l2 <= PIN_REL_L2 x the recorded worst class of its map (CLASSES_RECORD_PATH, written from the same execs
      under the same stamp), and
  (b) cap: rel_l2 <= CLASS_FACTOR x cap(n); CLASS_FACTOR = 1.50 comes from a complex64 model on the CPU, not from the GPU
      (output_classes.py has the derivation; tests/test_output_classes.py repeats it and shows that one class at twice its
      error passes the whole-buffer rule and fails here by name).
Recorded: every class of every map within 0.66-1.36 of its row's rel_l2 (both ends in K1 of the 256 x 256 plan tile_2^16x4;
the model: 0.70-1.36), the slot and half maps within 0.99-1.01; the worst class sits at 1.108 of cap(n): class 255 of
'K2 high 8 bits' (K2 = 510, 511 of the 512-point middle pass) of mid_tile_9_2^21x2/Forward (64 x 512 x 64), 1.30 x that
row's 0.851; no class stands out of its map's spread, and the check found no defect.

The worst max_rel sits
at 0.63 of MAX_REL_CAP_FACTOR x cap (k_chunk at n = 32: 1.66 x cap(32)).  For scale: a numpy fp32 radix-2 FFT with
f32-rounded f64 twiddles sits at 0.55-0.58 of the cap (log2 n = 10..20), the same FFT with its twiddle angle evaluated
in f32 at 1.12-1.58 (tests/test_error_budget.py); the flat 1e-5 sees neither.

Which tiled rows there are is a rule, not a choice.  resolve_tiled (fft_wgpu_amd/csrc/schedule.h) picks the kernel of every
pass from the length, the "factors" key, the flag keys "colsw" / "rows32" / "p1_gen" / "tile_ring" and the pass position;
oracle/kernel_cells.py reads every such decision from tests/golden/tiled_schedule.txt and names its *cells*: pass A
(kernel, log2 length, ring width), pass B (k_tile columns, log2 length), pass C (k_rows32, log2 length, ring width 0 / 32 / 64)
or (k_tile rows, log2 length, two or three passes) -- 35 over 2^16 .. 2^28, each its own template instantiation per direction
or its own branch on the slab layout or the pass count.  tests/test_kernel_cells.py demands that every cell is run by a row
here in each of the three plan kinds, and that a tiled row's `kernels` text names the kernels its cells give.  The rows
from _cell_row are the cells the hand-picked rows left out, each at the smallest (log2 n, factors, flag setting) that
reaches it; they set "factors" and all four flags themselves, and device_run.run reads every key back.

Out of the matrix on purpose: the 2^27..2^30 impulse test (tests/test_gpu_parity.py) keeps the flat bound; at those
sizes a one-index twiddle error rotates by 2 pi / N <= 5e-8, below fp32 resolution, and a dense fp64 reference costs O(n)
host work per output.  What only a transform of >= 4 GiB (n >= 2^29) tells apart -- the 64-bit-pointer form of k_tile (a
tile spanning 2^32 bytes) and the four buffer descriptors of k_p1_gen, one per quarter of a transform, which below that
size address what a single one would -- and the 2^19 .. 2^20-entry hi[] tables of those sizes are held by
oracle/large_plans.py instead: sparse inputs (swept impulses and combs) through every accepted factorisation of 2^29 and
2^30 in every plan kind, each compared output within pi / 2^20 of an exact float64 reference, the combs within this flat
bound.
"""
import hashlib
import json
import os

import numpy as np

from . import output_classes as oc
from .device_run import blocks, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_PATH = os.path.join(ROOT, "tests", "golden", "error_budget.json")
CLASSES_RECORD_PATH = os.path.join(ROOT, "tests", "golden", "error_budget_classes.json")
KERNEL_SOURCE_DIR = "fft_wgpu_amd/csrc"

C = 1.05
PIN_REL_L2 = 1.25
PIN_MAX_REL = 1.5
MAX_REL_CAP_FACTOR = 2.5
MIN_SAMPLES = 1 << 18
PATH_TILED = 7

KINDS = (("Forward", -1), ("Inverse", 1), ("Onlyinverse", 1))


def _f(*lg):
    """packed "factors" key: log2 N1 | log2 N2 << 8 | log2 N3 << 16."""
    return sum(v << (8 * i) for i, v in enumerate(lg))


def _samples(n, batch=1):
    return max(batch, -(-MIN_SAMPLES // n))


def _cell_row(name, lg, factors, flag_index, kernels):
    """A tiled row that sets "factors" and all four flag keys itself (flag_index: bit 0 colsw, 1 rows32, 2 p1_gen, 3 tile_ring, as
    schedule.h flag_setting), on at least two transforms so that the per-transform stride of every pass is exercised."""
    n = 1 << lg
    batch = _samples(n, 2)
    tun = {"factors": _f(*factors)}
    tun.update({key: flag_index >> i & 1 for i, key in enumerate(("colsw", "rows32", "p1_gen", "tile_ring"))})
    return ("%sx%d" % (name, batch), n, batch, tun, (PATH_TILED, _f(*factors), len(factors)), kernels)


# (id, n, batch, tunables, (path, factors, launches_per_exec), kernels).  Path 0: one launch (k_chunk up to 256, then
# k_small32<log2 n>); 1: the 2^20 two-pass pipeline; 2: the literal radix-2 recurrence, one launch per stage;
# 7: tiled (pass A columns, [pass B columns], pass C rows).
_CASES = (
    [("chunk_%d" % (1 << lg), 1 << lg, _samples(1 << lg), {}, (0, lg, 1), "k_chunk") for lg in range(1, 9)]
    + [("small32_%d" % lg, 1 << lg, _samples(1 << lg), {}, (0, lg, 1), "k_small32<%d>" % lg) for lg in range(9, 16)]
    + [
        ("literal_2^10", 1 << 10, 256, {"path": 2}, (2, 10, 10), "k_r2_stage x 10 (the reference recurrence)"),
        ("literal_2^20", 1 << 20, 1, {"path": 2}, (2, _f(6, 6, 8), 20), "k_r2_stage x 20 (the reference recurrence)"),
        ("pipeline_2^20x4", 1 << 20, 4, {}, (1, _f(10, 10), 2), "k_p1_1m + k_p2_1m"),
        ("threepass_2^20x1", 1 << 20, 1, {}, (7, _f(6, 6, 8), 3), "k_tile x 3 (64 x 64 x 256)"),
        ("tile_2^16x4", 1 << 16, 4, {}, (7, _f(8, 8), 2), "latency regime: k_tile columns + k_tile rows"),
        ("colsw_8_2^17x9", 1 << 17, 9, {}, (7, _f(8, 9), 2), "k_colsw<8,64> + k_rows32<9> (matrix layout: no tile ring for 512-point rows)"),
        ("colsw_9_2^19x3", 1 << 19, 3, {}, (7, _f(9, 10), 2), "k_colsw<9,32> + k_rows32<10> (tile ring)"),
        ("colsw0_2^19x3", 1 << 19, 3, {"colsw": 0}, (7, _f(9, 10), 2), "k_tile columns + k_rows32<10>"),
        ("colsw0_rows32_0_2^19x3", 1 << 19, 3, {"colsw": 0, "rows32": 0}, (7, _f(9, 10), 2),
         "k_tile columns + k_tile rows"),
        ("p1_gen_2^21x2", 1 << 21, 2, {}, (7, _f(10, 11), 2), "k_p1_gen + k_rows32<11>"),
        ("p1_gen0_2^21x2", 1 << 21, 2, {"p1_gen": 0}, (7, _f(10, 11), 2), "k_tile columns + k_rows32<11>"),
        ("p1_gen_2^22x2", 1 << 22, 2, {}, (7, _f(10, 12), 2), "k_p1_gen + k_rows32<12>"),
        ("cols32_2^23x1", 1 << 23, 1, {}, (7, _f(11, 12), 2), "k_cols32<11> + k_rows32<12>"),
        ("factors_9_9_2^18x1", 1 << 18, 1, {"factors": _f(9, 9)}, (7, _f(9, 9), 2), "k_tile columns + k_rows32<9>"),
        ("factors_6_6_6_2^18x1", 1 << 18, 1, {"factors": _f(6, 6, 6)}, (7, _f(6, 6, 6), 3), "k_tile x 3"),
        ("factors_10_10_2^20x1", 1 << 20, 1, {"factors": _f(10, 10)}, (7, _f(10, 10), 2), "k_p1_gen + k_rows32<10>"),
        ("factors_10_10_rows32_0_2^20x1", 1 << 20, 1, {"factors": _f(10, 10), "rows32": 0}, (7, _f(10, 10), 2),
         "k_p1_gen + k_tile rows"),
        ("factors_7_7_6_2^20x1", 1 << 20, 1, {"factors": _f(7, 7, 6)}, (7, _f(7, 7, 6), 3), "k_tile x 3"),
        ("tiled_2^24x1", 1 << 24, 1, {}, (7, _f(9, 7, 8), 3), "k_colsw<9,32> + k_tile columns + k_tile rows"),
        ("tiled_2^25x1", 1 << 25, 1, {}, (7, _f(9, 8, 8), 3), "k_colsw<9,32> + k_tile columns + k_tile rows"),
        ("tiled_2^26x1", 1 << 26, 1, {}, (7, _f(9, 8, 9), 3), "k_colsw<9,32> + k_tile columns + k_tile rows"),
    ]
    # the cells (oracle/kernel_cells.py) no row above runs, each at the smallest (log2 n, factors, flag setting) that reaches it
    + [_cell_row(*r) for r in (
        ("rows_tile_9_2^16", 16, (7, 9), 0, "k_tile columns + k_tile rows (512 points, two passes)"),
        ("rows_tile_7_2^16", 16, (9, 7), 0, "k_tile columns + k_tile rows (128 points, two passes)"),
        ("rows_tile_6_2^16", 16, (10, 6), 0, "k_tile columns + k_tile rows (64 points, two passes)"),
        ("rows_tile_7_three_2^19", 19, (6, 6, 7), 0, "k_tile columns x 2 + k_tile rows (128 points, three passes)"),
        ("ring64_2048_2^19", 19, (8, 11), 9, "k_colsw<8,64> + k_rows32<11> (tile ring 64)"),
        ("ring64_4096_2^20", 20, (8, 12), 9, "k_colsw<8,64> + k_rows32<12> (tile ring 64)"),
        ("ring32_2048_2^20", 20, (9, 11), 9, "k_colsw<9,32> + k_rows32<11> (tile ring 32)"),
        ("mid_tile_9_2^21", 21, (6, 9, 6), 0, "k_tile columns x 2 (512-point middle pass) + k_tile rows"),
        ("ring32_4096_2^21", 21, (9, 12), 9, "k_colsw<9,32> + k_rows32<12> (tile ring 32)"),
        ("rows_tile_10_three_2^22", 22, (6, 6, 10), 0, "k_tile columns x 2 + k_tile rows (1024 points, three passes)"),
        ("mid_tile_10_2^22", 22, (6, 10, 6), 0, "k_tile columns x 2 (1024-point middle pass) + k_tile rows"),
    )]
)

pack_factors, samples = _f, _samples      # the public names, for the modules that build rows of their own


def case_row(name):
    """The row `name` of _CASES by field, for modules that derive rows from it (oracle/special_values.py): a change of the
    tuple's shape is then made here once."""
    cid, n, batch, tunables, (path, factors, passes), kernels = next(c for c in _CASES if c[0] == name)
    return dict(case=cid, n=n, batch=batch, tunables=dict(tunables), path=path, factors=factors, passes=passes, kernels=kernels)


# every case in each of the three transforming plan kinds; id "<case>/<kind>"
MATRIX = [dict(id="%s/%s" % (c[0], kind), case=c[0], kind=kind, direction=direction, n=c[1], batch=c[2],
               tunables=c[3], path=c[4][0], factors=c[4][1], launches_per_exec=c[4][2], kernels=c[5])
          for c in _CASES for kind, direction in KINDS]


def cap(n):
    return C * 2.0 ** -24 * np.sqrt(np.log2(n))


def metrics(y, r, n, classes=None):
    """(rel_l2 over the batch, worst per-transform max_rel) of complex64 `y` against complex128 `r`, over
    device_run.blocks.  classes: an output_classes.ClassSums, fed |y - r|^2 and |r|^2 of every block."""
    batch = np.size(y) // n
    maxd = np.zeros(batch)
    maxr = np.zeros(batch)
    sd = sr = 0.0
    at = (-1, 0)                                       # the transform and output index the next block starts at
    for t0, diff, rb in blocks(y, r, n):
        k0 = at[1] if t0 == at[0] else 0
        at = (t0, k0 + diff.shape[1])
        t = slice(t0, t0 + diff.shape[0])
        d, m = np.abs(diff), np.abs(rb)
        maxd[t] = np.maximum(maxd[t], d.max(axis=1))   # NaN-propagating
        maxr[t] = np.maximum(maxr[t], m.max(axis=1))
        np.multiply(d, d, out=d)
        np.multiply(m, m, out=m)
        sd += float(d.sum())
        sr += float(m.sum())
        if classes is not None:
            classes.add(t0, k0, d, m)
    rel_l2 = np.sqrt(sd / sr) if sr > 0 else np.sqrt(sd)
    return float(rel_l2), float(np.max(maxd / np.where(maxr > 0, maxr, 1.0)))


def check(case, got, rec):
    """The rule: a list of failure messages (empty = pass).  `got` and `rec` hold rel_l2 and max_rel; `rec` None =
    no record for this case, itself a failure."""
    cid, c = case["id"], cap(case["n"])
    bad = []
    if rec is None:
        return ["%s: no recorded entry in %s (run tools/record_error_budget.py)" % (cid, os.path.relpath(RECORD_PATH, ROOT))]
    for key, pin, top in (("rel_l2", PIN_REL_L2, c), ("max_rel", PIN_MAX_REL, MAX_REL_CAP_FACTOR * c)):
        v = got[key]
        if not v <= pin * rec[key]:
            bad.append("%s: %s %.4g > %.2f x recorded %.4g (cap %.4g)" % (cid, key, v, pin, rec[key], top))
        if not v <= top:
            bad.append("%s: %s %.4g above the cap %.4g (recorded %.4g)" % (cid, key, v, top, rec[key]))
    return bad


def check_classes(case, got, rec):
    """The rule per output class (oracle/output_classes.py): `got` {map: rel_l2 per class}, `rec` the case's entry of
    CLASSES_RECORD_PATH (None = no record, itself a failure).  Every class must sit at or below PIN_REL_L2 x the recorded
    worst class of its map and at or below CLASS_FACTOR x cap(n).  The first 8 failures are kept."""
    cid, c = case["id"], cap(case["n"])
    where = "%s [%s]" % (cid, case["kernels"])
    if rec is None:
        return ["%s: no recorded entry in %s (run tools/record_error_budget.py)" % (cid, os.path.relpath(CLASSES_RECORD_PATH, ROOT))]
    bad = []
    if set(got) != set(rec["class_maps"]):
        bad.append("%s: class maps %s, the record holds %s" % (where, sorted(got), sorted(rec["class_maps"])))
    top = oc.CLASS_FACTOR * c
    for name, e in got.items():
        worst = rec["class_maps"].get(name, (0.0, 0.0))[1] * c
        for k in np.flatnonzero(~((e <= PIN_REL_L2 * worst) & (e <= top))):
            if e[k] <= top:
                bad.append("%s, class %d of '%s': rel_l2 %.4g > %.2f x the recorded worst class %.4g (cap %.2f x %.4g)"
                           % (where, k, name, e[k], PIN_REL_L2, worst, oc.CLASS_FACTOR, c))
            else:
                bad.append("%s, class %d of '%s': rel_l2 %.4g above the class cap %.2f x %.4g (recorded worst class %.4g)"
                           % (where, k, name, e[k], oc.CLASS_FACTOR, c, worst))
    return bad[:8]


def load_record(path=RECORD_PATH):
    with open(path) as f:
        return json.load(f)


def kernel_source_sha256(root=ROOT):
    """sha256 over the names and bytes of the kernel sources (build products excluded), in name order."""
    h = hashlib.sha256()
    d = os.path.join(root, KERNEL_SOURCE_DIR)
    for name in sorted(os.listdir(d)):
        if name.endswith((".o", ".so")) or not os.path.isfile(os.path.join(d, name)):
            continue
        h.update(name.encode() + b"\0")
        with open(os.path.join(d, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def measure(fw, dev, queue, cases=None, log=None):
    """Run `cases` (default MATRIX) -> {id: {rel_l2, max_rel, path, factors, launches_per_exec, classes}}, `classes` the
    rel_l2 of every output class of every map of the case (oracle/output_classes.py), reduced on the host from the same
    result.  The fp64 DFT of a (case, direction) is computed once and shared by Inverse and Onlyinverse."""
    import oracle
    cases = MATRIX if cases is None else cases
    out = {}
    memo = {}
    for case in cases:
        n, batch = case["n"], case["batch"]
        key = (n, batch, case["direction"])
        if key not in memo:
            memo.clear()
            x = oracle.gen_input(n, batch)
            memo[key] = (x, oracle.dft_f64(x, n, case["direction"]))
        x, r = memo[key]
        y, _, facts = run(fw, dev, queue, case["kind"], x, n, case["tunables"])
        rr = r / n if case["kind"] == "Inverse" else r
        sums = oc.ClassSums(case)
        rel_l2, max_rel = metrics(y, rr, n, sums)
        out[case["id"]] = dict(rel_l2=rel_l2, max_rel=max_rel, classes=sums.errors(), **facts)
        if log:
            log("%-44s rel_l2 %.3e (%.2f of cap)  max_rel %.3e  path %d factors %#x launches %d"
                % (case["id"], rel_l2, rel_l2 / cap(n), max_rel, facts["path"], facts["factors"],
                   facts["launches_per_exec"]))
    return out
