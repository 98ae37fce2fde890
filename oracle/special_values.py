"""NaN propagation, batch isolation and exact 2^s scaling of every kernel (TEST INFRASTRUCTURE ONLY, HIP-free).

Every accuracy test of the suite feeds the kernels dense uniform samples at scale 1 and compares a norm over a whole
transform.  Three exact properties of the transform see what no norm can, and need no tolerance:

  * completeness: every output of a DFT depends on every input, so one input sample with NaN in both parts makes all 2n
    output floats of its transform NaN, whatever the algorithm (both parts: trivial-twiddle shortcuts are covered too).
    A finite output never read that input.  A sample of +Inf - Inf i leaves no output finite in both parts; an all-zero
    transform gives zero (either sign).
  * batch isolation: 0 * NaN is NaN, so a lane that multiplies a neighbour's sample by zero, adds it at 1e-9 or reads it
    only in a ragged last group finds the NaN.  Every other transform of the batch keeps exactly the bits of the clean
    exec: the same batch and geometry with the special transforms replaced by generator data.
  * scaling: the kernels are built without fast-math and every twiddle is data-independent, so an input multiplied by
    2^s (exact in fp32) gives every output multiplied by 2^s, bit for bit, while nothing leaves the normal range.
    s = -40 is the benchmark's data (bench.py fills at 2^-40), +40 and +90 are amplitudes at which an intermediate that
    overflows before the result does would show.  An approximate reciprocal, an absolute threshold, a stray additive
    term or a flush breaks it.

Subnormal inputs and results are deliberately not asserted: the reference's WGSL may flush them, so no test may depend on
either behaviour.  The scales are chosen so that the restatement (oracle.forward_ref / inverse_ref / onlyinverse_ref)
meets every condition on these inputs; tests/test_special_values.py is the standing proof of that.

Rows: the non-tiled rows of error_budget._CASES named in NON_TILED, and one tiled row per distinct smallest shape of
kernel_cells.all_cells(), built as error_budget._cell_row builds its rows ("factors" and all four flag keys set by the row,
every key read back by device_run.run), so the kernel of every pass does not depend on the batch.  Every row runs
in Forward, Inverse and Onlyinverse.

Batch layout: transforms alternate clean / special, so every special transform has clean neighbours on both sides.
  n < 2^16   batch = error_budget.samples(n) rounded up to odd, at least 9: several workgroups, the last one ragged;
             specials at transforms 1, 3, 5 and at the last but one
  tiled      batch 7 with group = 2, streams = 2: a ragged last group, both chains used; specials at 1, 3, 5
  2^20       the two-pass pipeline at the same geometry
The specials are (a) generator data with sample p = NaN + NaN i, (b) the same with sample p = +Inf - Inf i, (c) all zero;
p moves from row to row and from special to special over {0, n - 1, one seeded interior index} ({0, 1} at n = 2); the
fourth special of the small rows repeats (a) at the interior index.

In that layout the ragged unit never holds a special.  Every one-launch kernel packs transforms_per_workgroup(n) =
8192 / n transforms into a workgroup (k_chunk: 8192 samples, kernels_chunk.hip CH; k_small32: XPW = 16 .. 1 for 2^9 ..
2^13, one transform from 2^14, small32_kernel.h), a power of two that divides samples(n): the last workgroup of a batch
of 2^k + 1 holds the clean last transform alone, and the special at the last but one closes the full workgroup before
it.  Likewise 7 transforms in groups of 2 leave the clean transform 6 alone in the last group.  A kernel that reads
across transforms only where its workgroup or group is partly valid would pass.  So every row also runs a *ragged
layout*, for the clean and the poisoned exec only (scaling does not depend on the geometry):
  n < 2^16   batch = samples(n) + 3: the last workgroup holds the last three transforms -- clean, (a), clean -- and is
             partly valid wherever a workgroup holds at least 4 transforms (n <= 2^11; from 2^12 on a workgroup holds
             one or two transforms and raggedness is moot)
  tiled, 2^20   batch 11 with group = 4, streams = 2: the last group holds transforms 8, 9, 10 of a group of 4 --
             clean, (a), clean
with specials at 1, 3, 5 as before.  tests/test_special_values.py computes for every row that the last special sits
inside the last, partly valid unit with a clean transform of the same unit on either side.

Per row and kind: the clean exec, the poisoned exec and three scaled execs, then the clean and the poisoned exec of the
ragged layout.  The fp64 DFT is never needed.
"""
import numpy as np

from . import error_budget as eb
from . import kernel_cells as kc
from .device_run import run

KINDS = eb.KINDS
SCALES = (-40, 40, 90)
SEED = 0x5EED
GROUP, STREAMS, TILED_BATCH = 2, 2, 7
RAGGED_GROUP, RAGGED_BATCH = 4, 11          # the ragged layout of the pipelined rows: groups {0..3} {4..7} {8, 9, 10}
NON_TILED = (["chunk_%d" % (1 << lg) for lg in range(1, 9)] + ["small32_%d" % lg for lg in range(9, 16)]
             + ["literal_2^10", "pipeline_2^20x4"])
NAN, INF, ZERO = "nan", "inf", "zero"
# Normalize (k_scale): (n, batch); 701 workgroups of 8192 samples with 3 transforms in the last one, and an odd log2 n
NORMALIZE_ROWS = ((64, 700 * 128 + 3), (1 << 13, 9))


# ---- the batch layout -----------------------------------------------------------------------------------------------
def _positions(n, index):
    """{0, n - 1, one seeded interior index} of row number `index`; {0, 1} at n = 2."""
    if n == 2:
        return (0, 1)
    return (0, n - 1, int(np.random.default_rng(SEED + index).integers(1, n - 1)))


def make_layout(n, batch, index, small):
    """{n, batch, specials: ((transform, NAN | INF | ZERO, sample index or None), ...)}"""
    pos = _positions(n, index)
    where = [1, 3, 5] + ([batch - 2] if small else [])
    what = [NAN, INF, ZERO] + ([NAN] if small else [])
    specials = []
    for j, (t, w) in enumerate(zip(where, what)):
        p = pos[(index + j) % len(pos)] if j < 3 else pos[-1]     # the fourth special: (a) again, at the interior index
        specials.append((t, w, None if w == ZERO else p))
    assert batch % 2 == 1 and len({t for t, _, _ in specials}) == len(specials) and all(0 < t < batch - 1 for t, _, _ in specials)
    return dict(n=n, batch=batch, specials=tuple(specials))


def _small_batch(n):
    return max(9, eb.samples(n) | 1)


def transforms_per_workgroup(n):
    """of the one-launch kernels (path 0): k_chunk takes 8192 samples per workgroup (kernels_chunk.hip CH), k_small32
    256 / (n / 32) transforms up to 2^13 and one from 2^14 (small32_kernel.h XPW)"""
    return max(1, 8192 // n)


def _row(case, n, batch, tunables, path, factors, passes, kernels, index, budget_row=None):
    """`tunables` without the geometry: the pipelined rows get group / streams here, per layout"""
    small = n < 1 << 16
    if small:
        geometry = ragged_geometry = {}
        groups = ragged_groups = 1
        ragged_batch = eb.samples(n) + 3
    else:
        geometry, ragged_geometry = dict(group=GROUP, streams=STREAMS), dict(group=RAGGED_GROUP, streams=STREAMS)
        groups, ragged_batch = -(-batch // GROUP), RAGGED_BATCH
        ragged_groups = -(-ragged_batch // RAGGED_GROUP)
    ragged = dict(batch=ragged_batch, tunables=dict(tunables, **ragged_geometry), launches_per_exec=passes * ragged_groups,
                  layout=make_layout(n, ragged_batch, index, True))
    return dict(case=case, n=n, batch=batch, tunables=dict(tunables, **geometry), path=path, factors=factors,
                launches_per_exec=passes * groups, kernels=kernels, budget_row=budget_row,
                layout=make_layout(n, batch, index, small), ragged=ragged)


def _rows():
    rows = []
    for name in NON_TILED:
        c = eb.case_row(name)
        n = c["n"]
        if n < 1 << 16:
            rows.append(_row(name, n, _small_batch(n), c["tunables"], c["path"], c["factors"], c["passes"], c["kernels"], len(rows), name))
        else:
            assert c["path"] == 1
            rows.append(_row("pipeline_2^20x%d" % TILED_BATCH, n, TILED_BATCH, c["tunables"], c["path"], c["factors"], c["passes"],
                             c["kernels"], len(rows), name))
    cells = kc.all_cells()
    for lg, factors, flags in sorted(set(cells.values())):
        reached = [c for c in kc.cells_of(lg, factors, flags) if cells[c] == (lg, factors, flags)]
        tun = {"factors": eb.pack_factors(*factors)}
        tun.update({key: flags >> i & 1 for i, key in enumerate(kc.FLAG_KEYS)})
        name = "cells_2^%d_%s_f%d" % (lg, "x".join(str(f) for f in factors), flags)
        kernels = " + ".join(kc.kernel_text(c) for c in kc.cells_of(lg, factors, flags))
        rows.append(_row(name, 1 << lg, TILED_BATCH, tun, kc.PATH_TILED, eb.pack_factors(*factors), len(factors),
                         "%s (smallest shape of: %s)" % (kernels, "; ".join(kc.describe(c) for c in reached)), len(rows)))
    return rows


def ragged_case(case):
    """The case of MATRIX on its row's ragged layout: same kernels, another batch and (pipelined rows) group size."""
    r = case["ragged"]
    return dict(case, id=case["id"] + "/ragged", batch=r["batch"], tunables=r["tunables"],
                launches_per_exec=r["launches_per_exec"], layout=r["layout"])


ROWS = _rows()
# every row in each of the three transforming plan kinds; id "<row>/<kind>".  The dicts carry what device_run.run
# and kernel_cells.cells_of_case read.
MATRIX = [dict(r, id="%s/%s" % (r["case"], kind), kind=kind, direction=direction) for r in ROWS for kind, direction in KINDS]


# ---- the inputs -----------------------------------------------------------------------------------------------------
def poison_value(what):
    return {NAN: np.complex64(complex(np.nan, np.nan)), INF: np.complex64(complex(np.inf, -np.inf))}[what]


def clean_input(oracle, layout):
    return oracle.gen_input(layout["n"], layout["batch"])


def poisoned_input(x_clean, layout):
    n = layout["n"]
    x = x_clean.copy()
    for t, what, p in layout["specials"]:
        if what == ZERO:
            x[t * n:(t + 1) * n] = 0
        else:
            x[t * n + p] = poison_value(what)
    return x


def scaling_input(x_clean, layout):
    """The unscaled input of the scaled execs: the clean batch with the zero transform in place."""
    n = layout["n"]
    x = x_clean.copy()
    for t, what, _ in layout["specials"]:
        if what == ZERO:
            x[t * n:(t + 1) * n] = 0
    return x


def scaled(x, s):
    """x * 2^s, exact in fp32 while nothing leaves the normal range."""
    f = np.float32(2.0 ** s)
    assert f > 0 and np.isfinite(f)
    return (x.view(np.float32) * f).view(np.complex64)


def scaling_reference(y_clean, y_poison, layout):
    """The unscaled result the scaled execs are compared with, from execs that did run: the clean exec's, with the zero
    transform's result taken from the poisoned exec (check_poison has held every other transform of the two to the same
    bits, and the zero transform to zero)."""
    n = layout["n"]
    y = y_clean.copy()
    for t, what, _ in layout["specials"]:
        if what == ZERO:
            y[t * n:(t + 1) * n] = y_poison[t * n:(t + 1) * n]
    return y


# ---- the checks: arrays in, messages out ----------------------------------------------------------------------------
def _f32(y, n):
    return np.ascontiguousarray(y, dtype=np.complex64).view(np.float32).reshape(-1, 2 * n)


def _u32(y, n):
    return np.ascontiguousarray(y, dtype=np.complex64).view(np.uint32).reshape(-1, 2 * n)


def check_poison(y, y_clean, layout):
    """`y`: result of the poisoned batch, `y_clean`: of the clean one (same batch and geometry) -> failure messages."""
    n, batch = layout["n"], layout["batch"]
    bad = []
    if np.size(y) != n * batch or np.size(y_clean) != n * batch:
        return ["result sizes %d / %d, the layout has %d x %d" % (np.size(y), np.size(y_clean), n, batch)]
    f, u, uc = _f32(y, n), _u32(y, n), _u32(y_clean, n)
    special = {}
    for t, what, p in layout["specials"]:
        special[t] = what
        row = f[t]
        if what == NAN:
            k = np.flatnonzero(~np.isnan(row))
            if k.size:
                bad.append("transform %d (NaN + NaN i at sample %d): %d of %d output floats are not NaN, first at output %d (%s): "
                           "that output never read the input" % (t, p, k.size, 2 * n, k[0] // 2, "im" if k[0] & 1 else "re"))
        elif what == INF:
            k = np.flatnonzero(np.isfinite(row[0::2]) & np.isfinite(row[1::2]))
            if k.size:
                bad.append("transform %d (+Inf - Inf i at sample %d): %d of %d outputs are finite in both parts, first at output %d"
                           % (t, p, k.size, n, k[0]))
        else:
            k = np.flatnonzero(~(row == 0))
            if k.size:
                bad.append("transform %d (all zero): %d output floats are not 0, first at output %d: %r" % (t, k.size, k[0] // 2, row[k[0]]))
    for t in range(batch):
        if t in special:
            continue
        k = np.flatnonzero(u[t] != uc[t])
        if k.size:
            near = [s for s in (t - 1, t + 1) if s in special]
            bad.append("clean transform %d (neighbours %s): %d floats differ from the clean exec, first at output %d: %r, clean %r"
                       % (t, ", ".join("%d %s" % (s, special[s]) for s in near) or "clean", k.size, k[0] // 2,
                          f[t][k[0]], _f32(y_clean, n)[t][k[0]]))
    if not np.isfinite(_f32(y_clean, n)).all():
        bad.append("the clean exec itself is not finite")
    return bad


def check_scaling(y_s, y_1, s):
    """`y_s`: result of the input times 2^s, `y_1`: of the input itself -> failure messages."""
    ys = np.ascontiguousarray(y_s, dtype=np.complex64).view(np.float32)
    y1 = np.ascontiguousarray(y_1, dtype=np.complex64).view(np.float32)
    if ys.size != y1.size:
        return ["2^%d: result sizes %d / %d" % (s, ys.size, y1.size)]
    bad = []
    k = np.flatnonzero(~np.isfinite(ys))
    if k.size:
        bad.append("2^%d: %d floats are not finite, first at float %d: %r" % (s, k.size, k[0], ys[k[0]]))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = y1 * np.float32(2.0 ** s)
    k = np.flatnonzero(ys.view(np.uint32) != want.view(np.uint32))
    if k.size:
        bad.append("2^%d: %d of %d floats differ from 2^%d x the unscaled result, first at float %d: %r, wanted %r"
                   % (s, k.size, ys.size, s, k[0], ys[k[0]], want[k[0]]))
    return bad


# ---- Normalize: elementwise, so the pattern of the output is the pattern of the input --------------------------------
def normalize_input(oracle, n, batch):
    """Generator data with a zero transform and NaN / Inf in one or both parts of distinct samples (normalize_spots)."""
    x = oracle.gen_input(n, batch, first_transform=5)
    x[2 * n:3 * n] = 0
    f = x.view(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    vals = [(nan, nan), (inf, -inf), (nan, None), (None, nan), (-inf, None), (None, inf), (nan, inf), (inf, inf), (None, -inf),
            (nan, nan), (-inf, nan)]
    for i, (re, im) in zip(normalize_spots(n, batch), vals):
        if re is not None:
            f[2 * i] = re
        if im is not None:
            f[2 * i + 1] = im
    return x


def normalize_spots(n, batch):
    """The distinct samples that get a NaN / Inf: both ends of the first transform and the start of the second, both sides
    of the first seam between k_scale's 8192-sample workgroups, mid-buffer, the end of the last but two transform and
    the start and the last two samples of the last one (at 64 x 89603 inside the ragged last workgroup).  At n = 2^13 a
    workgroup is one transform: the seam is the transform boundary, two spots coincide with it and nine remain."""
    total = n * batch
    spots = [0, 1, n - 1, n, 8191, 8192, total // 2 + 1, total - 2 * n - 1, total - n, total - 2, total - 1]
    return list(dict.fromkeys(spots))


def normalize_scaling_input(x):
    """The unscaled input of Normalize's scaled execs: `x` with every non-finite float replaced by 0.25."""
    f = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    return np.where(np.isfinite(f), f, np.float32(0.25)).view(np.complex64)


def check_normalize(y, x, y_ref):
    """`y`: the kernel's result on `x`, `y_ref`: oracle.normalize_ref(x, n) -> failure messages."""
    fy = np.ascontiguousarray(y, dtype=np.complex64).view(np.float32)
    fx = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    fr = np.ascontiguousarray(y_ref, dtype=np.complex64).view(np.float32)
    if not fy.size == fx.size == fr.size:
        return ["sizes %d / %d / %d" % (fy.size, fx.size, fr.size)]
    bad = []
    k = np.flatnonzero(np.isnan(fy) != np.isnan(fx))
    if k.size:
        bad.append("NaN pattern differs from the input's at %d floats, first at sample %d" % (k.size, k[0] // 2))
    k = np.flatnonzero((np.isposinf(fy) != np.isposinf(fx)) | (np.isneginf(fy) != np.isneginf(fx)))
    if k.size:
        bad.append("Inf pattern differs from the input's at %d floats, first at sample %d" % (k.size, k[0] // 2))
    k = np.flatnonzero(np.isfinite(fx) & (fy.view(np.uint32) != fr.view(np.uint32)))
    if k.size:
        bad.append("%d finite floats differ from normalize_ref, first at sample %d: %r, wanted %r" % (k.size, k[0] // 2, fy[k[0]], fr[k[0]]))
    return bad


# ---- running a row --------------------------------------------------------------------------------------------------
def check_results(layout, y_clean, y_poison, y_scaled):
    """All checks of one (row, kind) from its five results; y_scaled: {s: result}."""
    bad = check_poison(y_poison, y_clean, layout)
    y_1 = scaling_reference(y_clean, y_poison, layout)
    for s in SCALES:
        bad += check_scaling(y_scaled[s], y_1, s)
    return bad


def run_row_kind(fw, dev, queue, oracle, case):
    """The five execs of one case of MATRIX through the C ABI (device_run.run), then the clean and the poisoned exec
    of its ragged layout -> (messages, plan facts, plan facts of the ragged layout)."""
    def one(c, x):
        y, _, facts = run(fw, dev, queue, c["kind"], x, c["n"], c["tunables"])
        return y, facts
    layout = case["layout"]
    x = clean_input(oracle, layout)
    y_clean, facts = one(case, x)
    y_poison, facts_p = one(case, poisoned_input(x, layout))
    xs = scaling_input(x, layout)
    y_scaled = {s: one(case, scaled(xs, s))[0] for s in SCALES}
    bad = ["%s: %s" % (case["id"], m) for m in check_results(layout, y_clean, y_poison, y_scaled)]
    if facts_p != facts:
        bad.append("%s: plan facts differ between the clean and the poisoned exec: %s / %s" % (case["id"], facts, facts_p))
    rc = ragged_case(case)
    x = clean_input(oracle, rc["layout"])
    y_clean, facts_r = one(rc, x)
    y_poison, facts_p = one(rc, poisoned_input(x, rc["layout"]))
    bad += ["%s: %s" % (rc["id"], m) for m in check_poison(y_poison, y_clean, rc["layout"])]
    if facts_p != facts_r:
        bad.append("%s: plan facts differ between the clean and the poisoned exec: %s / %s" % (rc["id"], facts_r, facts_p))
    return bad, facts, facts_r


def run_normalize(fw, dev, queue, oracle, n, batch):
    """Normalize on normalize_input and at the three scales -> messages."""
    even = (n.bit_length() - 1) % 2 == 0                      # processor.rs:433-439: reads buffer1 if log2 n is even

    def one(x):
        y, where, _ = run(fw, dev, queue, "Normalize", x, n, fill=lambda a, b: queue.write_buffer(a if even else b, 0, x))
        return y, where == ("src2" if even else "src")
    x = normalize_input(oracle, n, batch)
    y, ok = one(x)
    bad = check_normalize(y, x, oracle.normalize_ref(x, n))
    if not ok:
        bad.append("the result is not in the other buffer")
    xs = normalize_scaling_input(x)
    y_1 = one(xs)[0]
    bad += check_normalize(y_1, xs, oracle.normalize_ref(xs, n))
    for s in SCALES:
        bad += check_scaling(one(scaled(xs, s))[0], y_1, s)
    return ["normalize %d x %d: %s" % (n, batch, m) for m in bad]
