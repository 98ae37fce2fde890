"""The 2^28 .. 2^30 plans against an fp64 DFT on sparse inputs: swept impulses and combs (TEST INFRASTRUCTURE ONLY; HIP-free
apart from run_case, in the style of oracle/impulse_sweep.py, whose planned / execute / check / PIN / CAP / _rng it reuses).

The three largest sizes run code no smaller size runs.  launch_tile (fft_wgpu_amd/csrc/kernels_tiled.hip) takes the
64-bit-pointer form of k_tile (BUF = false) when a tile spans 2^32 bytes: pass A as k_tile columns (span 8 n + 128) and the
last pass as k_tile rows (out_stride N1 N2, span 8 n + 128), both from n = 2^29; the middle pass (pitch N3) keeps the
descriptor form.  k_p1_gen splits a transform over four buffer descriptors, one per quarter, which below 4 GiB address what
one would; at 2^30 its pitch is the launcher's limit 2^20 and its exponents reach 2^30.  The two-level twiddle tables
hi[e >> 10] lo[e & 1023] have 2^19 .. 2^20 hi entries for pass A and 512 .. 1024 for the middle pass (tw_hi_b), where the rows
of impulse_sweep stop at 64.  k_colsw<9,32> at 2^28 sits at its limit: byte offsets up to 2^31.  A dense input has no
reference at these sizes in seconds; a sparse one has an exact O(M) reference per compared output.

Rows (ROWS): batch 1, "factors" and where it decides anything "p1_gen" (at 2^28 "colsw") set by the row and read back by
planned.  At 2^29 and 2^30 they are exactly the factor tuples the "factors" key accepts (tests/golden/tiled_schedule.txt), with
every pass-A kernel the golden gives at each size (k_tile columns at 512 and 1024 points, k_p1_gen):
  colsw_2^28     9,9,10    colsw 1    k_colsw<9,32> with byte offsets up to 2^31
  p1gen_2^29     10,9,10   p1_gen 1   four live descriptors at pitch 2^19; k_tile rows<10> in pointer form
  tilec10_2^29   10,9,10   p1_gen 0   k_tile columns<10> in pointer form
  tilec9_2^29    9,10,10              k_tile columns<9> in pointer form
  tiler9_2^29    10,10,9   p1_gen 1   k_tile rows<9> in pointer form
  p1gen_2^30     10,10,10  p1_gen 1   pitch 2^20, exponents up to 2^30, 2^20 hi entries
  tilec10_2^30   10,10,10  p1_gen 0   k_tile columns<10> in pointer form at the largest size
each in Forward, Inverse and Onlyinverse (the Inverse and Onlyinverse plans are configured like the Forward one, so the
inverse pointer-form column kernel runs), and batch2_2^29: p1gen_2^29, Forward, on a buffer of two transforms, 8 of the
row's impulses written into transform 1 only; the windows of transform 0 must come back exactly zero (the batch stride
b * in_sb beyond 4 GiB in both pointer-form kernels).  22 cases.

Impulse sweep of a case: T = 128 execs of one transform each (a row's "T"; no row needed fewer).  Before each exec the buffer
is zeroed on the device (fill_synthetic at scale 0), then one 8-byte impulse 1 + 0i is written at p_t = r_t + R a_t, R = n /
N1.  Residues r_t: one per stratum of R / T at a seeded offset, with 0, 1 and R - 1 forced (transforms 0, 1 and T - 1), so
the last digits r mod N3 include 0 and N3 - 1 and the middle digits r // N3 include 0 and N2 - 1.  Columns a_t: seeded in
[0, N1), T / 4 per quarter a // (N1 / 4) -- every descriptor of k_p1_gen is live equally often --, with a = 0 (transform 1)
and a = N1 - 1 (transform T - 1, so p = n - 1 is swept) forced.

Compared per exec: 34 windows of w = 2048 outputs -- the head [0, w), the tail [n - w, n) and one seeded w-aligned window in
each of 32 near-equal strata of [w, n - w) -- and only they are downloaded.  w >= N1, so every window holds every K1; the 34
windows are spread over K3, and the last pass stores at stride N1 N2, so they sample the pointer-form stores over the whole
span.  Reference: exp(-+2 pi i ((p k) mod n) / n) in float64 on the compared indices (p k < 2^60 fits int64); no n-entry
table is built anywhere (impulse_sweep.twiddle_table would be 16 GiB at 2^30).  The Inverse result is multiplied by n.

Rule: impulse_sweep.check unchanged -- worst |y - r| <= PIN x recorded and <= CAP = pi / 2^20 = 3.0e-6.  The cap is derived,
not measured: it is half the rotation 2 pi 1024 / n = 5.9e-6 that a hi index one off causes at 2^30 and a quarter of it at
2^29 (and far less than one of the middle pass's table, domain n / N1).  A lo index one off rotates by 2 pi / n <= 2.3e-8,
below fp32 resolution at these sizes, and is not claimed.  An fp32 model of the twiddle path (five table factors, the two
inter-pass ones as hi lo, multiplied with fp32 cmul; tests/test_large_plans.py) stays near 3.6e-7 = 0.12 x CAP; the kernels'
radix stages add to that.  A recorded worst above CAP is a finding to explain from the code, not a reason to move the cap.
What this holds is how the tables are indexed and the buffers addressed at these sizes -- an error there shows at every
residue of its range -- not every table entry: the kernels look W^(r K1) up as a product over partial digits of K1 (k_tile:
r t, r TPX, 4 r TPX, 8 r TPX; k_p1_gen: r q, 32 r k2), so T residues read under T (N1 / 16 + 35) of the n / 1024 hi entries,
1 - 2 %.

Combs of a case: four more execs with M <= 1024 non-zeros g_m (seeded complex64, re and im uniform in [-1, 1)), one 8-byte
upload each: two column combs (p = r + R a for all a < N1, at r = R - 1 and at a seeded r: pass A dense over the full span
and all four descriptors), one middle comb (all r2 < N2 at a seeded (a, r3), a in the top quarter) and one row comb (all r3 <
N3 at a seeded (a, r2), a in the top quarter).  Reference: sum_m g_m exp(-+2 pi i ((p_m k) mod n) / n) in float64, in chunks,
on head + tail + 6 seeded windows of 2048 = 2^14 outputs.  Metric: device_run.parity's max_rel and rel_l2 over the compared
outputs (the maximum of the reference is that over the compared ones).  Bound: REL_TOL, the flat bound oracle/error_budget.py
keeps for these sizes, and each figure pinned to error_budget.PIN_MAX_REL x recorded.

tools/record_large_plans.py writes RECORD_PATH, tests/test_gpu_large_plans.py applies the rules, tests/test_large_plans.py
computes every statement above from the functions here and shows that the errors this module exists for are rejected.
"""
import functools
import json
import os
import time

import numpy as np

from . import error_budget as eb
from . import impulse_sweep as im
from .device_run import execute, parity, planned
from .impulse_sweep import CAP, PIN

ROOT = eb.ROOT
RECORD_PATH = os.path.join(ROOT, "tests", "golden", "large_plans.json")

KINDS = eb.KINDS
REL_TOL = 1e-5                 # tests/conftest.py REL_TOL (tests/test_large_plans.py holds the two together)
PIN_COMB = eb.PIN_MAX_REL
T_IMPULSES = 128               # execs of the impulse sweep
W = 2048                       # outputs per window
STRATA = 32                    # seeded windows between head and tail, per impulse exec
COMB_STRATA = 6                # the same, per comb exec
COMBS = ("column_last", "column_seeded", "middle", "row")
BATCH2_IMPULSES = 8
HEADROOM_BYTES = 8 << 30
INDEX_BASE = 1000              # the rows' "index" for impulse_sweep._rng: apart from the rows there


# ---- the rows -------------------------------------------------------------------------------------------------------
def _row(i, case, lg, factors, flags, kernels):
    n = 1 << lg
    tun = {"factors": eb.pack_factors(*factors)}
    tun.update(flags)
    return dict(case=case, index=INDEX_BASE + i, n=n, lg=lg, path=eb.PATH_TILED, factors=tun["factors"], lg_factors=tuple(factors),
                lengths=tuple(1 << v for v in factors), R=n >> factors[0], tunables=tun, kernels=kernels, T=T_IMPULSES)


ROWS = [_row(i, *r) for i, r in enumerate((
    ("colsw_2^28", 28, (9, 9, 10), {"colsw": 1}, "k_colsw<9,32> + k_tile columns + k_tile rows"),
    ("p1gen_2^29", 29, (10, 9, 10), {"p1_gen": 1}, "k_p1_gen + k_tile columns + k_tile rows<10> (pointer form)"),
    ("tilec10_2^29", 29, (10, 9, 10), {"p1_gen": 0}, "k_tile columns<10> (pointer form) + k_tile columns + k_tile rows<10> (pointer form)"),
    ("tilec9_2^29", 29, (9, 10, 10), {}, "k_tile columns<9> (pointer form) + k_tile columns + k_tile rows<10> (pointer form)"),
    ("tiler9_2^29", 29, (10, 10, 9), {"p1_gen": 1}, "k_p1_gen + k_tile columns + k_tile rows<9> (pointer form)"),
    ("p1gen_2^30", 30, (10, 10, 10), {"p1_gen": 1}, "k_p1_gen (pitch 2^20) + k_tile columns + k_tile rows<10> (pointer form)"),
    ("tilec10_2^30", 30, (10, 10, 10), {"p1_gen": 0}, "k_tile columns<10> (pointer form) + k_tile columns + k_tile rows<10> (pointer form)"),
))]


def row_named(name):
    return next(r for r in ROWS if r["case"] == name)


def _cases():
    out = [dict(r, id="%s/%s" % (r["case"], kind), kind=kind, direction=direction, batch=1, only=None, combs=True)
           for r in ROWS for kind, direction in KINDS]
    r = row_named("p1gen_2^29")
    out.append(dict(r, id="batch2_2^29/Forward", kind="Forward", direction=-1, batch=2, only=batch2_transforms(r), combs=False))
    return out


def batch2_transforms(row):
    """the 8 impulses of the batch-2 case: the forced ones (0, 1, T - 1) and five spread between them"""
    T = row["T"]
    return sorted({0, 1, T - 1} | {T // 6 * j + 2 for j in range(1, BATCH2_IMPULSES - 2)})


# ---- positions ------------------------------------------------------------------------------------------------------
def residues(row):
    """r_t: one per stratum of R / T at a seeded offset; 0, 1 and R - 1 forced."""
    R, T = row["R"], row["T"]
    S = R // T
    r = np.arange(T, dtype=np.int64) * S + im._rng(row, 0).integers(0, S, T)
    r[0], r[1], r[-1] = 0, 1, R - 1
    return r


def columns(row):
    """a_t: seeded in [0, N1), T / 4 per quarter; a = 0 at transform 1 and a = N1 - 1 at transform T - 1."""
    N1, T = row["lengths"][0], row["T"]
    rng = im._rng(row, 3)
    rest = np.repeat(np.arange(4, dtype=np.int64), T // 4).tolist()
    rest.remove(0)
    rest.remove(3)
    quarter = np.empty(T, dtype=np.int64)
    quarter[1], quarter[-1] = 0, 3
    free = np.array([t for t in range(T) if t not in (1, T - 1)])
    quarter[free] = rng.permutation(np.array(rest, dtype=np.int64))
    a = quarter * (N1 // 4) + rng.integers(0, N1 // 4, T)
    a[1], a[-1] = 0, N1 - 1
    return a


def positions(row):
    """p_t = r_t + R a_t of every exec: int64, a pure function of the row."""
    return residues(row) + row["R"] * columns(row)


def _windows(row, stream, execs, strata):
    n = row["n"]
    B = n // W - 2                                    # the w-aligned windows between head and tail
    j = np.arange(strata + 1, dtype=np.int64)
    edge = 1 + j * B // strata
    mid = im._rng(row, stream).integers(edge[:-1], edge[1:], size=(execs, strata)) * W
    return np.concatenate([np.zeros((execs, 1), dtype=np.int64), mid, np.full((execs, 1), n - W, dtype=np.int64)], axis=1)


def window_starts(row):
    """(T, 34) first outputs of the compared windows of every impulse exec, ascending"""
    return _windows(row, 1, row["T"], STRATA)


def comb_window_starts(row):
    """(4, 8) the same for the comb execs"""
    return _windows(row, 2, len(COMBS), COMB_STRATA)


def window_indices(starts):
    """the output indices of one exec's windows, ascending"""
    return (np.asarray(starts, dtype=np.int64)[:, None] + np.arange(W, dtype=np.int64)).reshape(-1)


def compared_outputs(case):
    T = case["T"] if case["only"] is None else len(case["only"])
    return T * (STRATA + 2) * W + (len(COMBS) * (COMB_STRATA + 2) * W if case["combs"] else 0)


def combs(row):
    """[(name, positions int64, amplitudes complex64)] of the four comb execs: a pure function of the row."""
    N1, N2, N3 = row["lengths"]
    R = row["R"]
    rng = im._rng(row, 4)
    out = []
    for name in COMBS:
        top = int(rng.integers(3 * N1 // 4, N1))
        if name == "column_last":
            p = (R - 1) + R * np.arange(N1, dtype=np.int64)
        elif name == "column_seeded":
            p = int(rng.integers(1, R - 1)) + R * np.arange(N1, dtype=np.int64)
        elif name == "middle":
            p = R * top + N3 * np.arange(N2, dtype=np.int64) + int(rng.integers(0, N3))
        else:
            p = R * top + N3 * int(rng.integers(0, N2)) + np.arange(N3, dtype=np.int64)
        g = rng.uniform(-1.0, 1.0, (len(p), 2)).astype(np.float32)
        out.append((name, p, (g[:, 0] + 1j * g[:, 1]).astype(np.complex64)))
    return out


def device_bytes_needed(case):
    """the skip rule of test_large_single_transform_properties, on the buffer the case runs"""
    return 4 * case["batch"] * case["n"] * 8 + HEADROOM_BYTES


# ---- references -----------------------------------------------------------------------------------------------------
def _sign(kind):
    return -1.0 if kind == "Forward" else 1.0


def impulse_reference(p, ks, n, kind):
    """exp(-+2 pi i ((p k) mod n) / n) at the outputs `ks`, complex128; nothing of size n is allocated"""
    ph = ((int(p) * np.asarray(ks, dtype=np.int64)) % n).astype(np.float64) * (_sign(kind) * 2.0 * np.pi / n)
    return np.cos(ph) + 1j * np.sin(ph)


def comb_reference(pos, g, ks, n, kind, chunk=W):
    """sum_m g_m exp(-+2 pi i ((p_m k) mod n) / n) at the outputs `ks`, complex128, `chunk` outputs at a time"""
    pos = np.asarray(pos, dtype=np.int64)
    ks = np.asarray(ks, dtype=np.int64)
    g = np.asarray(g).astype(np.complex128)
    out = np.empty(len(ks), dtype=np.complex128)
    c = _sign(kind) * 2.0 * np.pi / n
    for k0 in range(0, len(ks), chunk):
        ph = ((pos[:, None] * ks[None, k0:k0 + chunk]) % n).astype(np.float64)
        ph *= c
        out[k0:k0 + chunk] = g @ np.cos(ph) + 1j * (g @ np.sin(ph))
    return out


@functools.lru_cache(maxsize=2)
def _comb_references(case_name, direction):
    """the four comb references of a row in one direction (shared by Inverse and Onlyinverse), read-only"""
    row = row_named(case_name)
    kind = "Forward" if direction < 0 else "Onlyinverse"
    out = []
    for (name, p, g), starts in zip(combs(row), comb_window_starts(row)):
        r = comb_reference(p, g, window_indices(starts), row["n"], kind)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


def comb_metrics(y, r):
    """device_run.parity over the compared outputs as one transform -> (max_rel, rel_l2)"""
    mx, l2 = parity(np.asarray(y, dtype=np.complex64), r, len(r))
    return float(mx[0]), float(l2[0])


# ---- the sweep ------------------------------------------------------------------------------------------------------
def _fetch_windows(fetch, base, starts):
    return np.concatenate([fetch(base + int(s), W) for s in starts])


def sweep(case, run_exec):
    """Drive one case: run_exec(pos, amps) executes one transform that is zero but for amps[m] at pos[m] (in the last
    transform of the buffer, the ones before it all zero) and returns fetch(first sample of the buffer, count) -> complex64
    of the result.  -> dict(worst, t, k, p, compared, combs=[dict(name, max_rel, rel_l2)], zero_failures)."""
    n, kind = case["n"], case["kind"]
    base = (case["batch"] - 1) * n
    scale = float(n) if kind == "Inverse" else 1.0
    pos, win = positions(case), window_starts(case)
    one = np.ones(1, dtype=np.complex64)
    best = dict(worst=-1.0, t=0, k=0, p=0, compared=0, combs=[], zero_failures=[])
    for t in (range(case["T"]) if case["only"] is None else case["only"]):
        fetch = run_exec(pos[t:t + 1], one)
        ks = window_indices(win[t])
        d = np.abs(_fetch_windows(fetch, base, win[t]).astype(np.complex128) * scale - impulse_reference(pos[t], ks, n, kind))
        i = int(np.argmax(d))                             # the first NaN where there is one
        if im._beats(float(d[i]), best["worst"]):
            best.update(worst=float(d[i]), t=int(t), k=int(ks[i]), p=int(pos[t]))
        best["compared"] += d.size
        for b in range(case["batch"] - 1):                # the transforms that hold no impulse
            best["zero_failures"] += zero_failures(_fetch_windows(fetch, b * n, win[t]), b, t)
    if case["combs"]:
        refs = _comb_references(case["case"], case["direction"])
        for (name, p, g), starts, r in zip(combs(case), comb_window_starts(case), refs):
            y = _fetch_windows(run_exec(p, g), base, starts)
            mx, l2 = comb_metrics(y * np.float32(scale), r)
            best["combs"].append(dict(name=name, max_rel=mx, rel_l2=l2))
            best["compared"] += y.size
    return best


def zero_failures(z, transform, t):
    """messages for the samples of a transform without input that did not come back exactly zero (+-0)"""
    z = np.asarray(z)
    bad = np.flatnonzero(~(z == 0))                       # a NaN is not zero
    return ["transform %d of exec %d: %d of %d compared outputs are not zero, the first %r" % (transform, t, len(bad), z.size, z[bad[0]])] if len(bad) else []


# ---- the rules ------------------------------------------------------------------------------------------------------
def check_comb(cid, got, rec):
    """A comb's two figures against REL_TOL and PIN_COMB x recorded -> failure messages."""
    bad = []
    for key in ("max_rel", "rel_l2"):
        v = got[key]
        if not v <= REL_TOL:
            bad.append("%s: comb %s: %s %.4g above %.4g (recorded %.4g)" % (cid, got["name"], key, v, REL_TOL, rec[key]))
        if not v <= PIN_COMB * rec[key]:
            bad.append("%s: comb %s: %s %.4g > %.2f x recorded %.4g" % (cid, got["name"], key, v, PIN_COMB, rec[key]))
    return bad


def check(case, got, rec):
    """A list of failure messages (empty = pass): impulse_sweep.check on the impulses, check_comb on every comb, and the
    transforms without input exactly zero.  `rec` None = no record for this case, itself a failure."""
    cid = case["id"]
    if rec is None:
        return ["%s: no recorded entry in %s (run tools/record_large_plans.py)" % (cid, os.path.relpath(RECORD_PATH, ROOT))]
    bad = im.check(case, got, rec) + list(got["zero_failures"])
    names = [c["name"] for c in got["combs"]]
    if names != [c["name"] for c in rec["combs"]] or names != (list(COMBS) if case["combs"] else []):
        return bad + ["%s: combs %s, recorded %s" % (cid, names, [c["name"] for c in rec["combs"]])]
    for g, r in zip(got["combs"], rec["combs"]):
        bad += check_comb(cid, g, r)
    return bad


def load_record(path=RECORD_PATH):
    with open(path) as f:
        return json.load(f)


MATRIX = _cases()


# ---- running a case on the device -----------------------------------------------------------------------------------
def run_case(fw, dev, queue, case):
    """One case through the C ABI -> sweep's dict plus path, factors, the tunables read back, T and the wall seconds."""
    n, batch = case["n"], case["batch"]
    base = (batch - 1) * n
    t0 = time.time()
    with planned(fw, dev, queue, case["kind"], n, batch * n * 8, case["tunables"]) as p:
        def run_exec(pos, amps):
            dev.fill_synthetic(p.src, n, scale=0.0, encoder=p.enc)
            for m, pm in enumerate(pos):
                queue.write_buffer(p.src, (base + int(pm)) * 8, amps[m:m + 1], encoder=p.enc)
            out, _ = execute(p)
            return lambda first, count: out.map_read(first * 8, count * 8, p.enc)

        got = sweep(case, run_exec)
        got.update(path=int(p.plan.get("path")), factors=int(p.plan.get("factors")), tunables=p.held, T=case["T"])
    got["seconds"] = round(time.time() - t0, 2)
    return got
