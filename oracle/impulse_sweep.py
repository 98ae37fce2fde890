"""Impulse sweeps: the DFT matrix read out of every kernel, per output (TEST INFRASTRUCTURE ONLY, HIP-free).

Every accuracy test of the suite feeds the kernels dense uniform samples and compares a norm over a whole transform
(oracle/error_budget.py), and the exact tests of oracle/special_values.py ask for no accuracy at all.  A norm catches a gross
error anywhere and a subtle error everywhere; it cannot catch a subtle error in few places: one entry of a twiddle table
one index off, the last hi[] entry of a two-level table wrong.  At n = 2^20 such an entry rotates one intermediate by
2 pi / n = 6.0e-6; spread over a row FFT of random data that moves max_rel by about 4e-9 and rel_l2 by nothing.

An impulse is the input that sees one twiddle at a time.  For x = delta_p every butterfly adds a zero, so output k is
purely the product of the twiddles on its path: exp(-+2 pi i p k / n), magnitude 1, no cancellation, fp32 noise of a few
1e-7 -- and a one-index rotation at 2^20 stands 10x above that noise, per output.  A batch of impulses is the DFT matrix
read back row by row.  For a multi-pass plan n = N1 N2 [N3] (pass A: N1-point columns at stride R = n / N1) the impulse at
p = r + R a meets the pass-A twiddle W_n^(K1 r) for every K1 = k mod N1, so sweeping r over all residues mod R touches every
entry of A[q][c] B[k2][c] (tables.cpp, tile_1m.h) and of hi[e >> 10] lo[e & 1023] (tile_body.h, kernels_cols32.hip,
kernels_p1_gen.hip); in a three-pass plan the middle pass meets W_R^(K2 r3) with r3 = r mod N3 the same way.

Rows: the 44 rows of special_values.ROWS (chunk_2 .. small32_15, literal_2^10, the 2^20 pipeline, one tiled row per smallest
shape of every kernel cell, n <= 2^22) with their "factors" and four flag keys, so the kernel of every pass is reached by
construction; the geometry keys "group" / "streams" are dropped -- the plan's defaults apply, the sweep is about
arithmetic.  Every row runs in Forward, Inverse and Onlyinverse; run_case reads back path, factors and every key it set.

Sweep of a row: R = n for the one-launch and the literal rows, n / N1 for the pipelined ones; T = min(R, 4096) transforms,
transform t all zero but for 1 + 0i at p_t (positions(row): one seed, a pure function of the row).  What each row covers
completely and what it samples:
  chunk_2 .. small32_12, literal_2^10   (n <= 4096)        p_t = t: the whole DFT matrix, every input and every output
  small32_13                            (n = 2^13)         4096 of 8192 inputs, one per stratum of 2 at a seeded offset;
                                                           every output of each
  small32_14, small32_15                                   4096 inputs, one per stratum of 4 / 8; outputs sampled (below)
  pipeline_2^20 and every two-pass row  (R = 64 .. 4096)   every residue r_t = t, at p_t = r_t + R a_t with a_t seeded in
                                                           [0, N1): every pass-A twiddle entry at every K1; the column index
                                                           a and (from T n > 2^25) the outputs are sampled
  cells_2^18_6x6x6                      (R = 4096)         the same: every residue, so every (middle digit, last digit)
  the other three-pass rows             (R = 2^13 .. 2^16) 4096 residues, one per stratum of S = R / 4096 = 2 .. 16, among
                                                           them 0, 1 and R - 1; the offsets inside the strata are laid out
                                                           so that every last digit r mod N3 (every entry of the middle
                                                           pass's twiddle column) and every middle digit r // N3 occurs; of
                                                           the N2 N3 pairs one in S is present
tests/test_impulse_sweep.py computes each of these statements from positions(row).

Execution: chunks of at most 2^30 samples (8 GiB) per exec -- T n reaches 2^34 at 2^22 --, never fewer than 4 transforms
in the buffer (at n = 2 the two further ones stay zero and must come back zero).  The plan is created once per (row,
kind) on a buffer of the chunk size; before each exec the buffer is zeroed on the device (fill_synthetic at scale 0 gives
+-0, as good: adding either zero to a non-zero is exact), then the impulses are written, one 8-byte upload each,
stream-ordered.

What is compared: at most 2^25 outputs per (row, kind), which keeps the host side to seconds.  Where T n <= 2^25 every
output; otherwise per transform the head [0, w), the tail [n - w, n) and one seeded w-aligned window between them, w the
largest power of two with 3 T w <= 2^25 (2048 at T = 4096, 4096 at T = 2048, 8192 at T = 1024).  w >= N1 in every row, so the head holds
every K1.  Only those ranges are downloaded.

Reference and metric: float64 W[(p k) mod n] from one n-entry table of exp(-2 pi i j / n), conjugated for the inverse
kinds; the Inverse result is multiplied by n (exact).  worst = max over all compared outputs of |y - r| -- absolute,
since |r| = 1 -- with the (transform, output) it was found at.

Rule (check): worst <= PIN x recorded (PIN = error_budget.PIN_MAX_REL: GPU results are bit-deterministic) and worst <= CAP
= pi / 2^20 = 3.0e-6, half of a one-index rotation at 2^20.  The cap is derived, not measured: any value under it means a
one-index twiddle error is visible for every n <= 2^20 and an error of ceil(n / 2^20) indices above, except for a row
recorded above CAP / 2, where an error of about one index step may stay under the cap and the pin is what holds the row.
The reference's own arithmetic stays inside the cap on these inputs (forward_ref 5.0e-7 at 2^20, inverse_ref x n with its
f32 on-the-fly twiddles 1.8e-6 at 2^20 and 1.9e-6 at 2^22; tests/test_impulse_sweep.py is the standing proof up to 2^20).
tools/record_impulse_response.py writes RECORD_PATH, tests/test_gpu_impulse_sweep.py applies the rule.
"""
import json
import math
import os

import numpy as np

from . import error_budget as eb
from . import special_values as sv
from .device_run import execute, planned

ROOT = eb.ROOT
RECORD_PATH = os.path.join(ROOT, "tests", "golden", "impulse_response.json")

KINDS = eb.KINDS
PIN = eb.PIN_MAX_REL
CAP = math.pi / (1 << 20)
SEED = 0x5EED
MAX_T = 4096                  # transforms per (row, kind)
MAX_CHUNK = 1 << 30           # samples per exec
MAX_COMPARED = 1 << 25        # outputs per (row, kind)
MIN_TRANSFORMS = 4            # in the buffer of one exec
GEOMETRY_KEYS = ("group", "streams")
HEADROOM_BYTES = 8 << 30      # beside the chunk and its partner buffer: the ring and the tables


# ---- the rows -------------------------------------------------------------------------------------------------------
def _rows():
    rows = []
    for index, r in enumerate(sv.ROWS):
        lf = [r["factors"] >> (8 * i) & 255 for i in range(3)]
        pipelined = r["path"] in (1, eb.PATH_TILED)
        lf = [v for v in lf if v] if pipelined else []
        n = r["n"]
        name = "pipeline_2^20" if r["path"] == 1 else r["case"]
        rows.append(dict(case=name, index=index, n=n, path=r["path"], factors=r["factors"], kernels=r["kernels"],
                         tunables={k: v for k, v in r["tunables"].items() if k not in GEOMETRY_KEYS},
                         lengths=tuple(1 << v for v in lf), R=n >> lf[0] if pipelined else n))
    return rows


ROWS = _rows()
MATRIX = [dict(r, id="%s/%s" % (r["case"], kind), kind=kind, direction=direction) for r in ROWS for kind, direction in KINDS]


def transforms(row):
    return min(row["R"], MAX_T)


def _rng(row, stream):
    return np.random.default_rng([SEED, row["index"], stream])


def _sampled_residues(row, rng):
    """4096 of the R > 4096 residues of a three-pass row: residue t S + o_t of stratum t (S = R / 4096).  A block of N3 / S
    strata is one middle digit m; inside it stratum j takes the offset (m + c_j) mod S, c_j seeded: over the N2 >= S blocks
    every offset of every stratum occurs, hence every last digit.  c_0 = c_last = 0 gives residues 0 and R - 1; transform 1
    takes residue 1 instead of its stratum's (the digits it leaves are met again S blocks further on)."""
    R = row["R"]
    _, N2, N3 = row["lengths"]
    S = R // MAX_T
    per = N3 // S
    assert S > 1 and per >= 1 and N3 % S == 0 and N2 % S == 0 and N2 >= S, row["case"]
    c = rng.integers(0, S, per)
    c[0] = c[-1] = 0
    t = np.arange(MAX_T, dtype=np.int64)
    r = t * S + (t // per + c[t % per]) % S
    r[1] = 1
    return r


def positions(row):
    """p_t of every transform: int64, a pure function of the row."""
    n, R, T = row["n"], row["R"], transforms(row)
    rng = _rng(row, 0)
    if not row["lengths"]:
        if n <= MAX_T:
            return np.arange(n, dtype=np.int64)
        S = n // T
        return np.arange(T, dtype=np.int64) * S + rng.integers(0, S, T)
    r = np.arange(R, dtype=np.int64) if R <= MAX_T else _sampled_residues(row, rng)
    return r + R * rng.integers(0, row["lengths"][0], T)


def window_width(row):
    """None where every output is compared, else w: the largest power of two with 3 T w <= MAX_COMPARED."""
    T = transforms(row)
    if T * row["n"] <= MAX_COMPARED:
        return None
    return 1 << ((MAX_COMPARED // (3 * T)).bit_length() - 1)


def window_starts(row):
    """the seeded w-aligned window of every transform, between the head and the tail"""
    w = window_width(row)
    return w * _rng(row, 1).integers(1, row["n"] // w - 1, transforms(row))


def compared_outputs(row):
    w = window_width(row)
    return transforms(row) * (row["n"] if w is None else 3 * w)


def chunk_transforms(row):
    """impulse transforms per exec"""
    return min(transforms(row), MAX_CHUNK // row["n"])


def buffer_transforms(row):
    return max(MIN_TRANSFORMS, chunk_transforms(row))


def device_bytes_needed(row):
    return 2 * buffer_transforms(row) * row["n"] * 8 + HEADROOM_BYTES


# ---- reference and metric -------------------------------------------------------------------------------------------
def twiddle_table(n):
    return np.exp(-2j * np.pi * np.arange(n) / n)


def _beats(v, worst):
    """a NaN beats every number and is beaten by nothing"""
    return worst == worst and (v != v or v > worst)


def worst_of(y, p, ks, n, table, kind):
    """y: (transforms, outputs) complex64 results of impulses at p[t], at output indices ks[t] (or ks for all) ->
    (worst |y - r|, row of y, column of y); NaN wins."""
    y = np.asarray(y)
    ks = np.asarray(ks, dtype=np.int64)
    worst, where = -1.0, (0, 0)
    step = max(1, (1 << 22) // y.shape[1])
    for t0 in range(0, y.shape[0], step):
        kk = ks[t0:t0 + step] if ks.ndim == 2 else ks[None, :]
        r = table[(p[t0:t0 + step, None] * kk) % n]
        yb = y[t0:t0 + step].astype(np.complex128)
        if kind != "Forward":
            r = np.conj(r)
        if kind == "Inverse":
            yb = yb * n
        d = np.abs(yb - r)
        i = int(np.argmax(d))                       # the first NaN where there is one
        v = float(d.flat[i])
        if _beats(v, worst):
            worst, where = v, (t0 + i // d.shape[1], i % d.shape[1])
    return worst, where[0], where[1]


def sweep(row, kind, run_chunk, only=None, per=None):
    """Drive one (row, kind): run_chunk(p) executes the impulses at the positions `p` (one transform each, in a buffer of
    max(len(p), MIN_TRANSFORMS) transforms, the rest zero) and returns fetch(first sample, count) -> complex64 of the
    result.  `only`: the transforms to run (default all), `per`: transforms per chunk (default chunk_transforms).
    -> dict(worst, t, k, p, compared)."""
    n = row["n"]
    pos = positions(row)
    w = window_width(row)
    win = None if w is None else window_starts(row)
    ts = np.arange(len(pos)) if only is None else np.asarray(only)
    per = per or chunk_transforms(row)
    table = twiddle_table(n)
    best = dict(worst=-1.0, t=0, k=0, p=0, compared=0)
    for c0 in range(0, len(ts), per):
        tc = ts[c0:c0 + per]
        cnt = len(tc)
        fetch = run_chunk(pos[tc])
        if w is None:
            y = fetch(0, cnt * n).reshape(cnt, n)
            ks = np.arange(n, dtype=np.int64)
        else:
            y = np.empty((cnt, 3 * w), dtype=np.complex64)
            y[0, :w] = fetch(0, w)
            for j in range(1, cnt):                 # the tail of transform j - 1 and the head of j: one range
                s = fetch(j * n - w, 2 * w)
                y[j - 1, 2 * w:], y[j, :w] = s[:w], s[w:]
            y[cnt - 1, 2 * w:] = fetch(cnt * n - w, w)
            for j in range(cnt):
                y[j, w:2 * w] = fetch(j * n + int(win[tc[j]]), w)
            a = np.arange(w, dtype=np.int64)
            ks = np.concatenate([np.broadcast_to(a, (cnt, w)), win[tc][:, None] + a, np.broadcast_to(n - w + a, (cnt, w))], axis=1)
        v, j, c = worst_of(y, pos[tc], ks, n, table, kind)
        for extra in range(cnt, MIN_TRANSFORMS):     # the transforms that pad a short chunk hold no impulse
            z = fetch(extra * n, n)
            if not (z == 0).all():
                v, j, c = float("nan"), 0, 0
        best["compared"] += y.size
        if _beats(v, best["worst"]):
            best.update(worst=v, t=int(tc[j]), k=int(ks[j, c] if ks.ndim == 2 else ks[c]), p=int(pos[tc[j]]))
    return best


def impulses(p, n):
    """the input of run_chunk as a host array (the CPU tests; the GPU path writes the impulses on the device)"""
    x = np.zeros(max(len(p), MIN_TRANSFORMS) * n, dtype=np.complex64)
    x[np.arange(len(p)) * n + p] = 1
    return x


# ---- the rule -------------------------------------------------------------------------------------------------------
def check(case, got, rec):
    """A list of failure messages (empty = pass).  `got` and `rec` hold worst (got also t, k, p); `rec` None = no record
    for this case, itself a failure."""
    cid = case["id"]
    if rec is None:
        return ["%s: no recorded entry in %s (run tools/record_impulse_response.py)" % (cid, os.path.relpath(RECORD_PATH, ROOT))]
    v = got["worst"]
    at = "impulse at %d (transform %d), output %d" % (got.get("p", -1), got.get("t", -1), got.get("k", -1))
    bad = []
    if not v <= PIN * rec["worst"]:
        bad.append("%s: worst |y - W^(pk)| %.4g > %.2f x recorded %.4g (cap %.4g): %s" % (cid, v, PIN, rec["worst"], CAP, at))
    if not v <= CAP:
        bad.append("%s: worst |y - W^(pk)| %.4g above the cap %.4g (recorded %.4g): %s" % (cid, v, CAP, rec["worst"], at))
    return bad


def resolved_index_error(n, worst):
    """the smallest index error of a twiddle W_n^e that the pinned row must see: ceil(2 PIN worst / (2 pi / n))"""
    return max(1, math.ceil(2 * PIN * worst / (2 * math.pi / n)))


def load_record(path=RECORD_PATH):
    with open(path) as f:
        return json.load(f)


# ---- running a case on the device -----------------------------------------------------------------------------------
def run_case(fw, dev, queue, case):
    """One (row, kind) through the C ABI -> dict(worst, t, k, p, compared, path, factors, tunables read back)."""
    n, kind = case["n"], case["kind"]
    one = np.ones(1, dtype=np.complex64)
    with planned(fw, dev, queue, kind, n, buffer_transforms(case) * n * 8, case["tunables"]) as p:
        def run_chunk(pos):
            dev.fill_synthetic(p.src, n, scale=0.0, encoder=p.enc)
            for j, pj in enumerate(pos):
                queue.write_buffer(p.src, (j * n + int(pj)) * 8, one, encoder=p.enc)
            out, _ = execute(p)
            return lambda first, count: out.map_read(first * 8, count * 8, p.enc)

        got = sweep(case, kind, run_chunk)
        got.update(path=int(p.plan.get("path")), factors=int(p.plan.get("factors")), tunables=p.held)
    return got
