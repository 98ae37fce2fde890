"""not-gpu: the impulse sweeps of oracle/impulse_sweep.py -- what they cover, that the reference passes, that the smallest
error they exist for does not, and the record.

tests/test_gpu_impulse_sweep.py holds every compared output of up to 4096 swept impulses per (row, kind) to exp(-+2 pi i p k / n)
within CAP = pi / 2^20.  Here (a) every statement of the module's docstring on coverage is computed from positions(row); (b)
the reference's own arithmetic (oracle.forward_ref / inverse_ref / onlyinverse_ref) runs on the very sweep inputs of the rows
up to 2^16 and on 8 seeded transforms of the 2^20 pipeline row and stays under the cap: a failure on the GPU is the
kernel's; (c) doctored results are rejected and located; (d) the record is complete, under the cap and stamped; (e) the
standing argument for the gap: a numpy fp32 four-step FFT with exactly one inter-pass twiddle one index off.

(e) in figures.  1024 x 1024 at 2^20, entry (K1 = 197, r = 601) of the 2^20-domain table one index off: on generator data
rel_l2 moves from 1.68397e-7 to 1.68416e-7 and max_rel not at all -- the error budget cannot see it -- while the impulse at
residue 601 shows 6.0e-6 at exactly the outputs k = 197 mod 1024, twice the cap.  256 x 256 at 2^16, entry (37, 201) one
index of the 2^16 domain off: the impulse check flags exactly (37, 201) at 9.6e-5; the flat 1e-5 bound passes (max_rel
3.7e-6), the budget at this size does NOT stay inside its pin (rel_l2 3.0 x, max_rel 17 x the clean model's): one index at
2^16 is 16 steps of the 2^20 domain, where the budget begins to see single entries.  The same entry off by one step of the
2^20 domain (6.0e-6) leaves rel_l2 within 1.02 x; the sweep sees it as well.
"""
import math
import re

import numpy as np
import pytest

from conftest import REL_TOL
from oracle import error_budget as eb
from oracle import impulse_sweep as im
from oracle import special_values as sv
from test_error_budget import _model_fft

REF = {"Forward": "forward_ref", "Inverse": "inverse_ref", "Onlyinverse": "onlyinverse_ref"}
KINDS = [k for k, _ in im.KINDS]


def _row(name):
    return next(r for r in im.ROWS if r["case"] == name)


def _reference_chunk(oracle, kind, n, doctor=None):
    """run_chunk of im.sweep on the reference's arithmetic; doctor(y, p) may change the result of a chunk in place"""
    def run_chunk(p):
        y = getattr(oracle, REF[kind])(im.impulses(p, n), n)[0]
        if doctor is not None:
            doctor(y, p)
        return lambda first, count: y[first:first + count]
    return run_chunk


def _own_record(got):
    """the rule with the result's own value as the record: what is left is the cap"""
    return {"worst": got["worst"]}


# ---- (a) coverage ---------------------------------------------------------------------------------------------------
def test_rows_are_the_special_value_rows_without_their_geometry():
    assert len(im.ROWS) == len(sv.ROWS) == 44 and len(im.MATRIX) == 3 * 44
    assert len({c["id"] for c in im.MATRIX}) == len(im.MATRIX)
    for r, s in zip(im.ROWS, sv.ROWS):
        assert (r["n"], r["path"], r["factors"], r["kernels"]) == (s["n"], s["path"], s["factors"], s["kernels"])
        assert r["tunables"] == {k: v for k, v in s["tunables"].items() if k not in ("group", "streams")}
        assert not set(r["tunables"]) & {"group", "streams"}
        if r["path"] == eb.PATH_TILED:
            assert list(r["tunables"]) == ["factors", "colsw", "rows32", "p1_gen", "tile_ring"] and r["tunables"]["factors"] == r["factors"]
            assert math.prod(r["lengths"]) == r["n"] and len(r["lengths"]) in (2, 3) and r["R"] == r["n"] // r["lengths"][0]
        elif r["path"] == 1:
            assert r["case"] == "pipeline_2^20" and r["lengths"] == (1024, 1024) and r["R"] == 1024 and r["tunables"] == {}
        else:
            assert r["lengths"] == () and r["R"] == r["n"]
    assert max(r["n"] for r in im.ROWS) == 1 << 22
    assert {c["kind"] for c in im.MATRIX} == set(KINDS)


@pytest.mark.parametrize("row", im.ROWS, ids=[r["case"] for r in im.ROWS])
def test_positions_cover_what_the_docstring_says(row):
    n, R, T = row["n"], row["R"], im.transforms(row)
    p = im.positions(row)
    assert p.dtype == np.int64 and T == min(R, 4096) == len(p)
    assert ((0 <= p) & (p < n)).all() and len(np.unique(p)) == T
    assert np.array_equal(p, im.positions(row))                              # a pure function of the row
    if not row["lengths"]:
        if n <= 4096:
            assert np.array_equal(p, np.arange(n))                           # the whole DFT matrix
        else:
            assert np.array_equal(p // (n // T), np.arange(T))               # one per stratum
            assert len(set((p % (n // T)).tolist())) > 1                     # at seeded offsets
    else:
        N1 = row["lengths"][0]
        r = p % R
        if R <= 4096:
            assert np.array_equal(r, np.arange(R))                           # every residue, in order
        else:
            N2, N3 = row["lengths"][1:]
            assert {0, 1, R - 1} <= set(r.tolist())
            assert set((r % N3).tolist()) == set(range(N3))                  # every last digit
            assert set((r // N3).tolist()) == set(range(N2))                 # every middle digit
            S = R // T
            assert np.bincount(r // S, minlength=T).max() <= 2 and np.count_nonzero(np.bincount(r // S, minlength=T)) >= T - 1
        a = p // R
        assert a.max() < N1 and len(set(a.tolist())) > min(N1, T) // 3       # the column index is sampled widely
    # what is compared
    w = im.window_width(row)
    if T * n <= 1 << 25:
        assert w is None and im.compared_outputs(row) == T * n
    else:
        assert w & (w - 1) == 0 and 3 * T * w <= 1 << 25 < 3 * T * 2 * w
        win = im.window_starts(row)
        assert len(win) == T and (win % w == 0).all() and (win >= w).all() and (win + w <= n - w).all()
        assert len(set(win.tolist())) > 1 or n // w == 3
        if row["lengths"]:
            assert w >= row["lengths"][0]                                    # the head holds every K1
    assert im.compared_outputs(row) <= 1 << 25
    # the execs
    per = im.chunk_transforms(row)
    assert per * n <= 1 << 30 and T % per == 0 and im.buffer_transforms(row) >= 4
    assert im.buffer_transforms(row) == per or (n == 2 and per == 2)
    assert im.device_bytes_needed(row) >= 2 * im.buffer_transforms(row) * n * 8


def test_window_widths_of_the_rows():
    assert {im.transforms(r): im.window_width(r) for r in im.ROWS if im.window_width(r)} == {4096: 2048, 2048: 4096, 1024: 8192}
    assert im.CAP == math.pi / 2 ** 20 and im.PIN == eb.PIN_MAX_REL == 1.5


# ---- (b) the reference passes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in im.MATRIX if c["n"] <= 1 << 16], ids=lambda c: c["id"])
def test_the_reference_stays_under_the_cap_on_the_sweep_inputs(oracle, case):
    n = case["n"]
    got = im.sweep(case, case["kind"], _reference_chunk(oracle, case["kind"], n), per=max(1, (1 << 24) // n))
    assert got["compared"] == im.compared_outputs(case)
    assert 0 <= got["worst"] <= im.CAP and im.check(case, got, _own_record(got)) == [], got


@pytest.fixture(scope="module")
def eight_of_2_20():
    row = _row("pipeline_2^20")
    only = np.sort(np.random.default_rng(im.SEED).choice(im.transforms(row), 8, replace=False))
    return row, only


@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_stays_under_the_cap_on_eight_transforms_of_the_2_20_row(oracle, eight_of_2_20, kind):
    row, only = eight_of_2_20
    got = im.sweep(row, kind, _reference_chunk(oracle, kind, row["n"]), only=only)
    case = dict(row, id="%s/%s" % (row["case"], kind))
    assert got["compared"] == 8 * 3 * 8192 and got["t"] in only
    assert 0 < got["worst"] <= im.CAP and im.check(case, got, _own_record(got)) == [], got


# ---- (c) doctored results -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_1k(oracle):
    row = _row("small32_10")
    return row, im.sweep(row, "Forward", _reference_chunk(oracle, "Forward", row["n"]))


def _doctored(oracle, row, kind, doctor, rec, **kw):
    got = im.sweep(row, kind, _reference_chunk(oracle, kind, row["n"], doctor), **kw)
    return got, im.check(dict(row, id="%s/%s" % (row["case"], kind)), got, rec)


def test_one_output_rotated_by_one_index_of_2_20_is_rejected_and_located(oracle, clean_1k):
    row, clean = clean_1k
    n = row["n"]
    assert im.check(dict(row, id="x"), clean, _own_record(clean)) == []
    t, k = 777, 345

    def doctor(y, p):
        y[t * n + k] *= np.complex64(np.exp(2j * np.pi / 2 ** 20))
    got, bad = _doctored(oracle, row, "Forward", doctor, _own_record(clean))
    assert (got["t"], got["k"], got["p"]) == (t, k, t) and 5.5e-6 < got["worst"] < 6.5e-6
    assert len(bad) == 2 and "above the cap" in bad[1] and "transform 777" in bad[0] and "output 345" in bad[0]
    # half that rotation sits at the cap: the pin is what sees it
    def half(y, p):
        y[t * n + k] *= np.complex64(np.exp(1j * np.pi / 2 ** 20))
    got, bad = _doctored(oracle, row, "Forward", half, _own_record(clean))
    assert (got["t"], got["k"]) == (t, k) and len(bad) >= 1 and "x recorded" in bad[0]


def test_one_conjugated_transform_one_shifted_transform_and_a_nan_are_rejected(oracle, clean_1k):
    row, clean = clean_1k
    n = row["n"]
    rec = _own_record(clean)

    def conj(y, p):
        y[5 * n:6 * n] = np.conj(y[5 * n:6 * n])
    got, bad = _doctored(oracle, row, "Forward", conj, rec)
    assert got["t"] == 5 and got["worst"] > 1.9 and len(bad) == 2          # W^(5k) against its conjugate: up to 2

    def shift(y, p):
        y[300 * n:301 * n] = np.roll(y[300 * n:301 * n], 1)
    got, bad = _doctored(oracle, row, "Forward", shift, rec)
    assert got["t"] == 300 and got["worst"] > 1.0 and len(bad) == 2         # |W^300 - 1|

    def nan(y, p):
        y.view(np.float32)[2 * (900 * n + 17) + 1] = np.nan
    got, bad = _doctored(oracle, row, "Forward", nan, rec)
    assert math.isnan(got["worst"]) and (got["t"], got["k"]) == (900, 17) and len(bad) == 2
    # a NaN is not outvoted by a larger number elsewhere
    def both(y, p):
        nan(y, p)
        conj(y, p)
    got, bad = _doctored(oracle, row, "Forward", both, rec)
    assert math.isnan(got["worst"]) and len(bad) == 2
    assert "no recorded entry" in im.check(dict(row, id="x"), clean, None)[0]


def test_doctoring_is_seen_in_head_window_and_tail_of_a_sampled_row(oracle, eight_of_2_20):
    row, only = eight_of_2_20
    n, w = row["n"], im.window_width(row)
    win = im.window_starts(row)
    j = 3                                                   # the fourth of the eight transforms
    t = int(only[j])
    clean = im.sweep(row, "Onlyinverse", _reference_chunk(oracle, "Onlyinverse", n), only=only)
    for k in (0, w - 1, int(win[t]), int(win[t]) + w - 1, n - w, n - 1):
        def doctor(y, p, k=k):
            y[j * n + k] *= np.complex64(np.exp(2j * np.pi / 2 ** 20))
        got, bad = _doctored(oracle, row, "Onlyinverse", doctor, _own_record(clean), only=only)
        assert (got["t"], got["k"]) == (t, k) and bad, k
    # an output outside the three ranges is not compared: what the docstring calls sampled
    outside = next(k for k in (w, n - w - 1) if not win[t] <= k < win[t] + w)

    def doctor(y, p):
        y[j * n + outside] = 0
    got, bad = _doctored(oracle, row, "Onlyinverse", doctor, _own_record(clean), only=only)
    assert got == clean and not bad


def test_a_padding_transform_that_is_not_zero_is_rejected(oracle):
    row = _row("chunk_2")
    assert im.buffer_transforms(row) == 4 and im.transforms(row) == 2

    def doctor(y, p):
        assert y.size == 8
        y[7] = 1e-30
    got, bad = _doctored(oracle, row, "Forward", doctor, {"worst": 1e-7})
    assert math.isnan(got["worst"]) and bad


# ---- (d) the record -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    return im.load_record()


def test_every_case_has_a_record_under_the_cap(record):
    ids = [c["id"] for c in im.MATRIX]
    assert sorted(record["cases"]) == sorted(ids)
    for c in im.MATRIX:
        rec = record["cases"][c["id"]]
        assert set(rec) == {"worst", "t", "k", "p", "compared", "path", "factors", "tunables"}, c["id"]
        assert isinstance(rec["worst"], float) and 0.0 < rec["worst"] <= im.CAP, c["id"]
        assert (rec["path"], rec["factors"], rec["tunables"]) == (c["path"], c["factors"], c["tunables"]), c["id"]
        assert rec["compared"] == im.compared_outputs(c) and rec["p"] == int(im.positions(c)[rec["t"]]) and 0 <= rec["k"] < c["n"]
        assert im.check(c, rec, rec) == []
    assert record["cap"] == im.CAP and record["pin"] == im.PIN


def test_record_resolves_one_index_up_to_2_20(record):
    assert sorted(record["rows"]) == sorted(r["case"] for r in im.ROWS)
    for r in im.ROWS:
        rr = record["rows"][r["case"]]
        worst = max(record["cases"]["%s/%s" % (r["case"], k)]["worst"] for k in KINDS)
        assert rr == {"n": r["n"], "worst": worst, "resolved_index_error": im.resolved_index_error(r["n"], worst)}
        if r["n"] <= 1 << 20:
            assert rr["resolved_index_error"] == 1, r["case"]
        else:
            assert rr["resolved_index_error"] <= 2 * (r["n"] >> 20), r["case"]
    assert im.resolved_index_error(1 << 20, 1.9e-6) == 1 and im.resolved_index_error(1 << 20, 2.1e-6) == 2


def test_record_schema_and_stamp(record):
    assert set(record) == {"_comment", "stamp", "cap", "pin", "cases", "rows"}
    st = record["stamp"]
    assert re.fullmatch(r"[0-9a-f]{7,40}\+?", st["commit"]), st["commit"]
    assert st["kernel_sources"] == eb.KERNEL_SOURCE_DIR + "/*"
    assert st["library"] == "product" and "gfx950" in st["device"]
    assert st["kernel_source_sha256"] == eb.kernel_source_sha256(), \
        "kernel sources changed since the impulse sweeps were recorded: re-run tools/record_impulse_response.py"


# ---- (e) the standing argument: one inter-pass twiddle one index off ---------------------------------------------------
def _f32_twiddle(e, n, step=0.0):
    th = -2 * np.pi * ((np.asarray(e) % n) / n + step)
    return (np.cos(th).astype(np.float32) + 1j * np.sin(th).astype(np.float32)).astype(np.complex64)


def _four_step(x, N1, R, tw):
    """fp32 four-step FFT of the rows of x (n = N1 R): N1-point columns at stride R (the radix-2 model of
    test_error_budget.py), times tw[K1, r] = W_n^(K1 r), R-point rows; output k = K1 + N1 K2."""
    b = x.size // (N1 * R)
    cols = np.ascontiguousarray(x.reshape(b, N1, R).transpose(0, 2, 1))                       # [b, r, a]
    a = _model_fft(cols.reshape(-1), N1, False).reshape(b, R, N1)                             # [b, r, K1]
    a = (a * tw.T[None]).astype(np.complex64)
    y = _model_fft(np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1), R, False).reshape(b, N1, R)
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(-1)


def _impulse_worst(N1, R, tw, residues):
    """the impulse check on the model: impulses at p = r (a = 0) for r in `residues` -> {r: (worst, K1 of the worst)}"""
    n = N1 * R
    table = im.twiddle_table(n)
    out = {}
    for r in residues:
        y = _four_step(im.impulses(np.array([r]), n)[:n], N1, R, tw).reshape(1, n)
        v, _, k = im.worst_of(y, np.array([r], dtype=np.int64), np.arange(n), n, table, "Forward")
        out[r] = (v, k % N1)
    return out


def test_one_twiddle_one_index_off_at_256_x_256_is_flagged_at_its_k1_and_residue(oracle):
    N1 = R = 256
    n = N1 * R
    K1, r0 = 37, 201
    tw = _f32_twiddle(np.outer(np.arange(N1), np.arange(R)), n)
    bad = tw.copy()
    bad[K1, r0] = _f32_twiddle(K1 * r0 + 1, n)
    assert np.count_nonzero(bad != tw) == 1
    x = oracle.gen_input(n, eb.samples(n))
    ref = oracle.dft_f64(x, n, -1)
    clean_l2, clean_mx = eb.metrics(_four_step(x, N1, R, tw), ref, n)
    bad_l2, bad_mx = eb.metrics(_four_step(x, N1, R, bad), ref, n)
    print("256 x 256, (K1, r) = (%d, %d) one index of 2^16 off: rel_l2 %.4g -> %.4g, max_rel %.4g -> %.4g"
          % (K1, r0, clean_l2, bad_l2, clean_mx, bad_mx))
    assert clean_l2 <= 0.7 * eb.cap(n)                                       # the model is as good as the radix-2 one
    assert bad_mx <= REL_TOL and bad_l2 <= REL_TOL                           # the flat bound sees nothing
    # at 2^16 one index is 16 steps of the 2^20 domain and the budget does see the entry (module docstring)
    assert bad_l2 > eb.PIN_REL_L2 * clean_l2 and bad_mx > eb.PIN_MAX_REL * clean_mx
    # the impulse check: exactly that residue, exactly that K1
    seen = _impulse_worst(N1, R, bad, [0, 1, r0 - 1, r0, r0 + 1, R - 1])
    for r, (v, k1) in seen.items():
        if r == r0:
            assert k1 == K1 and 0.9 * 2 * np.pi / n < v < 1.1 * 2 * np.pi / n and v > 30 * im.CAP
        else:
            assert v <= im.CAP / 3, (r, v)
    # the same entry off by one step of the 2^20 domain: rel_l2 does not move, the impulse still stands above the cap
    fine = tw.copy()
    fine[K1, r0] = _f32_twiddle(K1 * r0, n, step=2.0 ** -20)
    fine_l2, fine_mx = eb.metrics(_four_step(x, N1, R, fine), ref, n)
    print("the same entry one step of 2^20 off: rel_l2 %.4g, max_rel %.4g" % (fine_l2, fine_mx))
    assert fine_l2 <= 1.02 * clean_l2
    v, k1 = _impulse_worst(N1, R, fine, [r0])[r0]
    assert k1 == K1 and v > im.CAP


def test_one_entry_of_a_2_20_domain_table_one_index_off_moves_no_budget_metric_and_is_seen_by_the_sweep(oracle):
    N1 = R = 1024
    n = N1 * R
    K1, r0 = 5 + 32 * 6, 601                                 # A[k1 = 5][c = 9] of tile 37 times B[k2 = 6][c] (tables.cpp)
    tw = _f32_twiddle(np.outer(np.arange(N1), np.arange(R)), n)
    bad = tw.copy()
    bad[K1, r0] = _f32_twiddle(K1 * r0 + 1, n)
    x = oracle.gen_input(n, 1)
    ref = oracle.dft_f64(x, n, -1)
    clean_l2, clean_mx = eb.metrics(_four_step(x, N1, R, tw), ref, n)
    bad_l2, bad_mx = eb.metrics(_four_step(x, N1, R, bad), ref, n)
    print("1024 x 1024, (K1, r) = (%d, %d) one index of 2^20 off: rel_l2 %.6g -> %.6g, max_rel %.6g -> %.6g"
          % (K1, r0, clean_l2, bad_l2, clean_mx, bad_mx))
    assert clean_l2 <= 0.7 * eb.cap(n)
    assert bad_l2 <= 1.001 * clean_l2 and bad_mx <= 1.001 * clean_mx         # far inside the pins 1.25 and 1.5
    assert eb.check(dict(id="model", n=n), dict(rel_l2=bad_l2, max_rel=bad_mx), dict(rel_l2=clean_l2, max_rel=clean_mx)) == []
    # the sweep's own transform of that residue (only the affected column is emulated: the others never meet the entry)
    row = _row("pipeline_2^20")
    p = im.positions(row)
    t = int(np.flatnonzero(p % R == r0)[0])
    assert t == r0                                                           # every residue is swept, in order
    w = im.window_width(row)

    def run_chunk(pp):
        y = _four_step(im.impulses(pp, n)[:n], N1, R, bad)
        z = np.zeros(im.MIN_TRANSFORMS * n, dtype=np.complex64)
        z[:n] = y
        return lambda first, count: z[first:first + count]
    got = im.sweep(row, "Forward", run_chunk, only=[t])
    case = dict(row, id="pipeline_2^20/Forward")
    assert got["k"] % N1 == K1 and got["t"] == t and 0.9 * 2 * np.pi / n < got["worst"] < 1.1 * 2 * np.pi / n
    assert K1 < N1 <= w                                                      # the head alone holds an output of that K1
    rec = im.load_record()["cases"]["pipeline_2^20/Forward"]
    bad_msgs = im.check(case, got, rec)
    assert len(bad_msgs) == 2 and "above the cap" in bad_msgs[1]
    # the clean model on the same transform passes the rule against the GPU's record
    def run_clean(pp):
        z = np.zeros(im.MIN_TRANSFORMS * n, dtype=np.complex64)
        z[:n] = _four_step(im.impulses(pp, n)[:n], N1, R, tw)
        return lambda first, count: z[first:first + count]
    assert im.check(case, im.sweep(row, "Forward", run_clean, only=[t]), rec) == []
