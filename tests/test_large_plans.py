"""not-gpu: the sparse-input checks of the 2^28 .. 2^30 plans (oracle/large_plans.py) -- what they cover, that an fp32 model of
the twiddle path passes, that the errors they exist for do not, and the record.

(a) the rows against tests/golden/tiled_schedule.txt and every statement of the module's docstring on positions and windows,
computed from the functions; (b) the record: every case stamped and under the cap; (c) an fp32 model of the twiddle path of
a three-pass plan -- the five table factors W_N1^(a K1), W_n^(r K1) = hi lo, W_N2^(r2 K2), W_R^(r3 K2) = hi lo, W_N3^(r3 K3),
each f64 rounded to f32 as tables.cpp builds them, multiplied with fp32 cmul -- passes the rule on a row's own (p, k), and the
same outputs with one hi index taken one too high (for one value of e >> 10, in pass A and again in the middle pass) fail it
at 2^29 and at 2^30; (d) a column comb whose quarter of the amplitudes was read as zeros, and one non-zero sample in the
empty transform of the batch-2 case, fail; (e) the reference evaluators run at 2^30 without an allocation of size n, and the
column comb's reference agrees with its closed form W^(r k) DFT_N1(g)[k mod N1].

The rows at 2^29 and 2^30 are the accepted factor tuples, and per size they run every pass-A kernel the golden gives for any
of them (k_tile columns at 512 and 1024 points, k_p1_gen); 10,10,9 runs with k_p1_gen only: its k_tile columns<10> is the
instantiation 10,9,10 with p1_gen 0 already runs at the same span.
"""
import re
import tracemalloc

import numpy as np
import pytest

from conftest import REL_TOL
from oracle import error_budget as eb
from oracle import impulse_sweep as im
from oracle import kernel_cells as kc
from oracle import large_plans as lp

KINDS = [k for k, _ in lp.KINDS]
ROW_IDS = [r["case"] for r in lp.ROWS]


# ---- (a) rows, positions, windows -------------------------------------------------------------------------------------
def _pass_a_of(row):
    """the pass-A kernels the golden gives for the flag settings the row leaves open, and its later passes"""
    by_flag = kc.parse_golden()[1][(row["lg"], row["lg_factors"])]
    fixed = {k: v for k, v in row["tunables"].items() if k in kc.FLAG_KEYS}
    if row["lg"] <= 28:
        fixed = dict(kc.FLAG_DEFAULTS, **fixed)
    picked = [by_flag[i] for i in range(16) if all((i >> kc.FLAG_KEYS.index(k) & 1) == v for k, v in fixed.items())]
    assert picked and all(d[1:] == ("tilec", "tiler", 0, 3) for d in picked), row["case"]
    return {d[0] for d in picked}


def test_rows_are_the_accepted_tuples_of_the_golden_with_every_pass_a_kernel():
    table = kc.parse_golden()[1]
    assert ROW_IDS == ["colsw_2^28", "p1gen_2^29", "tilec10_2^29", "tilec9_2^29", "tiler9_2^29", "p1gen_2^30", "tilec10_2^30"]
    for lg, tuples in ((29, {(9, 10, 10), (10, 9, 10), (10, 10, 9)}), (30, {(10, 10, 10)})):
        accepted = {f for (l, f) in table if l == lg}
        rows = [r for r in lp.ROWS if r["lg"] == lg]
        assert accepted == tuples == {r["lg_factors"] for r in rows}
        golden = {(d[0], f[0]) for f in accepted for d in table[(lg, f)]}
        ran = set()
        for r in rows:
            a = _pass_a_of(r)
            assert len(a) == 1, (r["case"], a)                               # the row's keys decide the kernel
            ran.add((a.pop(), r["lg_factors"][0]))
        assert ran == golden, (lg, ran, golden)
        for f in accepted:                                                   # both decisions of a tuple that has two ...
            if len({d[0] for d in table[(lg, f)]}) == 2 and f != (10, 10, 9):   # ... (module docstring: but 10,10,9)
                assert {r["tunables"].get("p1_gen") for r in rows if r["lg_factors"] == f} == {0, 1}
    r28 = lp.row_named("colsw_2^28")
    assert _pass_a_of(r28) == {"colsw"} and r28["tunables"] == {"factors": eb.pack_factors(9, 9, 10), "colsw": 1}
    for r in lp.ROWS:
        assert r["n"] == 1 << r["lg"] == int(np.prod(r["lengths"], dtype=np.int64)) and r["R"] == r["n"] // r["lengths"][0]
        assert r["factors"] == r["tunables"]["factors"] == eb.pack_factors(*r["lg_factors"]) and r["path"] == eb.PATH_TILED
        assert set(r["tunables"]) <= {"factors", "p1_gen", "colsw"}
        assert ("p1_gen" in r["tunables"]) == (r["lg_factors"][0] == 10)     # set wherever it decides anything
    assert len({r["index"] for r in lp.ROWS} | {r["index"] for r in im.ROWS}) == len(lp.ROWS) + len(im.ROWS)


def test_matrix_is_every_row_in_every_kind_and_the_batch_2_case():
    assert len(lp.MATRIX) == 22 == len({c["id"] for c in lp.MATRIX})
    assert [c["id"] for c in lp.MATRIX[:21]] == ["%s/%s" % (r, k) for r in ROW_IDS for k in KINDS]
    for c in lp.MATRIX[:21]:
        assert (c["batch"], c["only"], c["combs"]) == (1, None, True)
        assert lp.compared_outputs(c) == c["T"] * 34 * 2048 + 4 * (1 << 14)
        assert lp.device_bytes_needed(c) == 4 * c["n"] * 8 + (8 << 30)
    b = lp.MATRIX[21]
    row = lp.row_named("p1gen_2^29")
    assert (b["id"], b["kind"], b["batch"], b["combs"], b["tunables"]) == ("batch2_2^29/Forward", "Forward", 2, False, row["tunables"])
    assert len(b["only"]) == 8 == len(set(b["only"])) and {0, 1, b["T"] - 1} <= set(b["only"]) and max(b["only"]) < b["T"]
    assert lp.compared_outputs(b) == 8 * 34 * 2048
    assert b["batch"] * b["n"] * 8 == 8 << 30                                # the batch stride is 4 GiB
    assert (lp.CAP, lp.PIN, lp.PIN_COMB, lp.REL_TOL) == (im.CAP, im.PIN, eb.PIN_MAX_REL, REL_TOL)
    assert lp.CAP == 0.5 * 2 * np.pi * 1024 / 2 ** 30 == 0.25 * 2 * np.pi * 1024 / 2 ** 29   # half / a quarter of one hi step


@pytest.mark.parametrize("row", lp.ROWS, ids=ROW_IDS)
def test_positions_and_windows_are_what_the_docstring_says(row):
    n, R, T = row["n"], row["R"], row["T"]
    N1, N2, N3 = row["lengths"]
    assert T in (32, 64, 128) and T == lp.T_IMPULSES
    p, r, a = lp.positions(row), lp.residues(row), lp.columns(row)
    assert p.dtype == np.int64 and len(p) == T == len(set(p.tolist())) and ((0 <= p) & (p < n)).all()
    assert np.array_equal(p, lp.positions(row)) and np.array_equal(p, r + R * a) and (r < R).all()
    # residues: one per stratum of R / T (stratum 1 gave its one to the forced residue 1), 0, 1 and R - 1 among them
    S = R // T
    assert {0, 1, R - 1} <= set(r.tolist())
    assert np.array_equal(np.delete(r // S, 1), np.delete(np.arange(T), 1)) and len(set((r % S).tolist())) > T // 4
    assert {0, N3 - 1} <= set((r % N3).tolist()) and {0, N2 - 1} <= set((r // N3).tolist())
    # columns: T / 4 per quarter, 0 and N1 - 1 among them, and the last input of the transform
    assert np.array_equal(np.bincount(a // (N1 // 4), minlength=4), [T // 4] * 4) and (a < N1).all()
    assert {0, N1 - 1} <= set(a.tolist()) and len(set(a.tolist())) > T // 2
    assert n - 1 in p.tolist()
    # windows: 34 per exec, w >= N1, disjoint, in range, w-aligned, one per stratum, not the same in every exec
    win = lp.window_starts(row)
    assert win.shape == (T, 34) and lp.W == 2048 >= N1
    assert (win[:, 0] == 0).all() and (win[:, -1] == n - lp.W).all() and (win % lp.W == 0).all()
    assert (np.diff(win, axis=1) >= lp.W).all() and (win >= 0).all() and (win + lp.W <= n).all()
    edge = 1 + np.arange(33, dtype=np.int64) * (n // lp.W - 2) // 32         # 32 strata of the windows 1 .. n / w - 2
    assert edge[0] == 1 and edge[-1] == n // lp.W - 1 and np.ptp(np.diff(edge)) <= 1
    block = win[:, 1:-1] // lp.W
    assert (block >= edge[:-1]).all() and (block < edge[1:]).all()
    assert (np.array([len(set(win[:, j].tolist())) for j in range(1, 33)]) > T // 2).all()
    ks = lp.window_indices(win[5])
    assert ks.shape == (34 * 2048,) and (np.diff(ks) > 0).all() and set((ks[:2048] % N1).tolist()) == set(range(N1))
    assert len(set((ks // (N1 * N2)).tolist())) >= 34                        # spread over K3
    cw = lp.comb_window_starts(row)
    assert cw.shape == (4, 8) and (np.diff(cw, axis=1) >= lp.W).all() and (cw[:, 0] == 0).all() and (cw[:, -1] == n - lp.W).all()


@pytest.mark.parametrize("row", lp.ROWS, ids=ROW_IDS)
def test_combs_are_what_the_docstring_says(row):
    n, R = row["n"], row["R"]
    N1, N2, N3 = row["lengths"]
    combs = lp.combs(row)
    assert [c[0] for c in combs] == list(lp.COMBS) == ["column_last", "column_seeded", "middle", "row"]
    for (name, p, g), (_, p2, g2) in zip(combs, lp.combs(row)):
        assert np.array_equal(p, p2) and np.array_equal(g, g2)               # a pure function of the row
        assert p.dtype == np.int64 and g.dtype == np.complex64 and len(p) == len(g) <= 1024 and len(set(p.tolist())) == len(p)
        assert ((0 <= p) & (p < n)).all() and (np.abs(g.real) <= 1).all() and (np.abs(g.imag) <= 1).all() and np.abs(g).min() > 0
    (_, p0, _), (_, p1, _), (_, pm, _), (_, pr, _) = combs
    for p, r in ((p0, R - 1), (p1, int(p1[0]))):
        assert np.array_equal(p, r + R * np.arange(N1)) and 0 < r < R        # every a: all four quarters, the full span
    assert p1[0] != R - 1 and p0[-1] == n - 1
    a, r = pm // R, pm % R
    assert len(set(a.tolist())) == 1 and a[0] >= 3 * N1 // 4 and np.array_equal(r // N3, np.arange(N2)) and len(set((r % N3).tolist())) == 1
    a, r = pr // R, pr % R
    assert len(set(a.tolist())) == 1 and a[0] >= 3 * N1 // 4 and np.array_equal(r % N3, np.arange(N3)) and len(set((r // N3).tolist())) == 1


# ---- (b) the record ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    return lp.load_record()


def test_every_case_has_a_stamped_record_under_the_cap(record):
    assert set(record) == {"_comment", "stamp", "cap", "pin", "rel_tol", "cases", "notes"}
    assert sorted(record["cases"]) == sorted(c["id"] for c in lp.MATRIX)
    assert (record["cap"], record["pin"], record["rel_tol"]) == (lp.CAP, lp.PIN, lp.REL_TOL)
    for c in lp.MATRIX:
        rec = record["cases"][c["id"]]
        assert set(rec) == {"worst", "t", "k", "p", "compared", "combs", "zero_failures", "path", "factors", "tunables", "T", "seconds"}, c["id"]
        assert isinstance(rec["worst"], float) and 0.0 < rec["worst"] <= lp.CAP, c["id"]
        assert (rec["path"], rec["factors"], rec["tunables"], rec["T"]) == (c["path"], c["factors"], c["tunables"], c["T"]), c["id"]
        assert rec["compared"] == lp.compared_outputs(c) and rec["p"] == int(lp.positions(c)[rec["t"]]) and 0 <= rec["k"] < c["n"]
        assert rec["zero_failures"] == [] and rec["seconds"] > 0
        assert [g["name"] for g in rec["combs"]] == (list(lp.COMBS) if c["combs"] else [])
        for g in rec["combs"]:
            assert 0.0 < g["max_rel"] <= lp.REL_TOL and 0.0 < g["rel_l2"] <= lp.REL_TOL, (c["id"], g)
        assert lp.check(c, rec, rec) == []
    st = record["stamp"]
    assert re.fullmatch(r"[0-9a-f]{7,40}\+?", st["commit"]), st["commit"]
    assert st["kernel_sources"] == eb.KERNEL_SOURCE_DIR + "/*" and st["library"] == "product" and "gfx950" in st["device"]
    assert st["kernel_source_sha256"] == eb.kernel_source_sha256(), \
        "kernel sources changed since the large plans were recorded: re-run tools/record_large_plans.py"


# ---- (c) the fp32 model of the twiddle path, clean and with one hi index one too high ---------------------------------------
def _tw32(e, domain):
    """tables.cpp tw_f64: f64 math rounded to f32"""
    th = -2.0 * np.pi * np.asarray(e, dtype=np.float64) / domain
    return (np.cos(th).astype(np.float32) + 1j * np.sin(th).astype(np.float32)).astype(np.complex64)


def _cmul32(a, b):
    ar, ai, br, bi = a.real, a.imag, b.real, b.imag                          # float32: every operation rounds
    return ((ar * br - ai * bi) + 1j * (ar * bi + ai * br)).astype(np.complex64)


def _model(row, p, ks, kind, doctor=None):
    """the output of the impulse at p at the outputs ks, as the product of the five table factors; doctor = (pass, h): the hi
    entry h of that pass's two-level table is read one index too high"""
    n, R = row["n"], row["R"]
    N1, N2, N3 = row["lengths"]
    a, r = divmod(int(p), R)
    r2, r3 = divmod(r, N3)
    K1, K2, K3 = ks % N1, ks // N1 % N2, ks // (N1 * N2)
    ea, eb_ = r * K1, r3 * K2
    assert ea.max() < n and eb_.max() < R
    ha, hb = ea >> 10, eb_ >> 10
    if doctor is not None:
        ha = np.where((ha == doctor[1]) & (doctor[0] == "A"), ha + 1, ha)
        hb = np.where((hb == doctor[1]) & (doctor[0] == "B"), hb + 1, hb)
    f = _tw32(a * K1 % N1, N1)
    f = _cmul32(f, _cmul32(_tw32(1024 * ha, n), _tw32(ea & 1023, n)))
    f = _cmul32(f, _tw32(r2 * K2 % N2, N2))
    f = _cmul32(f, _cmul32(_tw32(1024 * hb, R), _tw32(eb_ & 1023, R)))
    f = _cmul32(f, _tw32(r3 * K3 % N3, N3))
    if kind != "Forward":
        f = np.conj(f)
    return f / np.float32(n) if kind == "Inverse" else f


def _model_exec(case, doctor=None):
    n, base = case["n"], (case["batch"] - 1) * case["n"]

    def run_exec(pos, amps):
        assert len(pos) == 1 and amps[0] == 1
        return lambda first, count: _model(case, pos[0], np.arange(first - base, first - base + count, dtype=np.int64), case["kind"], doctor)
    return run_exec


def _sample(name, kind, execs=(0, 1, 40, 77, 127)):
    case = next(c for c in lp.MATRIX if c["id"] == "%s/%s" % (name, kind))
    return dict(case, only=list(execs), combs=False)


@pytest.mark.parametrize("name,kind", [("p1gen_2^29", "Forward"), ("tilec9_2^29", "Inverse"), ("tiler9_2^29", "Onlyinverse"),
                                       ("p1gen_2^30", "Forward"), ("tilec10_2^30", "Inverse"), ("colsw_2^28", "Forward")])
def test_the_fp32_twiddle_path_passes_on_a_rows_own_sample(name, kind):
    case = _sample(name, kind, execs=(0, 1, 23, 40, 58, 77, 101, 127))
    got = lp.sweep(case, _model_exec(case))
    print("%s: fp32 model worst %.3e = %.2f of the cap at p %d, k %d" % (case["id"], got["worst"], got["worst"] / lp.CAP, got["p"], got["k"]))
    assert got["compared"] == 8 * 34 * 2048 and got["p"] == int(lp.positions(case)[got["t"]])
    assert 0 < got["worst"] <= 0.25 * lp.CAP                                 # 3.6e-7 = 0.12 x CAP over random (p, k)
    assert lp.check(case, got, dict(got)) == []
    assert case["n"] - 1 in lp.positions(case)[case["only"]].tolist()        # p = n - 1 and k = n - 1 are in the sample
    assert case["n"] - 1 == lp.window_indices(lp.window_starts(case)[127])[-1]


@pytest.mark.parametrize("name", ["p1gen_2^29", "p1gen_2^30"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_one_hi_index_one_too_high_fails_the_rule(name, which):
    case = _sample(name, "Forward")
    n, R = case["n"], case["R"]
    N1, N2, N3 = case["lengths"]
    clean = lp.sweep(case, _model_exec(case))
    assert lp.check(case, clean, dict(clean)) == []
    # one value of e >> 10 that the sample meets: that of its exec 77 at the 1000th output of its 21st window
    t = 77
    p = int(lp.positions(case)[t])
    k = int(lp.window_starts(case)[t, 20]) + 999
    r = p % R
    h = (r * (k % N1)) >> 10 if which == "A" else ((r % N3) * (k // N1 % N2)) >> 10
    assert h > 0
    got = lp.sweep(case, _model_exec(case, (which, h)))
    bad = lp.check(case, got, dict(clean))
    step = 2 * np.pi * 1024 / (n if which == "A" else R)
    print("%s pass %s, hi[%d] read as hi[%d]: worst %.3e (clean %.3e, cap %.3e) at p %d, k %d"
          % (case["id"], which, h, h + 1, got["worst"], clean["worst"], lp.CAP, got["p"], got["k"]))
    assert 0.9 * step < got["worst"] < 1.1 * step and got["worst"] > 1.8 * lp.CAP
    assert len(bad) == 2 and "above the cap" in bad[1] and "x recorded" in bad[0]
    # located: the flagged output reads that very entry
    e = (got["p"] % R) * (got["k"] % N1) if which == "A" else (got["p"] % R % N3) * (got["k"] // N1 % N2)
    assert e >> 10 == h


# ---- (d) a descriptor that read zeros; a sample in the empty transform -------------------------------------------------
def test_a_column_comb_without_one_quarter_of_its_amplitudes_fails_its_bound():
    row = lp.row_named("p1gen_2^29")
    N1 = row["lengths"][0]
    (name, p, g), starts = lp.combs(row)[0], lp.comb_window_starts(row)[0]
    ks = lp.window_indices(starts)[::16]                                     # 1024 of the compared outputs
    r = lp.comb_reference(p, g, ks, row["n"], "Forward")
    clean = dict(zip(("max_rel", "rel_l2"), lp.comb_metrics(r.astype(np.complex64), r)), name=name)
    assert lp.check_comb("x", clean, clean) == [] and clean["max_rel"] < 2e-7
    for quarter in range(4):
        dropped = g.copy()
        dropped[quarter * N1 // 4:(quarter + 1) * N1 // 4] = 0               # p = r + R a: the amplitudes of that quarter of a
        y = lp.comb_reference(p, dropped, ks, row["n"], "Forward").astype(np.complex64)
        got = dict(zip(("max_rel", "rel_l2"), lp.comb_metrics(y, r)), name=name)
        bad = lp.check_comb("x", got, clean)
        assert got["max_rel"] > 0.1 and got["rel_l2"] > 0.1 and len(bad) == 4, (quarter, got)


def _reference_exec(case, doctor=None):
    """run_exec on the float64 reference rounded to complex64, over the whole buffer of the case"""
    n, base = case["n"], (case["batch"] - 1) * case["n"]

    def run_exec(pos, amps):
        def fetch(first, count):
            ks = np.arange(first % n, first % n + count, dtype=np.int64)
            y = lp.comb_reference(pos, amps, ks, n, case["kind"]).astype(np.complex64) if first >= base else np.zeros(count, np.complex64)
            if doctor is not None:
                doctor(y, first)
            return y
        return fetch
    return run_exec


def test_one_non_zero_sample_in_transform_0_of_the_batch_2_case_fails():
    case = lp.MATRIX[21]
    n = case["n"]
    clean = lp.sweep(case, _reference_exec(case))
    assert clean["zero_failures"] == [] and clean["compared"] == lp.compared_outputs(case) and clean["combs"] == []
    assert 0 < clean["worst"] < 1.5e-7 and lp.check(case, clean, dict(clean)) == []      # complex64 rounding of the reference
    assert "no recorded entry" in lp.check(case, clean, None)[0]
    t = case["only"][3]
    start = int(lp.window_starts(case)[t, 17])

    def doctor(y, first):
        if first == start:                                                   # that window of transform 0, in every exec that has it
            y[5] = 1e-30
    got = lp.sweep(case, _reference_exec(case, doctor))
    bad = lp.check(case, got, dict(clean))
    assert got["worst"] == clean["worst"] and len(bad) >= 1 and "transform 0 of exec %d" % t in bad[0] and "not zero" in bad[0]
    assert lp.zero_failures(np.array([0.0, -0.0], dtype=np.complex64), 0, 0) == []
    assert lp.zero_failures(np.array([0.0, np.nan], dtype=np.complex64), 0, 0) != []
    # the impulses went into transform 1: its windows are read n samples further on
    seen = []
    lp.sweep(dict(case, only=[0]), lambda pos, amps: lambda first, count: seen.append(first) or np.zeros(count, np.complex64))
    assert sorted(seen) == sorted([int(s) + b * n for b in (0, 1) for s in lp.window_starts(case)[0]])


# ---- (e) the reference evaluators ---------------------------------------------------------------------------------------
def test_the_references_run_at_2_30_without_anything_of_size_n_and_match_the_closed_form():
    row = lp.row_named("p1gen_2^30")
    n, R, N1 = row["n"], row["R"], row["lengths"][0]
    assert n == 1 << 30
    (_, p, g), starts = lp.combs(row)[1], lp.comb_window_starts(row)[1]
    ks = lp.window_indices(starts)
    pos, win = lp.positions(row), lp.window_starts(row)
    tracemalloc.start()
    try:
        comb = {kind: lp.comb_reference(p, g, ks, n, kind) for kind in ("Forward", "Onlyinverse")}
        imp = lp.impulse_reference(pos[-1], lp.window_indices(win[-1]), n, "Forward")
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert peak < n // 4, peak                                               # 256 MiB; one n-entry table is 16 GiB
    assert len(ks) == 1 << 14 and imp.shape == (34 * 2048,) and pos[-1] == n - 1
    # the impulse at n - 1 is W^(-k); its last output is W^(-(n - 1)) = W
    assert np.abs(imp - np.exp(2j * np.pi * lp.window_indices(win[-1]) / n)).max() < 1e-12
    # closed form of a column comb: W_n^(r k) DFT_N1(g)[k mod N1], both directions
    r = int(p[0])
    assert np.array_equal(p, r + R * np.arange(N1))
    g64 = g.astype(np.complex128)
    phase = (r * ks % n) * (2.0 * np.pi / n)
    fwd = np.exp(-1j * phase) * np.fft.fft(g64)[ks % N1]
    inv = np.exp(1j * phase) * (np.fft.ifft(g64) * N1)[ks % N1]
    scale = np.abs(fwd).max()
    assert np.abs(comb["Forward"] - fwd).max() < 1e-11 * scale and np.abs(comb["Onlyinverse"] - inv).max() < 1e-11 * scale
    assert np.abs(comb["Forward"]).max() > 10                               # about sqrt(N1): a dense column, not a stray sample
