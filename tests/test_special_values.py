"""not-gpu: the special-value checks of oracle/special_values.py accept the reference and reject doctored results.

tests/test_gpu_special_values.py holds every kernel to three exact properties: NaN in one input sample reaches every
output of its transform, no other transform of the batch changes a bit, and an input times 2^s gives the result times
2^s bit for bit.  Here the reference's own arithmetic (oracle.forward_ref / inverse_ref / onlyinverse_ref /
normalize_ref) runs on the exact batch layouts of the GPU rows and every check must stay silent: the standing proof that
inputs and scales were chosen so that the reference alone meets every condition, and a failure on the GPU is the kernel's.
Then each check is shown to see the smallest departure it exists for.
"""
import numpy as np
import pytest

from oracle import error_budget as eb
from oracle import kernel_cells as kc
from oracle import special_values as sv

REF = {"Forward": "forward_ref", "Inverse": "inverse_ref", "Onlyinverse": "onlyinverse_ref"}


def _row_at(n):
    """the first row of that length: a non-tiled one where there is one"""
    return next(r for r in sv.ROWS if r["n"] == n)


def _reference_results(oracle, layout, kind):
    n = layout["n"]
    ref = lambda x: getattr(oracle, REF[kind])(x, n)[0]
    x = sv.clean_input(oracle, layout)
    xs = sv.scaling_input(x, layout)
    return ref(x), ref(sv.poisoned_input(x, layout)), {s: ref(sv.scaled(xs, s)) for s in sv.SCALES}


@pytest.fixture(scope="module")
def results_1k(oracle):
    """the five reference results of the 2^10 row in Forward, shared (and left unchanged) by the doctoring tests"""
    layout = _row_at(1 << 10)["layout"]
    return (layout,) + _reference_results(oracle, layout, "Forward")


# ---- the check functions accept the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(n, k) for n in (2, 32, 256, 1 << 10, 1 << 13, 1 << 16) for k in REF] + [(1 << 20, "Forward")],
                         ids=lambda v: v if isinstance(v, str) else "2^%d" % (v.bit_length() - 1))
def test_checks_accept_the_reference_on_the_gpu_rows_layout(oracle, n, kind):
    row = _row_at(n)
    layout = row["layout"]
    assert layout["n"] == n and layout["batch"] == row["batch"]
    y_clean, y_poison, y_scaled = _reference_results(oracle, layout, kind)
    assert sv.check_results(layout, y_clean, y_poison, y_scaled) == []
    # the ragged layout: the clean and the poisoned exec
    ragged = row["ragged"]["layout"]
    ref = lambda x: getattr(oracle, REF[kind])(x, n)[0]
    x = sv.clean_input(oracle, ragged)
    assert ragged["batch"] == row["ragged"]["batch"] and x.size == n * ragged["batch"]
    assert sv.check_poison(ref(sv.poisoned_input(x, ragged)), ref(x), ragged) == []
    # nothing vacuous: the scaled inputs are exact and normal, and the results are neither all zero nor subnormal anywhere
    xs = sv.scaling_input(sv.clean_input(oracle, layout), layout).view(np.float32)
    tiny = float(np.finfo(np.float32).tiny)
    for s in sv.SCALES:
        a = np.abs(sv.scaled(xs.view(np.complex64), s).view(np.float32)).astype(np.float64)
        assert np.array_equal(a, np.abs(xs).astype(np.float64) * 2.0 ** s) and (a[a > 0] >= tiny).all()
        r = np.abs(y_scaled[s].view(np.float32))
        assert r.max() > 0 and (r[r > 0] >= tiny).all()


@pytest.mark.parametrize("n,batch", sv.NORMALIZE_ROWS)
def test_normalize_checks_accept_the_reference(oracle, n, batch):
    x = sv.normalize_input(oracle, n, batch)
    f = x.view(np.float32)
    spots = sv.normalize_spots(n, batch)
    assert len(spots) == len(set(spots)) >= 9 and all(0 <= i < n * batch and not 2 * n <= i < 3 * n for i in spots)
    assert {0, n - 1, n, 8191, 8192, n * batch - 1} <= set(spots)
    bad = np.flatnonzero(~(np.isfinite(x.real) & np.isfinite(x.imag)))
    assert sorted(spots) == bad.tolist()                            # one pattern per spot, none overwritten
    assert np.isnan(f).sum() >= 5 and np.isinf(f).sum() >= 6 and (x[2 * n:3 * n] == 0).all()
    assert not np.isfinite(f[-2 * n:]).all()                       # a special inside the last transform (the ragged workgroup)
    assert sv.check_normalize(oracle.normalize_ref(x, n), x, oracle.normalize_ref(x, n)) == []
    xs = sv.normalize_scaling_input(x)
    assert np.isfinite(xs.view(np.float32)).all() and (xs.view(np.float32)[np.isfinite(f)] == f[np.isfinite(f)]).all()
    y_1 = oracle.normalize_ref(xs, n)
    for s in sv.SCALES:
        assert sv.check_scaling(oracle.normalize_ref(sv.scaled(xs, s), n), y_1, s) == []


# ---- the check functions reject doctored results --------------------------------------------------------------------
def _special(layout, what):
    return next((t, p) for t, w, p in layout["specials"] if w == what)


def test_one_finite_float_inside_a_nan_transform_is_reported(results_1k):
    layout, y_clean, y_poison, _ = results_1k
    n = layout["n"]
    t, _ = _special(layout, sv.NAN)
    y = y_poison.copy()
    y.view(np.float32)[2 * (t * n + 700) + 1] = 0.5
    bad = sv.check_poison(y, y_clean, layout)
    assert len(bad) == 1 and "transform %d" % t in bad[0] and "output 700 (im)" in bad[0] and "never read" in bad[0]


def test_one_flipped_low_bit_in_a_clean_neighbour_is_reported(results_1k):
    layout, y_clean, y_poison, _ = results_1k
    n = layout["n"]
    for t in (0, 2, layout["batch"] - 1):
        y = y_poison.copy()
        y.view(np.uint32)[2 * (t * n + 3)] ^= 1
        bad = sv.check_poison(y, y_clean, layout)
        assert len(bad) == 1 and "clean transform %d" % t in bad[0] and "output 3" in bad[0], bad


def test_a_tiny_addend_in_the_zero_transform_is_reported(results_1k):
    layout, y_clean, y_poison, _ = results_1k
    n = layout["n"]
    t, _ = _special(layout, sv.ZERO)
    assert sv.check_poison(y_poison, y_clean, layout) == []
    y = y_poison.copy()
    y[t * n:(t + 1) * n] += np.float32(1e-30)
    bad = sv.check_poison(y, y_clean, layout)
    assert len(bad) == 1 and "all zero" in bad[0]
    y = y_poison.copy()
    y.view(np.float32)[2 * t * n:2 * (t + 1) * n] = -0.0             # compared by value: either sign of zero is zero
    assert sv.check_poison(y, y_clean, layout) == []


def test_an_inf_transform_with_one_finite_sample_is_reported(results_1k):
    layout, y_clean, y_poison, _ = results_1k
    n = layout["n"]
    t, _ = _special(layout, sv.INF)
    y = y_poison.copy()
    y[t * n + 9] = 1 + 2j
    bad = sv.check_poison(y, y_clean, layout)
    assert len(bad) == 1 and "finite in both parts" in bad[0] and "output 9" in bad[0]
    y.view(np.float32)[2 * (t * n + 9)] = np.inf                    # one part not finite is enough
    assert sv.check_poison(y, y_clean, layout) == []


@pytest.mark.parametrize("s", sv.SCALES)
def test_a_scaled_result_with_one_mantissa_bit_changed_or_one_inf_is_reported(results_1k, s):
    layout, y_clean, y_poison, y_scaled = results_1k
    y_1 = sv.scaling_reference(y_clean, y_poison, layout)
    assert sv.check_scaling(y_scaled[s], y_1, s) == []
    y = y_scaled[s].copy()
    y.view(np.uint32)[12345] ^= 1
    bad = sv.check_scaling(y, y_1, s)
    assert len(bad) == 1 and "differ" in bad[0] and "float 12345" in bad[0]
    y = y_scaled[s].copy()
    y.view(np.float32)[77] = np.inf
    bad = sv.check_scaling(y, y_1, s)
    assert len(bad) == 2 and "not finite" in bad[0] and "float 77" in bad[0]
    # an overflow of the expectation itself is not an excuse: inf wanted and inf got still fails as not finite
    big = np.full(4, 3e38, dtype=np.float32).view(np.complex64)
    assert any("not finite" in m for m in sv.check_scaling(np.full(4, np.inf, dtype=np.float32).view(np.complex64), big, 40))


def test_a_normalize_output_with_its_nan_one_sample_off_is_reported(oracle):
    n, batch = sv.NORMALIZE_ROWS[1]
    x = sv.normalize_input(oracle, n, batch)
    ref = oracle.normalize_ref(x, n)
    y = np.roll(ref, 1)
    bad = sv.check_normalize(y, x, ref)
    assert any("NaN pattern" in m for m in bad) and any("Inf pattern" in m for m in bad)
    y = ref.copy()
    i = int(np.flatnonzero(np.isnan(x.real) & np.isnan(x.imag))[0])
    y[i], y[i + 1] = ref[i + 1], ref[i]                              # the NaN one sample off, nothing else changed
    bad = sv.check_normalize(y, x, ref)
    assert bad and all("pattern" in m or "finite floats differ" in m for m in bad) and any("NaN pattern" in m for m in bad)
    y = ref.copy()
    y.view(np.uint32)[2 * 4000] ^= 1
    assert len(sv.check_normalize(y, x, ref)) == 1
    y = ref.copy()
    k = int(np.flatnonzero(np.isposinf(x.view(np.float32)))[0])
    y.view(np.float32)[k] = -np.inf                                  # the sign of an Inf is part of the pattern
    assert any("Inf pattern" in m for m in sv.check_normalize(y, x, ref))


# ---- coverage -------------------------------------------------------------------------------------------------------
def test_tiled_rows_run_every_cell_in_every_plan_kind():
    tiled = [c for c in sv.MATRIX if c["path"] == kc.PATH_TILED]
    assert kc.uncovered(tiled, ("Forward", "Inverse", "Onlyinverse")) == []
    cells = kc.all_cells()
    assert len(cells) == 35 and max(lg for lg, _, _ in cells.values()) <= 22
    shapes = sorted(set(cells.values()))
    rows = [r for r in sv.ROWS if r["path"] == kc.PATH_TILED]
    assert len(rows) == len(shapes) and all(r["n"] <= 1 << 22 for r in rows)
    for r, (lg, factors, flags) in zip(rows, shapes):
        tun = r["tunables"]
        # the row decides the kernel of every pass itself: "factors" and the four flags, then the geometry
        assert list(tun) == ["factors"] + list(kc.FLAG_KEYS) + ["group", "streams"], r["case"]
        assert r["n"] == 1 << lg and tun["factors"] == eb.pack_factors(*factors) == r["factors"]
        assert kc.flag_index({k: tun[k] for k in kc.FLAG_KEYS}) == flags
        assert (tun["group"], tun["streams"], r["batch"]) == (2, 2, 7)
        assert r["launches_per_exec"] == len(factors) * 4             # passes x groups: 7 transforms in groups of 2
        assert [t for t, _, _ in r["layout"]["specials"]] == [1, 3, 5]
        case = dict(r, id=r["case"], kind="Forward")
        assert all(kc.kernel_text(c) in r["kernels"] for c in kc.cells_of_case(case))
    # B tilec 8 and C tiler 9 (three passes) are reached well below the 2^25 / 2^26 rows of the error-budget matrix
    assert cells[("B", "tilec", 8)][0] <= 22 and cells[("C", "tiler", 9, 3)][0] <= 22


def test_every_non_tiled_row_is_present_with_its_layout():
    rows = {r["budget_row"]: r for r in sv.ROWS if r["budget_row"]}
    want = (["chunk_%d" % (1 << lg) for lg in range(1, 9)] + ["small32_%d" % lg for lg in range(9, 16)]
            + ["literal_2^10", "pipeline_2^20x4"])
    assert list(rows) == want == list(sv.NON_TILED)
    for name, r in rows.items():
        c = eb.case_row(name)
        n, tun, path, factors, passes = c["n"], c["tunables"], c["path"], c["factors"], c["passes"]
        assert (r["n"], r["path"], r["factors"]) == (n, path, factors)
        lay = r["layout"]
        where = [t for t, _, _ in lay["specials"]]
        what = [w for _, w, _ in lay["specials"]]
        if n < 1 << 16:
            batch = r["batch"]
            assert batch == max(9, eb.samples(n) | 1) and batch % 2 == 1 and batch * n >= eb.MIN_SAMPLES
            assert r["tunables"] == tun and r["launches_per_exec"] == passes
            assert where == [1, 3, 5, batch - 2] and what == [sv.NAN, sv.INF, sv.ZERO, sv.NAN]
        else:
            assert name == "pipeline_2^20x4" and r["batch"] == 7 and r["path"] == 1 and r["launches_per_exec"] == 2 * 4
            assert r["tunables"] == {"group": 2, "streams": 2} and where == [1, 3, 5]
        assert all(t % 2 == 1 and 0 < t < r["batch"] - 1 for t in where)    # clean neighbours on both sides
    ids = [c["id"] for c in sv.MATRIX]
    assert len(ids) == len(set(ids)) == 3 * len(sv.ROWS)
    assert eb.case_row("pipeline_2^20x4") == dict(case="pipeline_2^20x4", n=1 << 20, batch=4, tunables={}, path=1,
                                                  factors=eb.pack_factors(10, 10), passes=2, kernels="k_p1_1m + k_p2_1m")


def _unit_of(row, layout, tunables, t):
    """(index of the workgroup or group that holds transform t, transforms per unit)"""
    per = tunables["group"] if "group" in tunables else sv.transforms_per_workgroup(row["n"])
    return t // per, per


def test_the_issue_layout_leaves_the_ragged_unit_clean_and_the_ragged_layout_does_not():
    """In the first layout the last, partly valid workgroup (one-launch kernels) or group (pipelined plans) holds the clean
    last transform alone; the ragged layout puts a NaN transform with a clean one on either side into it."""
    partial = []
    for r in sv.ROWS:
        if r["path"] == 2:
            continue        # the literal recurrence: one butterfly per thread, no unit that holds whole transforms
        n, batch, lay = r["n"], r["batch"], r["layout"]
        last, per = _unit_of(r, lay, r["tunables"], batch - 1)
        in_last = [t for t in range(batch) if _unit_of(r, lay, r["tunables"], t)[0] == last]
        assert not set(in_last) & {t for t, _, _ in lay["specials"]}, r["case"]
        # the ragged layout
        rg = r["ragged"]
        batch, lay, tun = rg["batch"], rg["layout"], rg["tunables"]
        t, what, p = lay["specials"][-1]
        assert (t, what) == (batch - 2, sv.NAN) and [s[0] for s in lay["specials"][:3]] == [1, 3, 5] and batch % 2 == 1
        assert {k: v for k, v in tun.items() if k != "group"} == {k: v for k, v in r["tunables"].items() if k != "group"}
        last, per = _unit_of(r, lay, tun, batch - 1)
        in_last = [u for u in range(batch) if _unit_of(r, lay, tun, u)[0] == last]
        if "group" in tun:
            assert (batch, tun["group"], tun["streams"]) == (11, 4, 2) and in_last == [8, 9, 10]
            assert rg["launches_per_exec"] == r["launches_per_exec"] // 4 * 3       # passes x 3 groups
        else:
            assert batch == eb.samples(n) + 3 and rg["launches_per_exec"] == r["launches_per_exec"]
            if per < 4:
                assert n >= 1 << 12                                  # one or two transforms per workgroup: raggedness is moot
                continue
        assert in_last == [t - 1, t, t + 1] and len(in_last) < per, r["case"]       # partly valid, special in the middle
        partial.append(r["case"])
    one_launch = ["chunk_%d" % (1 << lg) for lg in range(1, 9)] + ["small32_%d" % lg for lg in range(9, 12)]
    assert partial[:len(one_launch)] == one_launch and len(partial) == len(one_launch) + 1 + 27
    # the workgroup sizes this rests on: k_chunk's 8192 samples, k_small32's XPW = 16, 8, 4, 2, 1, 1, 1 for 2^9 .. 2^15
    assert [sv.transforms_per_workgroup(1 << lg) for lg in range(9, 16)] == [16, 8, 4, 2, 1, 1, 1]
    assert all(sv.transforms_per_workgroup(1 << lg) << lg == 8192 for lg in range(1, 9))


def test_poisoned_sample_moves_over_first_last_and_interior():
    seen = {sv.NAN: set(), sv.INF: set()}
    for r in sv.ROWS:
        n = r["n"]
        for j, (t, what, p) in enumerate(r["layout"]["specials"]):
            if what == sv.ZERO:
                assert p is None
                continue
            assert 0 <= p < n
            seen[what].add("first" if p == 0 else "last" if p == n - 1 else "interior")
            if j == 3:
                assert n == 2 or 0 < p < n - 1
        ps = [p for _, w, p in r["layout"]["specials"][:3] if w != sv.ZERO]
        assert ps[0] != ps[1]
    assert seen[sv.NAN] == seen[sv.INF] == {"first", "last", "interior"}
    x = np.arange(1, 2 * 2 * 9 + 1, dtype=np.float32).view(np.complex64)     # 9 transforms of 2 points
    lay = sv.make_layout(2, 9, 0, True)
    xp = sv.poisoned_input(x, lay)
    for t, what, p in lay["specials"]:
        got = xp[2 * t:2 * t + 2]
        if what == sv.ZERO:
            assert (got == 0).all()
        else:
            v = got[p]
            assert (np.isnan(v.real) and np.isnan(v.imag)) if what == sv.NAN else (v.real == np.inf and v.imag == -np.inf)
            assert got[1 - p] == x[2 * t + 1 - p]
    clean = [t for t in range(9) if t not in {s[0] for s in lay["specials"]}]
    assert all((xp[2 * t:2 * t + 2] == x[2 * t:2 * t + 2]).all() for t in clean)
