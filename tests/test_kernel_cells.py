"""not-gpu: the error-budget matrix (oracle/error_budget.py) runs every pass kernel of the tiled plans, in every form and in
every plan kind.

oracle/kernel_cells.py reads tests/golden/tiled_schedule.txt (pinned to schedule.h by tests/test_schedule.py) and maps a
(length, factors, flag setting) to its cells: one pass kernel at one length in one form.  The set of cells is stated here as
the rule the kernel limits of schedule.h give; the matrix must reach all of it.
"""
import pytest

from oracle import error_budget as eb
from oracle import kernel_cells as kc

KINDS = ("Forward", "Inverse", "Onlyinverse")


def _rule():
    """The reachable cells by the kernel limits, over 2^16 .. 2^28."""
    colsw_width = {8: 64, 9: 32}                                    # schedule.h colsw_width: 2^(14 - lg)
    a = {("A", "colsw", lg, ring) for lg, w in colsw_width.items() for ring in (0, w)}
    a |= {("A", "cols32", 11, 0), ("A", "p1gen", 10, 0)} | {("A", "tilec", lg, 0) for lg in range(6, 11)}
    b = {("B", "tilec", lg) for lg in range(6, 11)}
    # the tile ring: rows of at least 32 x the ring width, 1024 points and up (rows32_ring_supported)
    c = {("C", "rows32", lg, ring) for lg in range(9, 13) for ring in (0, 32, 64)
         if ring == 0 or (lg >= 10 and 1 << (lg - 5) >= ring)}
    c |= {("C", "tiler", lg, passes) for lg in range(6, 11) for passes in (2, 3)}
    return a | b | c


def test_all_cells_is_the_set_the_kernel_limits_give():
    cells = kc.all_cells()
    assert set(cells) == _rule() and len(cells) == 35
    # nothing new below 2^16 (no tiled plan) and, of these kernels, nothing new above 2^22
    assert max(lg for lg, _, _ in cells.values()) <= 22
    assert set(kc.all_cells(range(12, 31))) == _rule()
    for cell, (lg, factors, flags) in cells.items():
        assert cell in kc.cells_of(lg, factors, flags) and sum(factors) == lg
        # the smallest: no earlier (lg, factors, flag index) of the table reaches it
        assert not any(cell in kc.cells_of(l2, f2, i) for (l2, f2) in kc.parse_golden()[1] if 16 <= l2 <= lg
                       for i in range(16) if (l2, f2, i) < (lg, factors, flags)), kc.describe(cell)


def test_flag_index_and_cells_of_agree_with_the_golden_lines():
    assert kc.flag_index({"colsw": 1, "rows32": 0, "p1_gen": 0, "tile_ring": 1}) == 9
    # T 19 8,11,0 | tilec/-/rows32 0 2 0 5555 | colsw/-/rows32 0 2 1 aa | colsw/-/rows32 64 2 1 aa00
    assert kc.cells_of(19, (8, 11), 0) == (("A", "tilec", 8, 0), ("C", "rows32", 11, 0))
    assert kc.cells_of(19, (8, 11), 1) == (("A", "colsw", 8, 0), ("C", "rows32", 11, 0))
    assert kc.cells_of(19, (8, 11), 9) == (("A", "colsw", 8, 64), ("C", "rows32", 11, 64))
    assert kc.cells_of(19, (8, 11), {"colsw": 1, "rows32": 1, "p1_gen": 1, "tile_ring": 1}) == kc.cells_of(19, (8, 11), 9)
    # T 20 10,10,0 | tilec/-/tiler 0 2 0 303 | tilec/-/rows32 0 2 0 c0c | p1gen/-/tiler 0 2 0 3030 | p1gen/-/rows32 0 2 0 c0c0
    assert kc.cells_of(20, (10, 10), 4) == (("A", "p1gen", 10, 0), ("C", "tiler", 10, 2))
    assert kc.cells_of(20, (10, 10), 2) == (("A", "tilec", 10, 0), ("C", "rows32", 10, 0))
    assert kc.cells_of(24, (9, 7, 8), 15) == (("A", "colsw", 9, 0), ("B", "tilec", 7), ("C", "tiler", 8, 3))
    with pytest.raises(KeyError):
        kc.cells_of(20, (5, 15), 0)                                 # "factors" refuses it
    assert kc.unpack_factors(eb._f(6, 9, 6)) == (6, 9, 6) and kc.unpack_factors(eb._f(8, 11)) == (8, 11)


def test_every_cell_is_run_in_every_plan_kind():
    missing = kc.uncovered(eb.MATRIX, KINDS)
    assert not missing, "no case of the error-budget matrix runs: " + "; ".join(
        "%s in %s (smallest shape: 2^%d, factors %s, flag index %d)" % ((kc.describe(c), k) + kc.all_cells()[c]) for c, k in missing)


def test_tiled_cases_name_the_kernels_they_run():
    tiled = [c for c in eb.MATRIX if c["path"] == kc.PATH_TILED]
    assert len(tiled) >= 3 * 29 and all(kc.cells_of_case(c) == () for c in eb.MATRIX if c["path"] != kc.PATH_TILED)
    for case in tiled:
        lg, factors, flags = kc.case_shape(case)
        cells = kc.cells_of_case(case)
        text = case["kernels"]
        assert eb._f(*factors) == case["factors"] and len(cells) == case["launches_per_exec"], case["id"]
        if {c[1] for c in cells} <= {"tilec", "tiler"} and "k_tile x %d" % len(cells) in text:
            names = []                                              # "k_tile x 3": every pass is the tile kernel
        else:
            names = [kc.kernel_text(c) for c in cells]
        assert all(name in text for name in names), (case["id"], text, names)
        # and no kernel the plan does not run: every k_... word of the text belongs to a cell
        said = {w.strip("(),:") for w in text.split() if w.startswith("k_")}
        assert said <= {kc.kernel_text(c).split()[0] for c in cells}, (case["id"], text, cells)
        ring = max(c[3] for c in cells if c[1] in ("colsw", "rows32")) if any(c[1] in ("colsw", "rows32") for c in cells) else 0
        assert ("tile ring" in text and "no tile ring" not in text) == (ring != 0), (case["id"], text, ring)


def test_new_rows_set_every_key_themselves_and_an_unset_flag_needs_a_default():
    case = next(c for c in eb.MATRIX if c["id"] == "ring64_2048_2^19x2/Inverse")
    assert list(case["tunables"]) == ["factors"] + list(kc.FLAG_KEYS) and case["batch"] == 2
    assert kc.case_shape(case) == (19, (8, 11), {"colsw": 1, "rows32": 0, "p1_gen": 0, "tile_ring": 1})
    # defaults: colsw as choose_path gives it for (lg, batch), 1 for the other three
    dflt = next(c for c in eb.MATRIX if c["id"] == "colsw_9_2^19x3/Forward")
    assert kc.case_shape(dflt) == (19, (9, 10), {"colsw": 1, "rows32": 1, "p1_gen": 1, "tile_ring": 1})
    few = next(c for c in eb.MATRIX if c["id"] == "tile_2^16x4/Forward")
    assert kc.case_shape(few)[2]["colsw"] == 0
    # a batch the golden has no choose_path line for: refused unless the case decides everything itself
    odd = dict(dflt, id="odd", batch=11)
    with pytest.raises(ValueError, match="no choose_path line"):
        kc.cells_of_case(odd)
    with pytest.raises(ValueError, match="no choose_path line"):
        kc.cells_of_case(dict(odd, tunables={"factors": eb._f(9, 10)}))
    assert kc.cells_of_case(dict(case, batch=11)) == kc.cells_of_case(case)
    # the default plan of 2^20 x 4 is the pipeline: a case that calls it tiled without "factors" is refused
    with pytest.raises(ValueError, match="takes path 1"):
        kc.cells_of_case(dict(dflt, id="p", n=1 << 20, batch=4, tunables={}))


@pytest.mark.parametrize("row,kind,cell", [
    ("rows_tile_7_2^16x4", "Inverse", ("C", "tiler", 7, 2)),
    ("mid_tile_10_2^22x2", "Forward", ("B", "tilec", 10)),
    ("ring32_4096_2^21x2", "Onlyinverse", ("C", "rows32", 12, 32)),
    ("cols32_2^23x1", "Forward", ("A", "cols32", 11, 0)),
])
def test_coverage_reports_the_cell_of_a_removed_row(row, kind, cell):
    assert any(c["case"] == row and c["kind"] == kind for c in eb.MATRIX)
    assert kc.uncovered([c for c in eb.MATRIX if not (c["case"] == row and c["kind"] == kind)], KINDS) == [(cell, kind)]
    gone = kc.uncovered([c for c in eb.MATRIX if c["case"] != row], KINDS)
    assert gone == [(cell, k) for k in KINDS]
