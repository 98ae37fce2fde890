"""Which pass kernels a tiled (path 7) plan launches, read from the pinned decision table (TEST INFRASTRUCTURE ONLY, HIP-free).

resolve_tiled (fft_wgpu_amd/csrc/schedule.h) picks the kernel of every pass from the transform length, the "factors" key,
the flag keys "colsw" / "rows32" / "p1_gen" / "tile_ring" and the pass position.  tests/golden/tiled_schedule.txt lists
every such decision and tests/test_schedule.py pins it to the header; this module reads that file, so it restates none of
the header's logic.

A *cell* is one pass kernel in one form that is its own code (a template instantiation, or a branch on the slab layout or
on the pass count):
  ("A", kernel, log2 length, ring width)   colsw 8 / 9 x {matrix layout 0, tile ring 64 / 32}, cols32 11, p1gen 10, tilec 6..10
  ("B", "tilec", log2 length)              6..10
  ("C", "rows32", log2 length, ring width) 9..12 x {0, 32, 64} where the ring exists
  ("C", "tiler", log2 length, passes)      6..10 x {2, 3}: d1_count == 1 or the middle factor
Kernel names are the golden's: colsw, cols32, p1gen, tilec (k_tile columns), rows32, tiler (k_tile rows).

oracle/error_budget.py's matrix is mapped to cells with `cells_of_case`; tests/test_kernel_cells.py demands that every
cell of `all_cells()` is run by some case of the matrix in every plan kind.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiled_schedule.txt")

# the lengths whose decisions can differ by kernel form: below 2^16 there is no tiled plan, above 2^28 the 32-bit-offset
# kernels (colsw, cols32, rows32) leave and only k_tile / k_p1_gen remain.  The decisions there name no new cell, but the code
# is not all met below: from 2^29 pass A as k_tile columns and the last pass as k_tile rows run in the 64-bit-pointer form
# (launch_tile: a tile spanning 2^32 bytes) and the four buffer descriptors of k_p1_gen address what one no longer could.
# Those forms, one row per accepted factor tuple of 2^29 and 2^30, belong to oracle/large_plans.py, not to this matrix.
LG_RANGE = range(16, 29)
FLAG_KEYS = ("colsw", "rows32", "p1_gen", "tile_ring")   # bit 0 .. 3 of a flag index, as schedule.h flag_setting
PATH_TILED = 7
# what fwa_plan_create leaves in the three flags choose_path does not decide (schedule.h TiledFlags); a "factors" re-tune
# assigns path and factors only (tuning.cpp), so the flags a plan was created with survive it
FLAG_DEFAULTS = {"rows32": 1, "p1_gen": 1, "tile_ring": 1}


def flag_index(flags):
    return sum((1 if flags[k] else 0) << i for i, k in enumerate(FLAG_KEYS))


def _factors(text):
    f = tuple(int(v) for v in text.split(","))
    return f[:2] if f[2] == 0 else f


def unpack_factors(packed):
    """the "factors" key (log2 N1 | log2 N2 << 8 | log2 N3 << 16) -> (a, b) or (a, b, c)"""
    f = (packed & 255, packed >> 8 & 255, packed >> 16 & 255)
    return f[:2] if f[2] == 0 else f


_parsed = None


def parse_golden(path=GOLDEN):
    """-> (defaults, table).  defaults[(lg, batch)] = (path, factors, colsw) of choose_path (the D lines);
    table[(lg, factors)] = the 16 decisions (pass A, pass B, pass C, ring width, passes) by flag index, for every factor
    tuple the "factors" key accepts (the T lines that are not "invalid")."""
    global _parsed
    if path == GOLDEN and _parsed is not None:
        return _parsed
    defaults, table = {}, {}
    with open(path) as f:
        for ln in f:
            w = ln.split()
            if not w or w[0] == "#":
                continue
            if w[0] == "D":
                got = (int(w[3]), _factors(w[4]), int(w[5]))
                assert defaults.setdefault((int(w[1]), int(w[2])), got) == got, ln
            elif w[0] == "T" and w[3] != "invalid":
                by_flag = [None] * 16
                for part in ln.split(" | ")[1:]:
                    kernels, ring, passes, _swizzle, mask = part.split()
                    a, b, c = kernels.split("/")
                    for i in range(16):
                        if int(mask, 16) >> i & 1:
                            assert by_flag[i] is None, ln
                            by_flag[i] = (a, b, c, int(ring), int(passes))
                assert None not in by_flag, ln
                table[(int(w[1]), _factors(w[2]))] = by_flag
    if path == GOLDEN:
        _parsed = (defaults, table)
    return defaults, table


def cells_of(lg, factors, flags):
    """The cells of a tiled plan of 2^lg points with these factors ((a, b) or (a, b, c), log2 each); `flags` is a flag index
    0 .. 15 or a dict of the four flag keys.  KeyError for factors the "factors" key refuses."""
    i = flags if isinstance(flags, int) else flag_index(flags)
    factors = tuple(factors)
    a, b, c, ring, passes = parse_golden()[1][(lg, factors)][i]
    assert passes == len(factors) and (b == "-") == (passes == 2)
    cells = [("A", a, factors[0], ring if a == "colsw" else 0)]
    if passes == 3:
        cells.append(("B", b, factors[1]))
    cells.append(("C", c, factors[-1], ring) if c == "rows32" else ("C", c, factors[-1], passes))
    return tuple(cells)


def all_cells(lgs=LG_RANGE):
    """{cell: the smallest (lg, factors, flag index) that reaches it}: lowest lg, then factors, then flag index."""
    table = parse_golden()[1]
    out = {}
    for lg, factors in sorted(k for k in table if k[0] in lgs):
        for i in range(16):
            for cell in cells_of(lg, factors, i):
                out.setdefault(cell, (lg, factors, i))
    return out


def case_shape(case):
    """An error-budget case (a row of oracle.error_budget.MATRIX) -> (lg, factors, flags dict) of the plan it runs, or None
    when the case is not a tiled plan.  A flag or the factors the case leaves unset are the plan's defaults for its
    (lg, batch), from the golden's D lines; ValueError where there is no such line."""
    if case["path"] != PATH_TILED:
        return None
    lg = case["n"].bit_length() - 1
    tun = case["tunables"]
    default = parse_golden()[0].get((lg, case["batch"]))
    if default is None and ("factors" not in tun or "colsw" not in tun):
        raise ValueError("%s: no choose_path line for 2^%d x %d in %s: the case must set \"factors\" and all of %s itself"
                         % (case["id"], lg, case["batch"], os.path.relpath(GOLDEN, ROOT), ", ".join(FLAG_KEYS)))
    if "factors" in tun:
        factors = unpack_factors(tun["factors"])
    else:
        if default[0] != PATH_TILED:
            raise ValueError("%s: the default plan of 2^%d x %d takes path %d, not the tiled path" % (case["id"], lg, case["batch"], default[0]))
        factors = default[1]
    flags = dict(FLAG_DEFAULTS, colsw=default[2] if default else None)
    flags.update({k: int(tun[k] != 0) for k in FLAG_KEYS if k in tun})
    return lg, factors, flags


def cells_of_case(case):
    shape = case_shape(case)
    return () if shape is None else cells_of(*shape)


def kernel_text(cell):
    """the name a case's `kernels` text gives this cell's kernel"""
    kernel, lg_l = cell[1], cell[2]
    return {"colsw": "k_colsw<%d,%d>" % (lg_l, 1 << (14 - lg_l)), "cols32": "k_cols32<%d>" % lg_l, "p1gen": "k_p1_gen",
            "tilec": "k_tile columns", "rows32": "k_rows32<%d>" % lg_l, "tiler": "k_tile rows"}[kernel]


def describe(cell):
    if cell[0] == "B":
        return "B tilec<%d>" % cell[2]
    if cell[1] == "tiler":
        return "C tiler<%d>, %s" % (cell[2], "two-pass" if cell[3] == 2 else "three-pass")
    tail = ", ring %d" % cell[3] if cell[3] else (", matrix" if cell[1] in ("colsw", "rows32") else "")
    return "%s %s<%d>%s" % (cell[0], cell[1], cell[2], tail)


def uncovered(matrix, kinds=("Forward", "Inverse", "Onlyinverse")):
    """[(cell, kind)] of all_cells() x kinds that no case of `matrix` runs, in all_cells()'s order."""
    ran = {(cell, case["kind"]) for case in matrix for cell in cells_of_case(case)}
    return [(cell, kind) for cell in all_cells() for kind in kinds if (cell, kind) not in ran]
