#!/usr/bin/env python3
"""tools/error_budget_mutants.py [build|run|all] [--only M1,M4] [--control] [--out FILE] -- evidence that the error budget
(oracle/error_budget.py) catches twiddle errors the flat 1e-5 bound lets through.

build: the copy-and-substitute build of tools/mutant_build.py: fft_wgpu_amd/csrc copied to build/variants/<mutant>/csrc, the
       mutant's textual substitutions applied (each must match exactly once), `make lab`.
run:   for each mutant, tools/record_error_budget.py --lab in a fresh child process with FWA_LAB_LIBRARY pointing at the
       mutant's laboratory library (under a time limit), then the budget's rule against the committed record.  One JSON
       line per mutant: worst max_rel / rel_l2 (and whether the old 1e-5 bound passes), the cases the budget rejects.
       --control first runs the tree's own laboratory library the same way (it must be rejected nowhere).  A child that
       fails (fault, abort, time limit) ends the run: nothing more is started on the device.

Every mutant is numerical only: it changes twiddle values, never an index into a buffer.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import error_budget as eb  # noqa: E402
from tools.mutant_build import TREE_LAB_LIBRARY, VARIANTS, build, lib_path  # noqa: E402

# name: (what it models, [(file, old, new), ...])
MUTANTS = {
    "M1": ("tw_f64: angle and cos / sin evaluated in float", [
        ("tables.cpp",
         "    const double theta = -2.0 * PI * (double)k / (double)n;\n"
         "    return v2f{(float)std::cos(theta), (float)std::sin(theta)};",
         "    const float theta = -2.0f * (float)PI * (float)k / (float)n;\n"
         "    return v2f{std::cos(theta), std::sin(theta)};")]),
    "M2": ("tw_f64: pi rounded to the f32 constant", [
        ("tables.cpp", "const double PI = 3.14159265358979323846;", "const double PI = (double)3.14159265358979323846f;")]),
    "M3": ("upload_level: hi[j] = W_cur^(1024 j + 1), one index off in the high level of every two-level table", [
        ("tables.cpp", "h[j] = tw_f64(1024 * j, cur);", "h[j] = tw_f64(1024 * j + 1, cur);")]),
    "M4": ("2^20 pipeline outer table: A[k1][c] = W_N^(n2 k + (k > 0))", [
        ("tables.cpp", "= tw_f64(n2 * k, N);                // A[k1][c]", "= tw_f64(n2 * k + (k > 0), N);                // A[k1][c]")]),
    "M5": ("cplx.h: constexpr Taylor series of tw_const cut from 12 to 4 terms", [
        ("cplx.h", "for (int i = 1; i < 12; ++i) { t *= -x2 / ((2 * i) * (2 * i + 1));",
         "for (int i = 1; i < 4; ++i) { t *= -x2 / ((2 * i) * (2 * i + 1));"),
        ("cplx.h", "for (int i = 1; i < 12; ++i) { t *= -x2 / ((2 * i - 1) * (2 * i));",
         "for (int i = 1; i < 4; ++i) { t *= -x2 / ((2 * i - 1) * (2 * i));")]),
}


def run(name, lib, record, timeout):
    """one child process: the whole matrix on `lib` -> a JSON-able summary, or None when the child failed."""
    out = os.path.join(VARIANTS, name, "measured.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    env = dict(os.environ, FWA_LAB_LIBRARY=lib)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "record_error_budget.py"), "--lab", "--out", out]
    try:
        p = subprocess.run(cmd, env=env, timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        print("%s: time limit of %d s reached" % (name, timeout), flush=True)
        return None
    if p.returncode not in (0, 1):          # 1: a plan drifted from the matrix (reported below); anything else: stop
        print("%s: child exited with %d\n%s\n%s" % (name, p.returncode, p.stdout[-3000:], p.stderr[-3000:]), flush=True)
        return None
    got = eb.load_record(out)["cases"]
    rejected, messages = [], []
    for case in eb.MATRIX:
        bad = eb.check(case, got[case["id"]], record["cases"].get(case["id"]))
        if bad:
            rejected.append(case["id"])
            messages += bad
    worst_mx = max(eb.MATRIX, key=lambda c: got[c["id"]]["max_rel"])
    worst_l2 = max(eb.MATRIX, key=lambda c: got[c["id"]]["rel_l2"])
    worst_cap = max(eb.MATRIX, key=lambda c: got[c["id"]]["rel_l2"] / eb.cap(c["n"]))
    drift = [c["id"] for c in eb.MATRIX if any(got[c["id"]][k] != c[k] for k in ("path", "factors", "launches_per_exec"))]
    return {
        "mutant": name, "what": MUTANTS[name][0] if name in MUTANTS else "unmutated laboratory build (control)",
        "substitutions": [{"file": f, "old": o, "new": n} for f, o, n in MUTANTS.get(name, (None, []))[1]],
        "worst_max_rel": got[worst_mx["id"]]["max_rel"], "worst_max_rel_case": worst_mx["id"],
        "worst_rel_l2": got[worst_l2["id"]]["rel_l2"], "worst_rel_l2_case": worst_l2["id"],
        "worst_rel_l2_over_cap": got[worst_cap["id"]]["rel_l2"] / eb.cap(worst_cap["n"]), "worst_over_cap_case": worst_cap["id"],
        "passes_flat_1e-5": all(got[c["id"]]["max_rel"] <= 1e-5 and got[c["id"]]["rel_l2"] <= 1e-5 for c in eb.MATRIX),
        "cases": len(eb.MATRIX), "budget_rejects": len(rejected), "caught": bool(rejected), "rejected_cases": rejected,
        "messages": messages[:40], "plan_drift": drift,
        "record_commit": record["stamp"]["commit"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("build", "run", "all"))
    ap.add_argument("--only", default="", help="comma-separated mutant names (default: all)")
    ap.add_argument("--control", action="store_true", help="run the unmutated laboratory build first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round7", "error_budget_mutants.jsonl"))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    args = ap.parse_args()
    names = [m for m in args.only.split(",") if m] or list(MUTANTS)
    if args.what in ("build", "all"):
        for name in names:
            build(name, MUTANTS[name][1])
    if args.what == "build":
        return
    record = eb.load_record()
    todo = ([("control", TREE_LAB_LIBRARY)] if args.control else []) + \
        [(m, lib_path(m)) for m in names]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, lib in todo:
            res = run(name, lib, record, args.timeout)
            if res is None:
                raise SystemExit("stopped after %s: nothing more is started on the device" % name)
            f.write(json.dumps(res) + "\n")
            f.flush()
            print("%s: worst max_rel %.3g (%s), worst rel_l2 %.3g; flat 1e-5 %s; budget rejects %d of %d cases%s" % (
                name, res["worst_max_rel"], res["worst_max_rel_case"], res["worst_rel_l2"],
                "passes" if res["passes_flat_1e-5"] else "FAILS", res["budget_rejects"], res["cases"],
                (": " + ", ".join(res["rejected_cases"][:12]) + (" ..." if len(res["rejected_cases"]) > 12 else ""))
                if res["rejected_cases"] else ""), flush=True)


if __name__ == "__main__":
    main()
