#!/usr/bin/env python3
"""tools/impulse_mutants.py [build|run|all] [--only S1,S4] [--control] [--out FILE] -- evidence that the impulse sweeps
(oracle/impulse_sweep.py) catch twiddle errors in few places, which the error budget (oracle/error_budget.py) lets through.

build: the copy-and-substitute build of tools/mutant_build.py, one textual substitution per mutant, `make lab`.
run:   for each mutant two fresh child processes with FWA_LAB_LIBRARY pointing at the mutant's laboratory library, each under
       a time limit: tools/record_error_budget.py --lab, then tools/record_impulse_response.py --lab; then both rules
       against the committed records.  One JSON line per mutant: the error-budget cases that reject it, the sweep cases
       that reject it and how far over their record the worst of them is.  --control first runs the tree's own laboratory
       library the same way (it must be rejected nowhere).  A child that fails (fault, abort, time limit) ends the run:
       nothing more is started on the device.

Every mutant is sparse and numerical only: it changes a few table values, never an index into a buffer.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import error_budget as eb  # noqa: E402
from oracle import impulse_sweep as im  # noqa: E402
from tools.mutant_build import TREE_LAB_LIBRARY, VARIANTS, build, lib_path  # noqa: E402

# name: (what it models, [(file, old, new)])
MUTANTS = {
    "S1": ("2^20 pipeline outer table: A[k1][c] one index off at the single entry tile 37, k1 = 5, c = 9 (column 601)", [
        ("tables.cpp", "= tw_f64(n2 * k, N);                // A[k1][c]",
         "= tw_f64(n2 * k + (tile == 37 && k == 5 && c == 9), N);                // A[k1][c]")]),
    "S2": ("2^20 pipeline outer table: B[k2][c] one index off only at column n2 = 1023, k2 = 31", [
        ("tables.cpp", "= tw_f64(32 * n2 * k, N);  // B[k2][c]", "= tw_f64(32 * n2 * k + (n2 == 1023 && k == 31), N);  // B[k2][c]")]),
    "S3": ("upload_level: only the last hi[] entry of every two-level table one index off", [
        ("tables.cpp", "h[j] = tw_f64(1024 * j, cur);", "h[j] = tw_f64(1024 * j + (nhi > 1 && j == nhi - 1), cur);")]),
    # S3 changes no output bit: every kernel looks W_cur^(col K1) up as a product of factors col x (a partial digit of K1), and the
    # largest such exponent lies below cur - 1024 (k_tile: col * 8 TPX <= (R - 1) L / 2, the last entry read is hi[nhi / 2 - 1])
    "S3b": ("upload_level: hi[nhi / 2 - 1], the last hi[] entry k_tile reads (col * 8 TPX at col = R - 1), one index off", [
        ("tables.cpp", "h[j] = tw_f64(1024 * j, cur);", "h[j] = tw_f64(1024 * j + (nhi > 1 && j == nhi / 2 - 1), cur);")]),
    "S4": ("upload_level: the interior entry lo[517] of every two-level table one index off", [
        ("tables.cpp", "l[j] = tw_f64(j, cur);", "l[j] = tw_f64(j + (j == 517), cur);")]),
    "S5": ("upload_half_table: the last entry of the 8192-point table one index off", [
        ("tables.cpp", "h[k] = tw_f64(k, n);", "h[k] = tw_f64(k + (n == 8192 && k == n / 2 - 1), n);")]),
}


def child(name, tool, out, lib, timeout):
    """one child process on `lib` -> the record it wrote, or None when the child failed"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--lab", "--out", out]
    try:
        p = subprocess.run(cmd, env=dict(os.environ, FWA_LAB_LIBRARY=lib), timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        print("%s: %s: time limit of %d s reached" % (name, tool, timeout), flush=True)
        return None
    if p.returncode not in (0, 1):          # 1: a plan drifted from its row (reported below); anything else: stop
        print("%s: %s exited with %d\n%s\n%s" % (name, tool, p.returncode, p.stdout[-3000:], p.stderr[-3000:]), flush=True)
        return None
    with open(out) as f:
        return json.load(f)["cases"]


def run(name, lib, budget_record, sweep_record, timeout):
    d = os.path.join(VARIANTS, name)
    budget = child(name, "record_error_budget.py", os.path.join(d, "measured_budget.json"), lib, timeout)
    if budget is None:
        return None
    swept = child(name, "record_impulse_response.py", os.path.join(d, "measured_impulse.json"), lib, timeout)
    if swept is None:
        return None
    budget_rejected = [c["id"] for c in eb.MATRIX if eb.check(c, budget[c["id"]], budget_record["cases"].get(c["id"]))]
    rejected, messages = [], []
    for c in im.MATRIX:
        bad = im.check(c, swept[c["id"]], sweep_record["cases"].get(c["id"]))
        if bad:
            rejected.append(c["id"])
            messages.append(bad[0])
    over = max(im.MATRIX, key=lambda c: swept[c["id"]]["worst"] / sweep_record["cases"][c["id"]]["worst"])
    drift = [c["id"] for c in eb.MATRIX if any(budget[c["id"]][k] != c[k] for k in ("path", "factors", "launches_per_exec"))] + \
        [c["id"] for c in im.MATRIX if (swept[c["id"]]["path"], swept[c["id"]]["factors"]) != (c["path"], c["factors"])]
    return {
        "mutant": name, "what": MUTANTS[name][0] if name in MUTANTS else "unmutated laboratory build (control)",
        "substitutions": [{"file": f, "old": o, "new": n} for f, o, n in MUTANTS.get(name, (None, []))[1]],
        "budget_cases": len(eb.MATRIX), "budget_rejects": len(budget_rejected), "budget_rejected_cases": budget_rejected,
        "budget_worst_max_rel": max(budget[c["id"]]["max_rel"] for c in eb.MATRIX),
        "sweep_cases": len(im.MATRIX), "sweep_rejects": len(rejected), "sweep_rejected_cases": rejected,
        "sweep_rejected_rows": sorted({i.split("/")[0] for i in rejected}, key=[r["case"] for r in im.ROWS].index),
        "sweep_worst_over_record": swept[over["id"]]["worst"] / sweep_record["cases"][over["id"]]["worst"],
        "sweep_worst_over_record_case": over["id"], "sweep_worst_there": swept[over["id"]]["worst"],
        "sweep_worst_at": {k: swept[over["id"]][k] for k in ("t", "p", "k")},
        "messages": messages[:12], "plan_drift": drift,
        "record_commits": [budget_record["stamp"]["commit"], sweep_record["stamp"]["commit"]],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("build", "run", "all"))
    ap.add_argument("--only", default="", help="comma-separated mutant names (default: all)")
    ap.add_argument("--control", action="store_true", help="run the unmutated laboratory build first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round7", "impulse_mutants.jsonl"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    args = ap.parse_args()
    names = [m for m in args.only.split(",") if m] or list(MUTANTS)
    if args.what in ("build", "all"):
        for name in names:
            build(name, MUTANTS[name][1])
    if args.what == "build":
        return
    budget_record, sweep_record = eb.load_record(), im.load_record()
    todo = ([("control", TREE_LAB_LIBRARY)] if args.control else []) + [(m, lib_path(m)) for m in names]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, lib in todo:
            res = run(name, lib, budget_record, sweep_record, args.timeout)
            if res is None:
                raise SystemExit("stopped after %s: nothing more is started on the device" % name)
            f.write(json.dumps(res) + "\n")
            f.flush()
            print("%s: error budget rejects %d of %d cases; sweep rejects %d of %d cases in %d rows, worst %.3g = %.1f x its record (%s)%s"
                  % (name, res["budget_rejects"], res["budget_cases"], res["sweep_rejects"], res["sweep_cases"],
                     len(res["sweep_rejected_rows"]), res["sweep_worst_there"], res["sweep_worst_over_record"],
                     res["sweep_worst_over_record_case"],
                     (": " + ", ".join(res["sweep_rejected_rows"][:10]) + (" ..." if len(res["sweep_rejected_rows"]) > 10 else ""))
                     if res["sweep_rejected_rows"] else ""), flush=True)


if __name__ == "__main__":
    main()
