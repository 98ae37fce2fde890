#!/usr/bin/env python3
"""tools/record_impulse_response.py [--out FILE] [--lab] [--only SUBSTR] -- run the impulse sweeps (oracle/impulse_sweep.py) on
device 0 and write one entry per (row, kind): worst |y - W^(pk)| over the compared outputs, the (transform, impulse position,
output) it was found at, and the path / factors the plan actually took; per row the resolved index error
ceil(2 PIN worst / (2 pi / n)) of its worst kind.  Default FILE: tests/golden/impulse_response.json, the record
tests/test_gpu_impulse_sweep.py pins to.

The file is stamped as tools/record_error_budget.py stamps its record: the commit it ran on (git, or $FWA_COMMIT) and the
sha256 of the kernel sources.  --lab loads the laboratory build ($FWA_LAB_LIBRARY when set: tools/impulse_mutants.py points it
at a mutant).  Exit status 1 when a case took another path / factorisation than its row names.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fft_wgpu_amd as fw  # noqa: E402
from oracle import error_budget as eb  # noqa: E402
from oracle import impulse_sweep as im  # noqa: E402
from tools.record_error_budget import commit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=im.RECORD_PATH)
    ap.add_argument("--lab", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose id contains one of these comma-separated strings")
    args = ap.parse_args()
    got = fw.prepare_gpu(0, lab=args.lab)
    if got is None:
        raise SystemExit("no gfx950 device visible")
    dev, queue = got
    only = [s for s in args.only.split(",") if s] or [""]
    cases = [c for c in im.MATRIX if any(s in c["id"] for s in only)]
    t0 = time.time()
    res = {}
    for c in cases:
        t1 = time.time()
        res[c["id"]] = r = im.run_case(fw, dev, queue, c)
        print("%-36s worst %.3e (%.2f of cap) at transform %d (impulse at %d), output %d; %d outputs, path %d factors %#x, %.1f s"
              % (c["id"], r["worst"], r["worst"] / im.CAP, r["t"], r["p"], r["k"], r["compared"], r["path"], r["factors"],
                 time.time() - t1), flush=True)
    drift = [c["id"] for c in cases if (res[c["id"]]["path"], res[c["id"]]["factors"]) != (c["path"], c["factors"])]
    rows = {}
    for row in im.ROWS:
        kinds = [res[i] for i in ("%s/%s" % (row["case"], k) for k, _ in im.KINDS) if i in res]
        if kinds:
            worst = max(k["worst"] for k in kinds)
            rows[row["case"]] = {"n": row["n"], "worst": worst, "resolved_index_error": im.resolved_index_error(row["n"], worst)}
    rec = {
        "_comment": "Worst |y - W^(pk)| of every kernel on swept impulses (oracle/impulse_sweep.py: rows, positions, compared "
                    "outputs, rule); written by tools/record_impulse_response.py, pinned by tests/test_gpu_impulse_sweep.py.",
        "stamp": {"commit": commit(), "kernel_sources": eb.KERNEL_SOURCE_DIR + "/*",
                  "kernel_source_sha256": eb.kernel_source_sha256(), "device": dev.info()["name"],
                  "library": "laboratory" if args.lab else "product", "seconds": round(time.time() - t0, 1)},
        "cap": im.CAP, "pin": im.PIN,
        "cases": res,
        "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    worst = max(cases, key=lambda c: res[c["id"]]["worst"])
    print("wrote %s: %d cases in %.0f s; largest worst %.3e = %.2f of the cap (%s)" % (
        args.out, len(res), time.time() - t0, res[worst["id"]]["worst"], res[worst["id"]]["worst"] / im.CAP, worst["id"]))
    if drift:
        print("plan drift (path / factors differ from the row):", ", ".join(drift))
        sys.exit(1)


if __name__ == "__main__":
    main()
