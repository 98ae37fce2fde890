#!/usr/bin/env python3
"""tools/record_error_budget.py [--out FILE] [--lab] [--only SUBSTR] -- run the error-budget matrix (oracle/error_budget.py)
on device 0 and write one entry per case: rel_l2, max_rel against the fp64 DFT, and the path / factors / launches per exec
the plan actually took.  Default FILE: tests/golden/error_budget.json, the record tests/test_gpu_error_budget.py pins to.

The file is stamped with the commit it ran on (git, or $FWA_COMMIT: the GPU box has no .git) and with the sha256 of the
kernel sources (fft_wgpu_amd/csrc/*, build products excluded), as tools/make_bench_reference.py stamps its figures.
--lab loads the laboratory build ($FWA_LAB_LIBRARY when set: tools/error_budget_mutants.py points it at a mutant).
Exit status 1 when a case took another path / factorisation / launch count than the matrix expects (the entry is written
with what it took).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fft_wgpu_amd as fw  # noqa: E402
from oracle import error_budget as eb  # noqa: E402


def commit():
    c = os.environ.get("FWA_COMMIT", "")
    if c:
        return c
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else "unknown (no .git on this box and no FWA_COMMIT given)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=eb.RECORD_PATH)
    ap.add_argument("--lab", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose id contains this string")
    args = ap.parse_args()
    got = fw.prepare_gpu(0, lab=args.lab)
    if got is None:
        raise SystemExit("no gfx950 device visible")
    dev, queue = got
    cases = [c for c in eb.MATRIX if args.only in c["id"]]
    t0 = time.time()
    res = eb.measure(fw, dev, queue, cases, log=lambda s: print(s, flush=True))
    drift = [c["id"] for c in cases if any(res[c["id"]][k] != c[k] for k in ("path", "factors", "launches_per_exec"))]
    rec = {
        "_comment": "Measured fp32 error of every kernel family against the fp64 DFT (oracle/error_budget.py: matrix, metric, "
                    "rule); written by tools/record_error_budget.py, pinned by tests/test_gpu_error_budget.py.",
        "stamp": {"commit": commit(), "kernel_sources": eb.KERNEL_SOURCE_DIR + "/*",
                  "kernel_source_sha256": eb.kernel_source_sha256(), "device": dev.info()["name"],
                  "library": "laboratory" if args.lab else "product", "seconds": round(time.time() - t0, 1)},
        "cases": res,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    worst = max(cases, key=lambda c: res[c["id"]]["rel_l2"] / eb.cap(c["n"]))
    print("wrote %s: %d cases in %.0f s; worst rel_l2 / cap %.3f (%s)" % (
        args.out, len(res), time.time() - t0, res[worst["id"]]["rel_l2"] / eb.cap(worst["n"]), worst["id"]))
    if drift:
        print("plan drift (path / factors / launches differ from the matrix):", ", ".join(drift))
        sys.exit(1)


if __name__ == "__main__":
    main()
