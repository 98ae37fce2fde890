#!/usr/bin/env python3
"""tools/record_large_plans.py [--out FILE] [--lab] [--only SUBSTR] [--merge] -- run the sparse-input checks of the 2^28 .. 2^30 plans
(oracle/large_plans.py) on device 0 and write one entry per case: worst |y - W^(pk)| over the compared outputs of the swept
impulses with the (exec, impulse position, output) it was found at, each comb's max_rel and rel_l2, the path / factors /
tunables the plan held, the number of impulse execs T and the wall seconds of the case.  Default FILE:
tests/golden/large_plans.json, the record tests/test_gpu_large_plans.py pins to.

The file is stamped as tools/record_error_budget.py stamps its record: the commit it ran on (git, or $FWA_COMMIT) and the
sha256 of the kernel sources.  --lab loads the laboratory build ($FWA_LAB_LIBRARY when set: a mutant built with
tools/mutant_build.py).  --merge keeps the entries of FILE that this run does not repeat (a run of part of the cases with
--only), provided its kernel-source hash is the current one.  "notes" is for the (p, k) of a failure that led to a fix; it
is carried over from FILE.  Exit status 1 when a case took another path / factorisation than its row names, left a transform
without input non-zero, or missed the cap or REL_TOL.
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
from oracle import large_plans as lp  # noqa: E402
from tools.record_error_budget import commit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=lp.RECORD_PATH)
    ap.add_argument("--lab", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose id contains one of these comma-separated strings")
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    got = fw.prepare_gpu(0, lab=args.lab)
    if got is None:
        raise SystemExit("no gfx950 device visible")
    dev, queue = got
    only = [s for s in args.only.split(",") if s] or [""]
    cases = [c for c in lp.MATRIX if any(s in c["id"] for s in only)]
    sha = eb.kernel_source_sha256()
    old = lp.load_record(args.out) if os.path.exists(args.out) else {}
    res = {}
    if args.merge:
        if old.get("stamp", {}).get("kernel_source_sha256") != sha:
            raise SystemExit("--merge: %s was recorded on other kernel sources" % args.out)
        res = dict(old["cases"])
    t0 = time.time()
    bad = []
    for c in cases:
        if dev.info()["hbm_bytes"] < lp.device_bytes_needed(c):
            raise SystemExit("%s needs %d bytes of device memory" % (c["id"], lp.device_bytes_needed(c)))
        res[c["id"]] = r = lp.run_case(fw, dev, queue, c)
        print("%-28s worst %.3e (%.2f of cap) at exec %d (impulse at %d), output %d; combs max_rel %s; path %d factors %#x, T %d, %.1f s"
              % (c["id"], r["worst"], r["worst"] / lp.CAP, r["t"], r["p"], r["k"],
                 " ".join("%.2e" % g["max_rel"] for g in r["combs"]) or "-", r["path"], r["factors"], r["T"], r["seconds"]), flush=True)
        if (r["path"], r["factors"]) != (c["path"], c["factors"]):
            bad.append("%s: plan drift (path / factors differ from the row)" % c["id"])
        bad += lp.check(c, r, r)
    rec = {
        "_comment": "Worst |y - W^(pk)| of swept impulses and the parity figures of four combs through every plan of 2^28 .. 2^30 "
                    "(oracle/large_plans.py: rows, positions, windows, rules); written by tools/record_large_plans.py, pinned by "
                    "tests/test_gpu_large_plans.py.  T: impulse execs of the case; seconds: its wall time when recorded.",
        "stamp": {"commit": commit(), "kernel_sources": eb.KERNEL_SOURCE_DIR + "/*", "kernel_source_sha256": sha,
                  "device": dev.info()["name"], "library": "laboratory" if args.lab else "product", "seconds": round(time.time() - t0, 1)},
        "cap": lp.CAP, "pin": lp.PIN, "rel_tol": lp.REL_TOL,
        "cases": res,
        "notes": old.get("notes", []),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    near = sorted(cases, key=lambda c: -res[c["id"]]["worst"])[:3]
    print("wrote %s: %d cases in %.0f s; closest to the cap: %s" % (
        args.out, len(cases), time.time() - t0, ", ".join("%s %.2f" % (c["id"], res[c["id"]]["worst"] / lp.CAP) for c in near)))
    if bad:
        print("\n".join(bad))
        sys.exit(1)


if __name__ == "__main__":
    main()
