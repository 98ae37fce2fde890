#!/usr/bin/env python3
"""tools/record_error_budget.py [--out FILE] [--classes-out FILE] [--lab] [--only SUBSTR] -- run the error-budget matrix
(oracle/error_budget.py) on device 0 and write one entry per case: rel_l2, max_rel against the fp64 DFT, and the path /
factors / launches per exec the plan actually took.  Default FILE: tests/golden/error_budget.json, the record
tests/test_gpu_error_budget.py pins to.  From the same execs it writes the per-class record (oracle/output_classes.py): per
case and per class map the best and the worst class as fractions of cap(n), to tests/golden/error_budget_classes.json (with
--out: to FILE's name with _classes before the extension), under the stamp of the first file.

A run whose cases come out exactly as FILE already holds them, on the kernel sources FILE is stamped with, leaves FILE as
it is -- results are bit-deterministic, so `git diff --stat` after a re-record shows whether anything moved -- and the
class record takes FILE's stamp.

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
from oracle import output_classes as oc  # noqa: E402


def commit():
    c = os.environ.get("FWA_COMMIT", "")
    if c:
        return c
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else "unknown (no .git on this box and no FWA_COMMIT given)"


def dump(rec, path):
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=eb.RECORD_PATH)
    ap.add_argument("--classes-out", default="")
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
    top = max(((float(e.max()) / eb.cap(c["n"]), c["id"], name, int(e.argmax())) for c in cases
               for name, e in res[c["id"]]["classes"].items()), key=lambda v: (v[0] != v[0], v[0]))
    classes = {c["id"]: oc.spread_record(oc.spread(res[c["id"]].pop("classes"), eb.cap(c["n"]))) for c in cases}
    rec = {
        "_comment": "Measured fp32 error of every kernel family against the fp64 DFT (oracle/error_budget.py: matrix, metric, "
                    "rule); written by tools/record_error_budget.py, pinned by tests/test_gpu_error_budget.py.",
        "stamp": {"commit": commit(), "kernel_sources": eb.KERNEL_SOURCE_DIR + "/*",
                  "kernel_source_sha256": eb.kernel_source_sha256(), "device": dev.info()["name"],
                  "library": "laboratory" if args.lab else "product", "seconds": round(time.time() - t0, 1)},
        "cases": res,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    old = None
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    same = old is not None and json.dumps(old.get("cases"), sort_keys=True) == json.dumps(res, sort_keys=True) and all(
        old["stamp"].get(k) == rec["stamp"][k] for k in ("kernel_source_sha256", "device", "library"))
    if same:
        rec = old
        print("%s: every case as recorded, on the same kernel sources: left as it is" % args.out)
    else:
        dump(rec, args.out)
    classes_out = args.classes_out or (eb.CLASSES_RECORD_PATH if os.path.abspath(args.out) == os.path.abspath(eb.RECORD_PATH)
                                       else "%s_classes%s" % os.path.splitext(args.out))
    dump({
        "_comment": "rel_l2 of the best and the worst output class of every class map of every case, as fractions of cap(n) "
                    "(oracle/output_classes.py: maps, metric, CLASS_FACTOR; oracle/error_budget.py check_classes: the rule); "
                    "written by tools/record_error_budget.py from the execs of %s, pinned by tests/test_gpu_error_budget.py."
                    % os.path.basename(args.out),
        "stamp": {k: rec["stamp"][k] for k in ("commit", "kernel_sources", "kernel_source_sha256", "device", "library")},
        "cases": classes,
    }, classes_out)
    print("wrote %s: worst class %.3f of cap (%s, class %d of '%s'); CLASS_FACTOR %.2f" % (
        classes_out, top[0], top[1], top[3], top[2], oc.CLASS_FACTOR))
    worst = max(cases, key=lambda c: res[c["id"]]["rel_l2"] / eb.cap(c["n"]))
    print("%s: %d cases in %.0f s; worst rel_l2 / cap %.3f (%s)" % (
        args.out, len(res), time.time() - t0, res[worst["id"]]["rel_l2"] / eb.cap(worst["n"]), worst["id"]))
    if drift:
        print("plan drift (path / factors / launches differ from the matrix):", ", ".join(drift))
        sys.exit(1)


if __name__ == "__main__":
    main()
