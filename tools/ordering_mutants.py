#!/usr/bin/env python3
"""tools/ordering_mutants.py [build|run|all] [--only O1,O3] [--control] [--out FILE] -- evidence that the ordering scenarios
(oracle/ordering.py, tests/test_gpu_ordering.py) reject a build that lacks one host-side ordering edge.

build: the copy-and-substitute build of tools/mutant_build.py, one laboratory library per mutant under build/variants/.
run:   for each mutant, this file again as a fresh child process (`--child`) with FWA_LAB_LIBRARY pointing at the mutant's
       laboratory library and Device(lab=True), under a time limit: every scenario except the graph captures (a capture with
       an unjoined stream is an error return of the runtime, not an ordering result), once each, no retries.  One JSON line per
       mutant: the scenarios that rejected it, the scenarios its row names (NAMED below) and which of those let it through.
       --control first runs the tree's own laboratory library the same way (it must be rejected nowhere).  A child that
       fails (fault, abort, time limit, or an exception inside a scenario) ends the run: nothing more is started on the device.

Every mutant is host-side only, in plan.cpp, and removes one wait: no index changes, so the only effect is a data race
inside memory the plans own.  A race can lose by luck: a named scenario that lets a mutant through is a finding about the
scenario (too little overlap), reported in the line's "missed" and not hidden by running again.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.mutant_build import TREE_LAB_LIBRARY, VARIANTS, build, lib_path  # noqa: E402

_DESTROY_WAIT = (
    "        if (plan->ran_on_stream && alive && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {\n"
    "            // everything this plan enqueued on its last caller stream precedes this marker\n"
    "            if (hipEventRecord(ev, plan->last_stream) == hipSuccess) waited = hipEventSynchronize(ev) == hipSuccess;\n"
    "            (void)hipEventDestroy(ev);\n"
    "        }\n")
_DESTROY_FALLBACK = "            (void)hipDeviceSynchronize();\n        }\n    }\n    release_pipeline(plan->ctx, plan->pipe, true);"
_NO_FALLBACK = "        }\n    }\n    release_pipeline(plan->ctx, plan->pipe, true);"

# name: (the edge removed, [(file, old, new), ...], prefixes / suffixes of the scenario ids that must reject it)
MUTANTS = {
    "O1": ("fwa_plan_destroy waits for nothing: neither the marker on the plan's last stream nor the device-wide fallback", [
        ("plan.cpp", _DESTROY_WAIT, "        (void)alive; (void)ev;\n"),
        ("plan.cpp", _DESTROY_FALLBACK, "            (void)0;\n" + _NO_FALLBACK)],
        lambda i: i.startswith("destroy_in_flight/")),
    "O2": ("fwa_plan_destroy: no hipDeviceSynchronize fallback for a wrapped or already destroyed stream", [
        ("plan.cpp", _DESTROY_FALLBACK, "            (void)0;\n" + _NO_FALLBACK)],
        lambda i: i.startswith("destroy_in_flight/") and i.endswith(("/wrapped", "/destroyed"))),
    "O3": ("run_groups: the caller's stream does not wait for the chains (no join)", [
        ("plan.cpp", "        if (r == hipSuccess) r = hipStreamWaitEvent(st, pl.done[i], 0);\n", "")],
        lambda i: i.startswith(("two_plans_two_streams/P1+T2", "alternating_streams/", "host_pipeline/", "default_two_chains/"))),
    "O4": ("run_groups: the chains do not wait for the caller's stream (no fork)", [
        ("plan.cpp", "        for (size_t i = 0; i < ns; ++i) HIP_TRY(ctx, hipStreamWaitEvent(pl.streams[i], pl.fork, 0));\n", "")],
        lambda i: i.startswith(("alternating_streams/", "host_pipeline/"))),
}


def scenario_ids():
    from oracle import ordering
    return [i for i, _ in ordering.SCENARIOS if not i.startswith("graph_forked/")]


def child(out):
    """Run the non-graph scenarios on the laboratory library $FWA_LAB_LIBRARY names -> {id: [failure messages]} in `out`."""
    import fft_wgpu_amd as fw
    import oracle
    from oracle import ordering
    oracle.build()
    got = fw.prepare_gpu(0, lab=True)
    if got is None:
        raise SystemExit("no gfx950 device visible")
    dev, queue = got
    res = {}
    for sid, scenario in ordering.SCENARIOS:
        if sid.startswith("graph_forked/"):
            continue
        res[sid] = scenario(fw, dev, queue, oracle)     # an exception ends the child: the parent stops the run
        print("%-44s %s" % (sid, "REJECTS: " + res[sid][0] if res[sid] else "passes"), flush=True)
        with open(out, "w") as f:
            json.dump(res, f)


def run(name, lib, timeout):
    """one child process: every non-graph scenario on `lib` -> a JSON-able summary, or None when the child failed."""
    out = os.path.join(VARIANTS, name, "ordering.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if os.path.exists(out):
        os.remove(out)
    env = dict(os.environ, FWA_LAB_LIBRARY=lib)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, timeout=timeout,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        print("%s: time limit of %d s reached" % (name, timeout), flush=True)
        return None
    if p.returncode != 0:
        print("%s: child exited with %d\n%s\n%s" % (name, p.returncode, p.stdout[-3000:], p.stderr[-3000:]), flush=True)
        return None
    with open(out) as f:
        got = json.load(f)
    ids = scenario_ids()
    assert list(got) == ids, "the child ran other scenarios than the list"
    what, subs, named = MUTANTS[name] if name in MUTANTS else ("unmutated laboratory build (control)", [], lambda i: False)
    rejected = [i for i in ids if got[i]]
    named_ids = [i for i in ids if named(i)]
    return {
        "mutant": name, "what": what, "substitutions": [{"file": f, "old": o, "new": n} for f, o, n in subs],
        "scenarios": len(ids), "rejected_by": rejected, "named": named_ids,
        "missed": [i for i in named_ids if i not in rejected],
        "caught": bool(rejected), "first_messages": {i: got[i][0] for i in rejected},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("build", "run", "all"))
    ap.add_argument("--only", default="", help="comma-separated mutant names (default: all)")
    ap.add_argument("--control", action="store_true", help="run the unmutated laboratory build first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round7", "ordering_mutants.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", metavar="FILE", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    names = [m for m in args.only.split(",") if m] or list(MUTANTS)
    if args.what in ("build", "all"):
        for name in names:
            build(name, MUTANTS[name][1])
    if args.what == "build":
        return
    todo = ([("control", TREE_LAB_LIBRARY)] if args.control else []) + [(m, lib_path(m)) for m in names]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, lib in todo:
            res = run(name, lib, args.timeout)
            if res is None:
                raise SystemExit("stopped after %s: nothing more is started on the device" % name)
            f.write(json.dumps(res) + "\n")
            f.flush()
            print("%s: rejected by %d of %d scenarios; named %d, missed %d%s" % (
                name, len(res["rejected_by"]), res["scenarios"], len(res["named"]), len(res["missed"]),
                (": " + ", ".join(res["missed"])) if res["missed"] else ""), flush=True)


if __name__ == "__main__":
    main()
