#!/usr/bin/env python3
"""Rate of the in-place 2-D plans against the in-place streaming ceiling and against the two-plan recipe, on one GPU.

Per shape: fft2d.Forward timed by HIP events, one event pair per exec, the median of 200 execs after 20 warm-up execs; in
the same run, alternating with it in blocks of 50, (a) the in-place fwa_calib_copy over the same bytes (every line read,
then written back: the ceiling of ONE pass, so a two-launch plan can reach 0.5 of it and the one-launch plan 1.0) and (b)
the recipe the 2-D plans replace: fw.Forward over the rows, then strided.Forward over the columns of the buffer it returns
(in place only where log2 cols is even; otherwise the row spectra land in the row plan's second buffer -- "in_place"
says which).  The spread is max - min of the recipe's four block medians: a difference between plan and recipe below it
is not a difference.  Every buffer is at least 1 GiB, four times the Infinity Cache.  One JSON line per shape.

    python tools/fft2d_rate.py --out profiles/round8/fft2d_rate.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 32), (8, 8), (64, 64), (256, 256), (1024, 1024), (512, 512), (2048, 128), (4096, 4096)]   # rows, cols
EXECS, WARMUP, BLOCK = 200, 20, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round8/fft2d_rate.jsonl")
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import fft2d, strided
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("fft2d_rate.py: no gfx950 device visible; there is nothing to measure without one")
    dev, queue = got
    enc = dev.create_command_encoder()
    out_rows = []
    for rows, cols in SHAPES:
        ibytes = 8 * rows * cols
        batch = max(1, (1 << 30) // ibytes)
        nbytes = batch * ibytes
        buf = dev.create_buffer(nbytes)
        dev.fill_synthetic(buf, cols, encoder=enc)
        plan = fft2d.Forward(dev, queue, buf, rows, cols)
        row_plan = fw.Forward(dev, queue, buf, cols)
        mid = row_plan.proc(enc)                               # the buffer the row spectra land in
        col_plan = strided.Forward(dev, queue, mid, rows, cols)
        ev = [(fw.Event(dev), fw.Event(dev)) for _ in range(BLOCK)]

        def timed(call):
            for a, b in ev:
                a.record(enc)
                call()
                b.record(enc)
            enc.synchronize()
            return [a.elapsed_ms(b) for a, b in ev]

        def recipe():
            row_plan.proc(enc)
            col_plan.proc(enc)
        calls = {"plan": lambda: plan.proc(enc), "copy": lambda: dev.calib_copy(buf, buf, nbytes, encoder=enc), "recipe": recipe}
        for _ in range(WARMUP):
            for call in calls.values():
                call()
        enc.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(EXECS // BLOCK):
            for k, call in calls.items():
                ms[k].append(timed(call))
        med = {k: statistics.median(t for block in v for t in block) for k, v in ms.items()}
        recipe_blocks = [statistics.median(b) for b in ms["recipe"]]
        spread = max(recipe_blocks) - min(recipe_blocks)
        row = {"rows": rows, "cols": cols, "batch": batch, "bytes": nbytes, "execs": EXECS,
               "launches_per_exec": plan.get("launches_per_exec"), "row_threads": plan.get("row_threads"),
               "row_lds_bytes": plan.get("row_lds_bytes"), "row_blocks": plan.get("row_blocks"), "col_blocks": plan.get("col_blocks"),
               "forward_ms_median": round(med["plan"], 5), "forward_ms_min": round(min(min(b) for b in ms["plan"]), 5),
               "forward_TBps_at_16B_per_sample": round(2 * nbytes / med["plan"] / 1e9, 3),
               "calib_copy_in_place_ms_median": round(med["copy"], 5), "calib_copy_TBps": round(2 * nbytes / med["copy"] / 1e9, 3),
               "forward_over_copy": round(med["copy"] / med["plan"], 3),
               "recipe_in_place": mid is buf, "recipe_ms_median": round(med["recipe"], 5),
               "recipe_block_medians_ms": [round(m, 5) for m in recipe_blocks], "recipe_spread_ms": round(spread, 5),
               "forward_over_recipe": round(med["recipe"] / med["plan"], 3),
               "slower_than_recipe_by_more_than_spread": bool(med["plan"] - med["recipe"] > spread),
               "device": dev.info()["name"]}
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        for h in (col_plan, row_plan, plan, buf):
            h.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
