#!/usr/bin/env python3
"""Rate of the fused FFT-convolution plans against the in-place streaming ceiling and against the recipe a user had before
them, on one GPU.

Per length: conv.Convolve over a 1-GiB `src` (four times the Infinity Cache) with F = 1 and F = 64 filter rows, in place
and out of place, timed by HIP events, one event pair per exec, the median and the minimum of 200 execs after 20 warm-up
execs; in the same run, alternating with them in blocks of 50, (a) the in-place fwa_calib_copy over the same buffer (every
line read, then written back: the ceiling of one pass over memory) and (b) the recipe: the product's Forward plan and then
its Inverse plan of length n over the same rows, two launches between one event pair, 32 bytes per sample -- the pointwise
multiply the recipe would also need (a third pass, 16 bytes per sample more, and a kernel this project does not have) is
NOT counted, so the comparison favours the recipe.  A fused plan moves 16 bytes per sample plus the F filter rows.  The
spread is max - min of the recipe's four block medians: a difference between plan and recipe below it is not a difference.
One JSON line per length.

    python tools/conv_rate.py --out profiles/round10/conv_rate.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = [8, 32, 64, 1024, 4096]
FILTERS = [1, 64]
EXECS, WARMUP, BLOCK = 200, 20, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round10/conv_rate.jsonl")
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import conv
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("conv_rate.py: no gfx950 device visible; there is nothing to measure without one")
    dev, queue = got
    enc = dev.create_command_encoder()
    out_rows = []
    for n in LENGTHS:
        batch = (1 << 30) // (8 * n)
        nbytes = batch * n * 8
        moved = 2 * nbytes
        x, y = dev.create_buffer(nbytes), dev.create_buffer(nbytes)
        dev.fill_synthetic(x, n, encoder=enc)
        # all-pass filters (|H| = 1, seeded random phases): the in-place execs then keep the data at its magnitude however
        # often they run, as the copy and the recipe (Forward, then the scaled Inverse) do
        banks = {F: dev.create_buffer(F * n * 8) for F in FILTERS}
        for F, b in banks.items():
            phase = np.random.default_rng(0xF117E5 + F).uniform(0, 2 * np.pi, F * n)
            queue.write_buffer(b, 0, np.exp(1j * phase).astype(np.complex64))
        plans = {}
        for F in FILTERS:
            plans["F%d_in_place" % F] = conv.Convolve(dev, queue, x, banks[F], x, n)
            plans["F%d_out_of_place" % F] = conv.Convolve(dev, queue, x, banks[F], y, n)
        # the recipe: Forward, then Inverse on the buffer Forward left its result in (its own second buffer when log2 n is odd)
        r_fwd = fw.Forward(dev, queue, x, n)
        r_inv = fw.Inverse(dev, queue, r_fwd.proc(enc), n)
        enc.synchronize()
        ev = [(fw.Event(dev), fw.Event(dev)) for _ in range(BLOCK)]

        def timed(call):
            for a, b in ev:
                a.record(enc)
                call()
                b.record(enc)
            enc.synchronize()
            return [a.elapsed_ms(b) for a, b in ev]

        def recipe():
            r_fwd.proc(enc)
            r_inv.proc(enc)

        calls = {k: (lambda p=p: p.proc(enc)) for k, p in plans.items()}
        calls["copy"] = lambda: dev.calib_copy(x, x, nbytes, encoder=enc)
        calls["recipe"] = recipe
        for _ in range(WARMUP):
            for call in calls.values():
                call()
        enc.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(EXECS // BLOCK):
            for k, call in calls.items():
                ms[k].append(timed(call))
        med = {k: statistics.median(t for block in v for t in block) for k, v in ms.items()}
        low = {k: min(min(block) for block in v) for k, v in ms.items()}
        blocks = [statistics.median(b) for b in ms["recipe"]]
        spread = max(blocks) - min(blocks)
        any_plan = next(iter(plans.values()))
        row = {"n": n, "batch": batch, "src_bytes": nbytes, "bytes_moved": moved, "recipe_bytes_moved": 2 * moved, "execs": EXECS,
               "threads": any_plan.get("threads"), "lds_bytes": any_plan.get("lds_bytes"), "rows_per_block": any_plan.get("rows_per_block"),
               "blocks": any_plan.get("blocks"),
               "calib_copy_in_place_ms_median": round(med["copy"], 5), "calib_copy_TBps": round(moved / med["copy"] / 1e9, 3),
               "recipe_ms_median": round(med["recipe"], 5), "recipe_ms_min": round(low["recipe"], 5),
               "recipe_block_medians_ms": [round(m, 5) for m in blocks], "recipe_spread_ms": round(spread, 5),
               "recipe_launches": r_fwd.get("launches_per_exec") + r_inv.get("launches_per_exec"),
               "device": dev.info()["name"]}
        for k in plans:
            own = [statistics.median(b) for b in ms[k]]
            row.update({k + "_ms_median": round(med[k], 5), k + "_ms_min": round(low[k], 5),
                        k + "_block_medians_ms": [round(m, 5) for m in own],
                        k + "_TBps": round(moved / med[k] / 1e9, 3),
                        k + "_rate_over_copy_rate": round(med["copy"] / med[k], 3),
                        k + "_over_recipe": round(med["recipe"] / med[k], 3),
                        k + "_slower_than_recipe_by_more_than_spread": bool(med[k] - med["recipe"] > spread)})
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        for h in list(plans.values()) + [r_inv, r_fwd] + list(banks.values()) + [y, x]:
            h.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
