#!/usr/bin/env python3
"""Rate of the real-input plans against the in-place streaming ceiling and against the recipe a user had before them,
on one GPU.

Per length: real.Forward (n f32 -> n / 2 + 1 samples per row) and real.Inverse (back) timed by HIP events, one event pair
per exec, the median and the minimum of 200 execs after 20 warm-up execs; in the same run, alternating with them in blocks
of 50, (a) the in-place fwa_calib_copy over the recipe's buffer (every line read, then written back: the ceiling of one
pass over memory) and (b) the recipe: the product's length-n complex Forward / Inverse over the same rows already promoted
to complex (16 n bytes per row; the promote pass itself, another 12 n bytes per row, is NOT counted).  A real plan moves
4 n + 8 (n / 2 + 1) bytes per row.  The spread is max - min of the recipe's four block medians: a difference between plan
and recipe below it is not a difference.  The real buffer is at least 1 GiB, four times the Infinity Cache; the spectrum
buffer is a little larger, the recipe's twice that.  One JSON line per length.

    python tools/real_rate.py --out profiles/round9/real_rate.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = [64, 1024, 4096]
EXECS, WARMUP, BLOCK = 200, 20, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round9/real_rate.jsonl")
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import real
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("real_rate.py: no gfx950 device visible; there is nothing to measure without one")
    dev, queue = got
    enc = dev.create_command_encoder()
    out_rows = []
    for n in LENGTHS:
        batch = (1 << 30) // (4 * n)
        real_bytes, spec_bytes, cplx_bytes = batch * n * 4, batch * (n // 2 + 1) * 8, batch * n * 8
        moved = real_bytes + spec_bytes
        x, spec, back, cbuf = (dev.create_buffer(b) for b in (real_bytes, spec_bytes, real_bytes, cplx_bytes))
        dev.fill_synthetic(x, n, encoder=enc)
        dev.fill_synthetic(cbuf, n, encoder=enc)
        fwd, inv = real.Forward(dev, queue, x, spec, n), real.Inverse(dev, queue, spec, back, n)
        r_fwd = fw.Forward(dev, queue, cbuf, n)
        r_inv = fw.Inverse(dev, queue, cbuf, n)
        ev = [(fw.Event(dev), fw.Event(dev)) for _ in range(BLOCK)]

        def timed(call):
            for a, b in ev:
                a.record(enc)
                call()
                b.record(enc)
            enc.synchronize()
            return [a.elapsed_ms(b) for a, b in ev]

        calls = {"forward": lambda: fwd.proc(enc), "inverse": lambda: inv.proc(enc),
                 "copy": lambda: dev.calib_copy(cbuf, cbuf, cplx_bytes, encoder=enc),
                 "recipe_forward": lambda: r_fwd.proc(enc), "recipe_inverse": lambda: r_inv.proc(enc)}
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
        row = {"n": n, "batch": batch, "real_bytes": real_bytes, "spectrum_bytes": spec_bytes, "bytes_moved": moved,
               "recipe_bytes_moved": 2 * cplx_bytes, "execs": EXECS, "threads": fwd.get("threads"), "lds_bytes": fwd.get("lds_bytes"),
               "rows_per_block": fwd.get("rows_per_block"), "blocks": fwd.get("blocks"),
               "calib_copy_in_place_ms_median": round(med["copy"], 5), "calib_copy_TBps": round(2 * cplx_bytes / med["copy"] / 1e9, 3),
               "device": dev.info()["name"]}
        for kind in ("forward", "inverse"):
            blocks = [statistics.median(b) for b in ms["recipe_" + kind]]
            spread = max(blocks) - min(blocks)
            row.update({kind + "_ms_median": round(med[kind], 5), kind + "_ms_min": round(low[kind], 5),
                        kind + "_TBps": round(moved / med[kind] / 1e9, 3),
                        kind + "_rate_over_copy_rate": round((moved / med[kind]) / (2 * cplx_bytes / med["copy"]), 3),
                        "recipe_" + kind + "_ms_median": round(med["recipe_" + kind], 5),
                        "recipe_" + kind + "_ms_min": round(low["recipe_" + kind], 5),
                        "recipe_" + kind + "_block_medians_ms": [round(m, 5) for m in blocks],
                        "recipe_" + kind + "_spread_ms": round(spread, 5),
                        kind + "_over_recipe": round(med["recipe_" + kind] / med[kind], 3),
                        kind + "_slower_than_recipe_by_more_than_spread": bool(med[kind] - med["recipe_" + kind] > spread)})
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        for h in (r_inv, r_fwd, inv, fwd, cbuf, back, spec, x):
            h.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
