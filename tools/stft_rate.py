#!/usr/bin/env python3
"""Rate of the framed real-input plans against the in-place streaming ceiling and against the recipe a user had before them,
on one GPU.

Per case (fft_len, hop, output, windowed or rectangular): stft.Spectrum / stft.Power over 16 signals of 2^24 f32 (1 GiB of
signal, four times the Infinity Cache) timed by HIP events, one event pair per exec, the median and the minimum of 200 execs
after 20 warm-up execs; in the same run, alternating with it in blocks of 50, (a) the in-place fwa_calib_copy over the recipe's
frame buffer (every line read, then written back: the ceiling of one pass over memory) and (b) the recipe: real.Forward over
the same number of frames ALREADY materialised and windowed (4 n bytes per frame; the materialise pass itself -- the signal
read, the window product and 4 n bytes written per frame -- is NOT counted, and the recipe stores spectra even where the plan
stores power).  A framed plan must read 4 min(hop, n) fresh bytes per frame and write 8 (n / 2 + 1) (spectrum) or
4 (n / 2 + 1) (power); the recipe reads 4 n and writes 8 (n / 2 + 1).  The spread is max - min of the recipe's four block
medians: a difference between plan and recipe below it is not a difference.  One JSON line per case.

    python tools/stft_rate.py --out profiles/round11/stft_rate.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = [64, 1024, 4096]
SIGNALS, SIGNAL_LEN = 16, 1 << 24
EXECS, WARMUP, BLOCK = 200, 20, 50


def cases():
    """(n, hop, output, windowed): every n at hop = n, n / 2, n / 4, windowed spectra; power at hop = n / 4; the rectangular
    plan at hop = n, the shape of real.Forward itself; one odd hop"""
    out = []
    for n in LENGTHS:
        out += [(n, hop, "Spectrum", True) for hop in (n, n // 2, n // 4)]
        out += [(n, n // 4, "Power", True), (n, n, "Spectrum", False)]
    out.append((1024, 255, "Spectrum", True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round11/stft_rate.jsonl")
    args = ap.parse_args()
    import numpy as np
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import real, stft
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("stft_rate.py: no gfx950 device visible; there is nothing to measure without one")
    dev, queue = got
    enc = dev.create_command_encoder()
    signal_bytes = SIGNALS * SIGNAL_LEN * 4
    x = dev.create_buffer(signal_bytes)
    dev.fill_synthetic(x, 4096, encoder=enc)
    out_rows = []
    for n, hop, output, windowed in cases():
        per = stft.describe(n, hop, SIGNAL_LEN, SIGNALS)["frames_per_signal"]
        frames = SIGNALS * per
        frame_bytes, spec_bytes = frames * n * 4, frames * (n // 2 + 1) * 8
        dst_bytes = spec_bytes if output == "Spectrum" else spec_bytes // 2
        fbuf, spec = dev.create_buffer(frame_bytes), dev.create_buffer(spec_bytes)
        dst = spec if output == "Spectrum" else dev.wrap_buffer(spec.device_ptr, dst_bytes)
        dev.fill_synthetic(fbuf, n, encoder=enc)
        win = None
        if windowed:
            win = dev.create_buffer(4 * n)
            queue.write_buffer(win, 0, (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32))
        plan = getattr(stft, output)(dev, queue, x, dst, n, hop, SIGNAL_LEN, window=win)
        recipe = real.Forward(dev, queue, fbuf, spec, n)
        assert recipe.get("batch") == frames == plan.get("frames")
        ev = [(fw.Event(dev), fw.Event(dev)) for _ in range(BLOCK)]

        def timed(call):
            for a, b in ev:
                a.record(enc)
                call()
                b.record(enc)
            enc.synchronize()
            return [a.elapsed_ms(b) for a, b in ev]

        calls = {"plan": lambda: plan.proc(enc), "copy": lambda: dev.calib_copy(fbuf, fbuf, frame_bytes, encoder=enc),
                 "recipe": lambda: recipe.proc(enc)}
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
        moved = frames * 4 * min(hop, n) + dst_bytes
        row = {"n": n, "hop": hop, "output": output, "windowed": windowed, "signals": SIGNALS, "signal_len": SIGNAL_LEN, "frames": frames,
               "signal_bytes": signal_bytes, "dst_bytes": dst_bytes, "bytes_moved": moved, "recipe_bytes_moved": frame_bytes + spec_bytes,
               "recipe": "real.Forward over the frames already materialised and windowed; the materialise pass is not counted",
               "execs": EXECS, "threads": plan.get("threads"), "lds_bytes": plan.get("lds_bytes"),
               "frames_per_block": plan.get("frames_per_block"), "blocks": plan.get("blocks"),
               "calib_copy_in_place_ms_median": round(med["copy"], 5), "calib_copy_TBps": round(2 * frame_bytes / med["copy"] / 1e9, 3),
               "plan_ms_median": round(med["plan"], 5), "plan_ms_min": round(low["plan"], 5), "plan_TBps": round(moved / med["plan"] / 1e9, 3),
               "recipe_ms_median": round(med["recipe"], 5), "recipe_ms_min": round(low["recipe"], 5),
               "recipe_block_medians_ms": [round(m, 5) for m in blocks], "recipe_spread_ms": round(spread, 5),
               "plan_over_recipe": round(med["recipe"] / med["plan"], 3),
               "plan_slower_than_recipe_by_more_than_spread": bool(med["plan"] - med["recipe"] > spread),
               "device": dev.info()["name"]}
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        for h in [recipe, plan] + ([win] if win is not None else []) + ([dst] if dst is not spec else []) + [spec, fbuf]:
            h.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
