#!/usr/bin/env python3
"""Rate of the strided-batch (column) plans against the in-place streaming ceiling, on one GPU.

Per shape: strided.Forward timed by HIP events, one event pair per exec, the median of 200 execs after 20 warm-up execs;
in the same run, alternating with it in blocks of 50, the in-place fwa_calib_copy over the same bytes (every line read,
then written back: the ceiling a one-pass kernel is compared with).  Bytes = the algorithmic 16 B per sample.  Every
buffer is at least 1 GiB (several matrices where one is smaller), four times the Infinity Cache.  One JSON line per shape.

    python tools/strided_rate.py --out profiles/round7/strided_rate.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 1 << 15), (1024, 1 << 15), (1024, (1 << 15) + 5), (4096, 1 << 15)]
EXECS, WARMUP, BLOCK = 200, 20, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round7/strided_rate.jsonl")
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import strided
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("strided_rate.py: no gfx950 device visible; there is nothing to measure without one")
    dev, queue = got
    enc = dev.create_command_encoder()
    rows = []
    for n, howmany in SHAPES:
        mbytes = 8 * n * howmany
        batch = max(1, (1 << 30) // mbytes)
        nbytes = batch * mbytes
        buf = dev.create_buffer(nbytes)
        dev.fill_synthetic(buf, n, encoder=enc)
        plan = strided.Forward(dev, queue, buf, n, howmany)
        ev = [(fw.Event(dev), fw.Event(dev)) for _ in range(BLOCK)]

        def timed(call, count):
            ms = []
            for _ in range(count // BLOCK):
                for a, b in ev:
                    a.record(enc)
                    call()
                    b.record(enc)
                enc.synchronize()
                ms += [a.elapsed_ms(b) for a, b in ev]
            return ms
        fft = lambda: plan.proc(enc)
        copy = lambda: dev.calib_copy(buf, buf, nbytes, encoder=enc)
        for _ in range(WARMUP):
            fft()
            copy()
        enc.synchronize()
        t_fft, t_copy = [], []
        for _ in range(EXECS // BLOCK):
            t_fft += timed(fft, BLOCK)
            t_copy += timed(copy, BLOCK)
        m_fft, m_copy = statistics.median(t_fft), statistics.median(t_copy)
        row = {"fft_len": n, "howmany": howmany, "batch": batch, "bytes": nbytes, "execs": EXECS,
               "tile_cols": plan.get("tile_cols"), "threads": plan.get("threads"), "blocks": plan.get("blocks"),
               "forward_ms_median": round(m_fft, 5), "forward_ms_min": round(min(t_fft), 5),
               "forward_TBps": round(2 * nbytes / m_fft / 1e9, 3),
               "calib_copy_in_place_ms_median": round(m_copy, 5), "calib_copy_TBps": round(2 * nbytes / m_copy / 1e9, 3),
               "forward_over_copy": round(m_copy / m_fft, 3), "device": dev.info()["name"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        plan.destroy()
        buf.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
