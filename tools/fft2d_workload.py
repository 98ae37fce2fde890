#!/usr/bin/env python3
"""A few execs of one 2-D plan and nothing else: the workload of a counters-only profiler run.

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d OUT -- \\
        python tools/fft2d_workload.py --rows 32 --cols 32 --batch 65536

(no tracing combined with the counters).  profiles/round8/lds_bank_conflict_summary.json is the per-kernel sum of such runs.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, required=True)
    ap.add_argument("--cols", type=int, required=True)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--execs", type=int, default=4)
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import fft2d
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("fft2d_workload.py: no gfx950 device visible")
    dev, queue = got
    enc = dev.create_command_encoder()
    buf = dev.create_buffer(8 * args.rows * args.cols * args.batch)
    dev.fill_synthetic(buf, args.cols, encoder=enc)
    plan = fft2d.Forward(dev, queue, buf, args.rows, args.cols)
    for _ in range(args.execs):
        plan.proc(enc)
    enc.synchronize()
    print("%d execs of %d x %d x %d, %d launch(es) each" % (args.execs, args.batch, args.rows, args.cols, plan.get("launches_per_exec")))
    plan.destroy()
    buf.destroy()


if __name__ == "__main__":
    main()
