#!/usr/bin/env python3
"""A few execs of one real-input plan pair (Forward, then Onlyinverse) and nothing else: the workload of a counters-only
profiler run.

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d OUT -- \\
        python tools/real_workload.py --n 1024 --batch 65536

(no tracing combined with the counters).  profiles/round9/real_lds_bank_conflict_summary.json is the per-kernel sum of
such runs (tools/pmc_summary.py).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--execs", type=int, default=4)
    args = ap.parse_args()
    import fft_wgpu_amd as fw
    from fft_wgpu_amd import real
    got = fw.prepare_gpu(0)
    if got is None:
        raise SystemExit("real_workload.py: no gfx950 device visible")
    dev, queue = got
    enc = dev.create_command_encoder()
    x = dev.create_buffer(4 * args.n * args.batch)
    spec = dev.create_buffer(8 * (args.n // 2 + 1) * args.batch)
    dev.fill_synthetic(x, args.n, encoder=enc)
    fwd, inv = real.Forward(dev, queue, x, spec, args.n), real.Onlyinverse(dev, queue, spec, x, args.n)
    for _ in range(args.execs):
        fwd.proc(enc)
    for _ in range(args.execs):
        inv.proc(enc)
    enc.synchronize()
    print("%d Forward and %d Onlyinverse execs of %d rows of n = %d" % (args.execs, args.execs, args.batch, args.n))
    for h in (fwd, inv, x, spec):
        h.destroy()


if __name__ == "__main__":
    main()
