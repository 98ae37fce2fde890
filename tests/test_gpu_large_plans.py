"""GPU: the plans of 2^28 .. 2^30 against an fp64 DFT on sparse inputs (oracle/large_plans.py).

One test per case: the seven rows -- k_colsw<9,32> at its 2^31-byte limit, k_p1_gen over four live descriptors and at pitch
2^20, and every 64-bit-pointer instantiation of k_tile a plan can reach (columns and rows at 512 and 1024 points) -- in
Forward, Inverse and Onlyinverse, and p1gen_2^29 on a buffer of two transforms.  The plan must take the path and factorisation
its row names and hold every key the row set.  Then 128 execs of one transform each, all zero but for 1 + 0i at a position
swept over the residues, the columns and all four quarters of the buffer (p = n - 1 among them), with 34 windows of 2048
outputs spread over the whole result held to exp(-+2 pi i p k / n) in float64: the worst |y - r| must stay within the pin of
tests/golden/large_plans.json and under CAP = pi / 2^20, half the rotation of a hi[] index one off at 2^30.  Four combs of up
to 1024 non-zeros follow -- two dense columns, which every descriptor of pass A must read, one middle and one row comb -- held
to their O(M) float64 sums within REL_TOL and the pin.  In the batch-2 case the windows of the transform without input must
come back exactly zero.  tests/test_large_plans.py shows on the CPU that an fp32 model of the twiddle path passes and that a
hi index one off, a quarter read as zeros and a stray sample do not.  A case without a record fails.  Re-record with
tools/record_large_plans.py on purpose only.
"""
import os

import pytest

from oracle import large_plans as lp
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


@pytest.fixture(scope="module")
def record():
    assert os.path.exists(lp.RECORD_PATH), "no large-plan record: run tools/record_large_plans.py"
    return lp.load_record()


@pytest.mark.parametrize("case", lp.MATRIX, ids=[c["id"] for c in lp.MATRIX])
def test_sparse_inputs_through_the_large_plans(gpu, record, case):
    fw, dev, queue = gpu
    if dev.info()["hbm_bytes"] < lp.device_bytes_needed(case):
        pytest.skip("needs ~4 buffers of the transform size in device memory")
    got = lp.run_case(fw, dev, queue, case)
    print("%s [%s]: %d outputs compared in %.1f s: worst %.3e (%.2f of the cap) at exec %d (impulse at %d), output %d; combs %s"
          % (case["id"], case["kernels"], got["compared"], got["seconds"], got["worst"], got["worst"] / lp.CAP, got["t"], got["p"],
             got["k"], ", ".join("%s %.2e / %.2e" % (g["name"], g["max_rel"], g["rel_l2"]) for g in got["combs"]) or "-"))
    bad = []
    if (got["path"], got["factors"]) != (case["path"], case["factors"]):
        bad.append("%s [%s]: plan took path/factors %s, the row names %s"
                   % (case["id"], case["kernels"], (got["path"], got["factors"]), (case["path"], case["factors"])))
    assert got["tunables"] == case["tunables"] and got["compared"] == lp.compared_outputs(case) and got["T"] == case["T"]
    bad += lp.check(case, got, record["cases"].get(case["id"]))
    assert not bad, "\n".join(bad)
