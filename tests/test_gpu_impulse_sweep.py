"""GPU: the DFT matrix read out of every kernel by swept impulses, per output (oracle/impulse_sweep.py).

One test per (row, kind).  The plan must take the path and factorisation its row names and hold every key the row set;
then up to 4096 transforms, each all zero but for 1 + 0i at one position, go through it in execs of at most 2^30 samples,
and every compared output y[k] of the impulse at p is held to exp(-+2 pi i p k / n) from a float64 table: the worst
|y - r| must stay within the pin of tests/golden/impulse_response.json and under CAP = pi / 2^20, half of a one-index
rotation of a 2^20-domain twiddle.  The positions run over every residue that indexes the pass-A twiddle (every two-pass
row, the 2^20 pipeline, 64 x 64 x 64) or over 4096 of them with every digit present (the longer three-pass rows), so one
table entry one index off shows at the outputs it feeds -- the failure message names the transform, the impulse position
and the output -- where the norms of tests/test_gpu_error_budget.py move by nothing.  tests/test_impulse_sweep.py shows on
the CPU that the reference's own arithmetic passes and that the smallest such error does not.  A case without a record
fails.  Re-record with tools/record_impulse_response.py on purpose only.
"""
import os

import pytest

from oracle import impulse_sweep as im
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


@pytest.fixture(scope="module")
def record():
    assert os.path.exists(im.RECORD_PATH), "no impulse-response record: run tools/record_impulse_response.py"
    return im.load_record()


@pytest.mark.parametrize("case", im.MATRIX, ids=[c["id"] for c in im.MATRIX])
def test_swept_impulses_give_the_dft_matrix_per_output(gpu, oracle, record, case):
    fw, dev, queue = gpu
    if dev.info()["hbm_bytes"] < im.device_bytes_needed(case):
        pytest.skip("needs two buffers of %d transforms of 2^%d" % (im.buffer_transforms(case), case["n"].bit_length() - 1))
    got = im.run_case(fw, dev, queue, case)
    print("%s [%s]: %d impulses, %d outputs compared: worst %.3e (%.2f of the cap) at transform %d (impulse at %d), output %d"
          % (case["id"], case["kernels"], im.transforms(case), got["compared"], got["worst"], got["worst"] / im.CAP,
             got["t"], got["p"], got["k"]))
    bad = []
    if (got["path"], got["factors"]) != (case["path"], case["factors"]):
        bad.append("%s [%s]: plan took path/factors %s, the row names %s"
                   % (case["id"], case["kernels"], (got["path"], got["factors"]), (case["path"], case["factors"])))
    assert got["tunables"] == case["tunables"] and got["compared"] == im.compared_outputs(case)
    bad += im.check(case, got, record["cases"].get(case["id"]))
    assert not bad, "\n".join(bad)
