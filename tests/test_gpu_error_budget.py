"""GPU: every kernel family held to its own measured fp32 error (oracle/error_budget.py), not only to the flat 1e-5.

The matrix runs once per module (the fp64 DFT of an input is shared by Inverse and Onlyinverse); each case row is then
one test over its three plan kinds: the plan must take the path / factorisation / launch count the matrix names, and
its rel_l2 and max_rel must pass the rule against tests/golden/error_budget.json -- within the pin of the recorded value
and under the cap.  A case without a record fails.  Re-record with tools/record_error_budget.py on purpose only.

The same results, reduced per output class on the host (oracle/output_classes.py: the digits of the output index in
windows of 8 bits, the arithmetic thread and the half of k_chunk, the workgroup slot of k_small32), must pass the rule per
class against tests/golden/error_budget_classes.json: every class within the pin of the recorded worst class of its map and
under CLASS_FACTOR x cap(n).  A loss confined to one thread, register or tile line moves the whole-buffer figure by a few
per cent; it doubles its class.

The 2^27..2^30 impulse test of test_gpu_parity.py stays outside the matrix: a one-index twiddle error there (2 pi / N
<= 5e-8) sits below fp32 resolution.
"""
import os

import pytest

from oracle import error_budget as eb
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu

ROWS = sorted({c["case"] for c in eb.MATRIX}, key=[c["case"] for c in eb.MATRIX].index)


@pytest.fixture(scope="module")
def measured():
    return eb.measure(*open_gpu())


@pytest.fixture(scope="module")
def record():
    assert os.path.exists(eb.RECORD_PATH), "no error-budget record: run tools/record_error_budget.py"
    return eb.load_record()


@pytest.fixture(scope="module")
def class_record():
    assert os.path.exists(eb.CLASSES_RECORD_PATH), "no per-class record: run tools/record_error_budget.py"
    return eb.load_record(eb.CLASSES_RECORD_PATH)


@pytest.mark.parametrize("row", ROWS)
def test_kernel_family_within_its_error_budget(measured, record, row):
    bad = []
    for case in (c for c in eb.MATRIX if c["case"] == row):
        got = measured[case["id"]]
        took = tuple(got[k] for k in ("path", "factors", "launches_per_exec"))
        want = (case["path"], case["factors"], case["launches_per_exec"])
        if took != want:
            bad.append("%s [%s]: plan took path/factors/launches %s, the matrix names %s" % (case["id"], case["kernels"], took, want))
        bad += eb.check(case, got, record["cases"].get(case["id"]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("row", ROWS)
def test_kernel_family_classes_within_budget(measured, class_record, row):
    bad = []
    for case in (c for c in eb.MATRIX if c["case"] == row):
        bad += eb.check_classes(case, measured[case["id"]]["classes"], class_record["cases"].get(case["id"]))
    assert not bad, "\n".join(bad[:8])
