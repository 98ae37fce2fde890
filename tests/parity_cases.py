"""What the parity tests of the product library (test_gpu_parity.py), of the laboratory build (test_gpu_lab.py) and of
the sharded forms (test_gpu_sharding.py) share: the runner in their call shape, the parity assertion and the
fixture-size body.  A plain module, not a test file."""
import pytest

from conftest import REL_TOL
from oracle import device_run

# the keys the parity tests ask of a plan beside path, factors and launches_per_exec
FACTS = ("group", "xcd_swizzle", "p1_gen", "rows32", "colsw", "ring_rotate", "scratch_bytes", "device_error")


def run(fw, dev, queue, kind, x, n, **tunables):
    """device_run.run with the tunables as keywords (path, group, streams, tile_w, factors, small_reg, ...; None = not
    set) -> (result, 0 | 1: the buffer of processor.rs:153-157 it landed in, plan facts)."""
    y, where, facts = device_run.run(fw, dev, queue, kind, x, n, tunables, FACTS)
    return y, int(where != "src"), facts


def check(y, r, n, tol=REL_TOL):
    """every transform of `y` within `tol` of `r` in max_rel and rel-L2 -> the worst (max_rel, rel_l2)"""
    bad, worst = device_run.parity_failures(y, r, n, tol)
    assert not bad, (n,) + bad[0]
    return worst


def hip_runtime():
    hip = device_run.hip_runtime()
    if hip is None:
        pytest.skip("no libamdhip64 mapped in this process")
    return hip


# K4: numpy float64 fixtures, every power of two 2..1024: the shipped kernels (k_chunk up to 256, k_small32 from 512) and
# the literal one-launch-per-stage recurrence (path=2) in test_gpu_parity.py; the laboratory kernels (small_reg = 2, 3)
# run the same body in test_gpu_lab.py
def fixture_sizes_body(gpu, k4, path, small_reg):
    fw, dev, queue = gpu
    for lg in range(1, 11):
        n = 1 << lg
        x = k4[f"x_{n}"]
        y, which, _ = run(fw, dev, queue, "Forward", x, n, path=path, small_reg=small_reg)
        check(y, k4[f"fwd_{n}"], n)
        assert which == lg % 2
        y, _, _ = run(fw, dev, queue, "Onlyinverse", x, n, path=path, small_reg=small_reg)
        check(y, k4[f"inv_unscaled_{n}"], n)
        y, _, _ = run(fw, dev, queue, "Inverse", x, n, path=path, small_reg=small_reg)
        check(y, k4[f"inv_unscaled_{n}"] / n, n)
