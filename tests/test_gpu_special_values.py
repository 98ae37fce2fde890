"""GPU: NaN propagation, batch isolation and exact 2^s scaling of every kernel (oracle/special_values.py).

One test per row, over its three plan kinds, through the C ABI with the call sequence of device_run.run: the
plan must take the path / factorisation / launch count the row names; then
  * one input sample NaN + NaN i makes all 2n output floats of its transform NaN, +Inf - Inf i leaves no output finite in
    both parts, an all-zero transform gives zero;
  * every other transform of the batch keeps exactly the bits of the clean exec -- also on the row's ragged layout, where
    a special transform with a clean one on either side sits inside the partly valid last workgroup or group;
  * the input times 2^-40 (the benchmark's data), 2^40 and 2^90 gives the result times the same power, bit for bit and
    finite.
Every assertion is exact: bit-identity, isnan, isfinite or == 0.  Subnormals are not asserted.  tests/test_special_values.py
shows on the CPU that the reference's arithmetic meets every condition on these inputs, so a failure here is the kernel's:
a clean neighbour whose bits change names the transform that was read across; a finite output in a NaN transform names
the output index, which maps through the row's factorisation to the tile and stage that skipped the input.
"""
import numpy as np
import pytest

from oracle import special_values as sv
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


@pytest.mark.parametrize("row", [r["case"] for r in sv.ROWS])
def test_special_values_isolation_and_scaling(gpu, oracle, row):
    fw, dev, queue = gpu
    bad = []
    for case in (c for c in sv.MATRIX if c["case"] == row):
        msgs, facts, facts_ragged = sv.run_row_kind(fw, dev, queue, oracle, case)
        for c, got in ((case, facts), (sv.ragged_case(case), facts_ragged)):
            took = tuple(got[k] for k in ("path", "factors", "launches_per_exec"))
            want = (c["path"], c["factors"], c["launches_per_exec"])
            if took != want:
                msgs.append("%s [%s]: plan took path/factors/launches %s, the row names %s" % (c["id"], c["kernels"], took, want))
        spec = lambda lay: ", ".join("%s@%d%s" % (w, t, "" if p is None else "[%d]" % p) for t, w, p in lay["specials"])
        print("%s [%s] %d x %d: poison %s, clean neighbours bit-identical, scaling 2^%s; ragged layout x %d: poison %s, "
              "clean neighbours bit-identical: %s"
              % (case["id"], case["kernels"], case["n"], case["batch"], spec(case["layout"]),
                 "/".join("%+d" % s for s in sv.SCALES), case["ragged"]["batch"], spec(case["ragged"]["layout"]),
                 "ok" if not msgs else "%d FAILURES" % len(msgs)))
        bad += msgs
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("lg_scale", [-40, -20])
def test_device_generator_is_bit_identical_to_oracle_at_the_benchmark_scales(gpu, oracle, lg_scale):
    """The twin of test_gpu_parity.py::test_device_generator_is_bit_identical_to_oracle (scale 2^-7) at the scales bench.py
    and the timing tools fill their buffers at: the data the kernels are timed on."""
    fw, dev, queue = gpu
    n, batch = 4096, 9
    buf = dev.create_buffer(n * batch * 8)
    dev.fill_synthetic(buf, n, first_transform=3, scale=2.0 ** lg_scale)
    dev.poll()
    got = buf.map_read()
    want = oracle.gen_input(n, batch, first_transform=3, scale=2.0 ** lg_scale)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and it is the unit-scale data times that power of two, exactly: nothing flushed, nothing rounded
    unit = oracle.gen_input(n, batch, first_transform=3)
    assert np.array_equal(got.view(np.uint32), (unit.view(np.float32) * np.float32(2.0 ** lg_scale)).view(np.uint32))
    assert np.isfinite(got.view(np.float32)).all() and np.count_nonzero(got) > got.size - 8


@pytest.mark.parametrize("n,batch", sv.NORMALIZE_ROWS)
def test_normalize_keeps_the_pattern_and_scales_exactly(gpu, oracle, n, batch):
    fw, dev, queue = gpu
    bad = sv.run_normalize(fw, dev, queue, oracle, n, batch)
    print("normalize %d x %d: NaN / Inf pattern, finite samples bit-identical to normalize_ref, scaling 2^%s: %s"
          % (n, batch, "/".join("%+d" % s for s in sv.SCALES), "ok" if not bad else "%d FAILURES" % len(bad)))
    assert not bad, "\n".join(bad)
