"""GPU: the host-side ordering of fwa_plan_exec / fwa_plan_destroy (oracle/ordering.py: the scenarios, their shapes and the
geometry each one asserts).

What the header promises under "Threading" and what plan.cpp says about graph capture and plan lifetime, run for real:
an exec that forks to the chain streams captured into a hipGraph and replayed, two and three plans of one context on
their own caller streams, a plan destroyed with its exec in flight and its pooled ring handed on, one plan on
alternating caller streams ordered only on the device, HostPipeline over pipelined plans, the default two-chain geometry
of a tiled plan.  Every comparison is bit-identity with a solo, host-synchronised exec of the same geometry, which is
itself held to the fp64 DFT at REL_TOL.  tools/ordering_mutants.py runs the same scenarios on builds that lack one
ordering edge each (profiles/round7/ordering_mutants.jsonl).
"""
import pytest

from oracle import ordering
from oracle.device_run import open_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


@pytest.mark.parametrize("scenario", [s for _, s in ordering.SCENARIOS], ids=[i for i, _ in ordering.SCENARIOS])
def test_ordering_scenario(gpu, oracle, scenario):
    fw, dev, queue = gpu
    bad = scenario(fw, dev, queue, oracle)
    assert not bad, "\n".join(bad)
