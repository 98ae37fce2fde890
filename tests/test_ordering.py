"""not-gpu: the ordering scenarios (oracle/ordering.py) keep reaching every mechanism they were written for.

Each tag of ordering.MECHANISM_TAGS names one plan geometry -- the 2^20 pipeline and the tiled plans on two chains, the
three-pass plan, the single-chain plans that run on the caller's stream, the default two-chain tiled plan.  A scenario
list that lost one of them would still be green on the GPU.
"""
from conftest import REL_TOL

from oracle import ordering


def test_every_mechanism_has_a_scenario_and_names_its_geometry():
    ids = [i for i, _ in ordering.SCENARIOS]
    assert len(ids) == len(set(ids)) and all(callable(s) for _, s in ordering.SCENARIOS)
    for tag in ordering.MECHANISM_TAGS:
        assert any(tag in i.replace("+", "/").split("/") for i in ids), "no scenario runs the shape " + tag
        # every shape states the whole geometry its plans are held to, and no buffer is above ~450 MiB
        shape = ordering.SHAPES[tag]
        assert set(shape["want"]) == {"path", "factors", "launches_per_exec", "group", "streams"}, tag
        assert shape["n"] * shape["batch"] * 8 <= 450 << 20, tag
        groups = -(-shape["batch"] // shape["want"]["group"])
        passes = 3 if shape["want"]["factors"] >> 16 else 2
        assert shape["want"]["launches_per_exec"] == passes * groups and shape["want"]["streams"] <= groups, tag
    # the families of the issue, each with the cases it names
    count = {f: sum(i.startswith(f + "/") for i in ids) for f in {i.split("/")[0] for i in ids}}
    assert count == {"graph_forked": 7, "two_plans_two_streams": 3, "destroy_in_flight": 8, "alternating_streams": 2,
                     "host_pipeline": 2, "default_two_chains": 1}
    # the forked scenarios fork: two chains wherever a scenario is about the chain streams, one where it is about the
    # caller's stream; a result that is read after its plan has gone lives in the caller's src (even log2 n)
    for tag in ("P1", "T2", "T3", "D2"):
        assert ordering.SHAPES[tag]["want"]["streams"] == 2
    for tag in ("S1", "S2"):
        assert ordering.SHAPES[tag]["want"]["streams"] == 1 and ordering.SHAPES[tag]["n"].bit_length() % 2 == 1
    assert ordering.REL_TOL == REL_TOL
