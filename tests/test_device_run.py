"""not-gpu: the shared pieces the GPU tests and tools run their plans through -- _Plan.configure (fft_wgpu_amd/processor.py)
on a recording stand-in, PLAN_KEYS as the one key order over every case matrix, and the parity metric of
oracle/device_run.py against the C cross-check oracle.compare and against error_budget.metrics as it was before the block
walk was shared."""
import math

import numpy as np
import pytest

import test_gpu_containment as tc
from fft_wgpu_amd.processor import PLAN_KEYS, _Plan
from oracle import device_run as dr
from oracle import error_budget as eb
from oracle import impulse_sweep as im
from oracle import large_plans as lp
from oracle import ordering
from oracle import special_values as sv

FLAG_KEYS = ("colsw", "rows32", "p1_gen", "tile_ring")


# ---- configure ------------------------------------------------------------------------------------------------------
class StandIn:
    """records every set; holds what was set, or what `clamp` says instead"""
    configure = _Plan.configure

    def __init__(self, clamp=()):
        self.calls, self.held, self.clamp = [], {}, dict(clamp)

    def set(self, key, value):
        self.calls.append((key, value))
        self.held[key] = self.clamp.get(key, value)

    def get(self, key):
        return self.held[key]


def test_configure_sets_in_plan_keys_order_and_returns_what_the_plan_holds():
    plan = StandIn()
    given = {key: 3 + i for i, key in enumerate(reversed(PLAN_KEYS))}
    held = plan.configure(given)
    assert [k for k, _ in plan.calls] == list(PLAN_KEYS) and dict(plan.calls) == given
    assert held == {k: v for k, v in given.items() if k != "inject_launch_failure"}     # no getter: set, not read back
    plan = StandIn()
    assert plan.configure({"streams": 2, "factors": 0x0808, "group": 4}) == {"factors": 0x0808, "group": 4, "streams": 2}
    assert [k for k, _ in plan.calls] == ["factors", "group", "streams"]


def test_configure_rejects_an_unknown_key_before_any_set():
    plan = StandIn()
    with pytest.raises(ValueError, match="max_teams"):
        plan.configure({"group": 2, "max_teams": 1})
    assert plan.calls == []


def test_configure_names_a_key_the_plan_clamped():
    plan = StandIn(clamp={"group": 4})
    with pytest.raises(ValueError, match=r"set group = 8, the plan holds 4"):
        plan.configure({"factors": 0x0808, "group": 8, "streams": 2})
    assert [k for k, _ in plan.calls] == ["factors", "group"]           # it stops at the key that did not take
    plan = StandIn(clamp={"group": 4})
    assert plan.configure({"group": 8, "streams": 2}, verify=False) == {"group": 4, "streams": 2}


def test_configure_skips_none_values():
    plan = StandIn()
    assert plan.configure({"path": None, "small_reg": 1, "group": None}) == {"small_reg": 1}
    assert plan.calls == [("small_reg", 1)]


# ---- PLAN_KEYS is the key order of every matrix --------------------------------------------------------------------------
def _factors_first(tunables):
    """the order of the error-budget, special-value and impulse runners before configure: "factors" first, the rest as the
    dict lists them (a stable sort on `key != "factors"`)"""
    return [k for k, _ in sorted(tunables.items(), key=lambda kv: kv[0] != "factors")]


def _ordering_order(tunables):
    """the order of oracle/ordering.py before configure: its own three keys"""
    assert set(tunables) <= {"factors", "group", "streams"}
    return [k for k in ("factors", "group", "streams") if k in tunables]


def _plan_keys_order(tunables):
    return [k for k in PLAN_KEYS if k in tunables]


def _matrices():
    for case in eb.MATRIX:
        yield "error_budget " + case["id"], case["tunables"], _factors_first
    for case in sv.MATRIX:
        yield "special_values " + case["id"], case["tunables"], _factors_first
        yield "special_values " + case["id"] + "/ragged", sv.ragged_case(case)["tunables"], _factors_first
    for case in im.MATRIX:
        yield "impulse_sweep " + case["id"], case["tunables"], _factors_first
    for case in lp.MATRIX:
        yield "large_plans " + case["id"], case["tunables"], _plan_keys_order      # written for configure
    for tag, shape in ordering.SHAPES.items():
        yield "ordering " + tag, shape["tunables"], _ordering_order
    for spec in tc.build_specs():
        yield "containment " + spec["id"], spec["tunables"], _plan_keys_order


def test_plan_keys_order_is_the_previous_order_of_every_matrix_up_to_the_flag_keys():
    """The runners that configure replaced set the keys of a case in their own orders.  Under PLAN_KEYS every case sets the
    same keys, and with the four flag keys taken out, in the same order: only where "colsw", "rows32", "p1_gen" and
    "tile_ring" stand has changed.  fwa_plan_set_i64 only stores those four (tuning.cpp) and nothing reads them before the
    exec (plan.cpp exec_tiled, launches_per_exec), so they commute with every other key once "factors", which comes first
    in every order, has re-planned.  No case sets both "path" and "factors", whose order did differ."""
    seen = flagged = 0
    for name, tunables, previous in _matrices():
        assert set(tunables) <= set(PLAN_KEYS), name
        new, old = _plan_keys_order(tunables), previous(tunables)
        assert sorted(new) == sorted(old) == sorted(tunables), name
        assert [k for k in new if k not in FLAG_KEYS] == [k for k in old if k not in FLAG_KEYS], (name, old, new)
        assert not {"path", "factors"} <= set(tunables), name
        seen += 1
        flagged += new != old
    assert seen > 500 and flagged > 100          # the matrices are there, and the flag keys did move in many of them
    flags = [k for k in PLAN_KEYS if k in FLAG_KEYS]
    assert sorted(flags) == sorted(FLAG_KEYS) and PLAN_KEYS.index("factors") < min(PLAN_KEYS.index(k) for k in flags)


# ---- the parity metric against oracle.compare ----------------------------------------------------------------------------
def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


@pytest.fixture(scope="module")
def signals(oracle):
    """(n, y complex64, r complex128) at n = 2, 64, 4096, a few transforms each: the fp32 restatement against the fp64 DFT"""
    out = []
    for n, batch in ((2, 5), (64, 4), (4096, 3)):
        x = oracle.gen_input(n, batch, first_transform=n)
        y, r = oracle.forward_ref(x, n)[0], oracle.dft_f64(x, n, -1)
        y.setflags(write=False)
        r.setflags(write=False)
        out.append((n, y, r))
    return out


def _compare_all(oracle, y, r, n):
    return [oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n]) for t in range(y.size // n)]


def test_parity_equals_the_c_compare_transform_by_transform(oracle, signals):
    for n, y, r in signals:
        mx, l2 = dr.parity(y, r, n)
        assert mx.shape == l2.shape == (y.size // n,)
        for t, (cmx, cl2) in enumerate(_compare_all(oracle, y, r, n)):
            print("n %d transform %d: max_rel %.17g / %.17g (%.2f ulp), rel_l2 %.17g / %.17g (%.2f ulp)"
                  % (n, t, mx[t], cmx, _ulps(mx[t], cmx), l2[t], cl2, _ulps(l2[t], cl2)))
            assert cmx < 1e-5 and cl2 < 1e-5
            assert _ulps(mx[t], cmx) <= 1 and _ulps(l2[t], cl2) <= 1, (n, t)


def test_parity_propagates_a_nan_sample_as_compare_does(oracle, signals):
    for n, y, r in signals:
        y = y.copy()
        y[n + 1] = np.complex64(complex(np.nan, 0.0))                    # one sample of transform 1
        mx, l2 = dr.parity(y, r, n)
        ref = _compare_all(oracle, y, r, n)
        assert math.isnan(mx[1]) and math.isnan(l2[1]) and all(math.isnan(v) for v in ref[1])
        assert not np.isnan(np.delete(mx, 1)).any() and not np.isnan(np.delete(l2, 1)).any()
        bad, worst = dr.parity_failures(y, r, n, 1e-5)
        assert [t for t, _, _ in bad] == [1] and all(math.isnan(v) for v in worst)


def test_parity_takes_the_numerators_alone_on_an_all_zero_reference(oracle, signals):
    for n, y, r in signals:
        r = r.copy()
        r[:n] = 0
        mx, l2 = dr.parity(y, r, n)
        cmx, cl2 = oracle.compare(y[:n], r[:n])
        d = np.abs(y[:n].astype(np.complex128))
        assert _ulps(mx[0], d.max()) <= 1 and _ulps(mx[0], cmx) <= 1      # max_k |y - 0|
        assert _ulps(l2[0], cl2) <= 1                                    # sqrt(sum_k |y - 0|^2)
        assert abs(l2[0] - math.sqrt(float((d * d).sum()))) <= n * np.finfo(float).eps * l2[0]
        assert [t for t, _, _ in dr.parity_failures(y, r, n, 1e-5)[0]] == [0]


def test_parity_of_a_result_equal_to_its_reference_is_exactly_zero(oracle, signals):
    for n, y, _ in signals:
        mx, l2 = dr.parity(y, y.astype(np.complex128), n)
        assert (mx == 0).all() and (l2 == 0).all()
        assert dr.parity_failures(y, y.astype(np.complex128), n, 0.0) == ([], (0.0, 0.0))
        assert all(oracle.compare(y[t * n:(t + 1) * n], y[t * n:(t + 1) * n].astype(np.complex128)) == (0.0, 0.0)
                   for t in range(y.size // n))


def test_parity_walks_a_transform_longer_than_a_block_in_pieces(oracle, monkeypatch):
    n, batch = 4096, 3
    x = oracle.gen_input(n, batch)
    y, r = oracle.forward_ref(x, n)[0], oracle.dft_f64(x, n, -1)
    whole = dr.parity(y, r, n)
    monkeypatch.setattr(dr, "BLOCK", 1024)                                # four pieces per transform
    assert [d.shape for _, d, _ in dr.blocks(y, r, n)] == [(1, 1024)] * 12
    pieces = dr.parity(y, r, n)
    assert np.array_equal(whole[0], pieces[0])                            # a maximum does not depend on the walk
    # two orders of summing n positive terms differ by less than 2 n eps in each sum, so by less than that in sqrt(sd / sr)
    assert (np.abs(whole[1] - pieces[1]) <= 2 * n * np.finfo(float).eps * whole[1]).all()


# ---- error_budget.metrics returns what it returned before ----------------------------------------------------------------
def _metrics_before(y, r, n):
    """error_budget.metrics as it stood before it was built on device_run.blocks"""
    y = np.asarray(y).reshape(-1, n)
    r = np.asarray(r).reshape(-1, n)
    batch = y.shape[0]
    maxd = np.zeros(batch)
    maxr = np.zeros(batch)
    sd = sr = 0.0
    rows = max(1, (1 << 22) // n)
    cols = min(n, 1 << 22)
    for t0 in range(0, batch, rows):
        for k0 in range(0, n, cols):
            yb = y[t0:t0 + rows, k0:k0 + cols].astype(np.complex128)
            rb = r[t0:t0 + rows, k0:k0 + cols]
            d = np.abs(yb - rb)
            m = np.abs(rb)
            maxd[t0:t0 + rows] = np.maximum(maxd[t0:t0 + rows], d.max(axis=1))   # NaN-propagating
            maxr[t0:t0 + rows] = np.maximum(maxr[t0:t0 + rows], m.max(axis=1))
            sd += float((d * d).sum())
            sr += float((m * m).sum())
    rel_l2 = np.sqrt(sd / sr) if sr > 0 else np.sqrt(sd)
    return float(rel_l2), float(np.max(maxd / np.where(maxr > 0, maxr, 1.0)))


def _same_floats(a, b):
    return all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b)) and len(a) == len(b) == 2


def test_metrics_returns_the_floats_it_returned_before(oracle, signals):
    cases = []
    for n, y, r in signals:
        y_nan, r_zero = y.copy(), r.copy()
        y_nan[n + 1] = np.complex64(complex(np.nan, 0.0))
        r_zero[:n] = 0
        cases += [(n, y, r), (n, y_nan, r), (n, y, r_zero), (n, y, y.astype(np.complex128)), (n, y, np.zeros_like(r))]
    n = 1 << 23                                                           # two blocks per transform, two transforms
    x = oracle.gen_input(n, 2)
    cases.append((n, x, x.astype(np.complex128) * (1 + 1e-7)))
    for n, y, r in cases:
        assert _same_floats(eb.metrics(y, r, n), _metrics_before(y, r, n)), n
