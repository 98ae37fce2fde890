"""not-gpu: the per-class layer of the error budget (oracle/output_classes.py, error_budget.check_classes) has resolution and
hides nothing.

The complex64 model CLASS_FACTOR was derived from is run again: its table must reproduce and pass the class cap.  A model
result with the error of ONE class doubled -- a k mod T thread of k_small32, a K1 thread of a two-pass plan, an arithmetic
thread of k_chunk -- still passes the whole-buffer cap and pin and fails its class by name.  The maps are proven against the
prose they were written from, every class of every row holds at least 1024 samples, and the record
(tests/golden/error_budget_classes.json) covers the matrix on the kernel sources in the tree.
"""
import re

import numpy as np
import pytest

import side_sweeps as ss
from oracle import error_budget as eb
from oracle import output_classes as oc

CASES = {c["case"]: c for c in eb.MATRIX if c["kind"] == "Forward"}          # the maps do not depend on the kind


def _input_and_reference(oracle, case):
    n, batch = case["n"], case["batch"]
    x = oracle.gen_input(n, batch)
    return x, np.fft.fft(x.astype(np.complex128).reshape(batch, n), axis=1).reshape(-1)


def _measured(case, y, ref):
    """what eb.measure makes of a result: ((rel_l2, max_rel), {map: rel_l2 per class})"""
    sums = oc.ClassSums(case)
    return eb.metrics(y, ref, case["n"], sums), sums.errors()


def _own_record(case, errors):
    return oc.spread_record(oc.spread(errors, eb.cap(case["n"])))


# ---- the model: CLASS_FACTOR reproduces, and the model passes its cap --------------------------------------------------------
@pytest.fixture(scope="module")
def model_runs(oracle):
    """{row: (whole-buffer rel_l2, {map: rel_l2 per class})} of the model over MODEL_ROWS"""
    out = {}
    for row in oc.MODEL_ROWS:
        x, ref = _input_and_reference(oracle, CASES[row])
        whole, errors, _ = oc.model_row(CASES[row], x, ref)
        out[row] = (whole, errors)
    return out


def test_model_is_a_transform_in_both_directions(oracle):
    for n, lgs in ((8, (3,)), (2048, (11,)), (1 << 12, (6, 6)), (1 << 15, (5, 4, 6))):
        x = oracle.gen_input(n, 3)
        want = np.fft.fft(x.astype(np.complex128).reshape(3, n), axis=1).reshape(-1)
        back = np.fft.ifft(x.astype(np.complex128).reshape(3, n), axis=1).reshape(-1) * n
        for sign, r in ((-1, want), (1, back)):
            y = oc.model_fft(x, n, lgs, sign)
            assert y.dtype == np.complex64
            assert eb.metrics(y, r, n)[0] <= eb.cap(n), (n, lgs, sign)


def test_model_rows_are_every_one_launch_length_and_the_tiled_digit_shapes():
    one_launch = [r for r in oc.MODEL_ROWS if CASES[r]["path"] == 0]
    assert [CASES[r]["n"] for r in one_launch] == [1 << lg for lg in range(1, 16)]
    assert sorted(oc.digits(CASES[r]) for r in oc.MODEL_ROWS if CASES[r]["path"] == 7) == [[6, 6, 6], [6, 9, 6], [8, 8]]


def test_class_factor_follows_from_the_model(model_runs):
    """the derivation of the module's docstring: the worst (class / whole buffer) ratio, times 1.1, rounded up to 0.05"""
    ratios = {}
    for row, (whole, errors) in model_runs.items():
        if whole == 0.0:                                                  # n = 2: exact on this input, no ratio
            assert CASES[row]["n"] == 2 and all((e == 0).all() for e in errors.values())
            continue
        ratios[row] = max(float(e.max()) for e in errors.values()) / whole
        print("model %-22s whole %.3f of cap, classes %.3f .. %.3f of the whole" % (
            row, whole / eb.cap(CASES[row]["n"]), min(float(e.min()) for e in errors.values()) / whole, ratios[row]))
    assert len(ratios) == len(oc.MODEL_ROWS) - 1
    worst = max(ratios.values())
    assert worst <= oc.CLASS_FACTOR / 1.1, ratios
    assert oc.class_factor(worst) == pytest.approx(oc.CLASS_FACTOR, abs=1e-9), worst
    # ... and the table of the docstring is this one
    for row, ratio in ratios.items():
        line = re.search(r"^  %s +([\d.]+) +([\d.]+) +([\d.]+) " % re.escape(row), oc.__doc__, re.M)
        assert line, row
        assert float(line.group(3)) == pytest.approx(ratio, abs=0.02), (row, line.group(0), ratio)
        assert float(line.group(1)) == pytest.approx(model_runs[row][0] / eb.cap(CASES[row]["n"]), abs=0.02), row
    assert "= %.2f." % oc.CLASS_FACTOR in " ".join(oc.__doc__.split())


def test_model_passes_the_class_rule(model_runs):
    for row, (whole, errors) in model_runs.items():
        case = CASES[row]
        assert whole <= eb.cap(case["n"])
        assert eb.check_classes(case, errors, _own_record(case, errors)) == [], row
        assert all(hi <= oc.CLASS_FACTOR for lo, hi in oc.spread(errors, eb.cap(case["n"])).values()), row


# ---- one class at twice its error ------------------------------------------------------------------------------------------
def _thread_of_small32(case):
    T = case["n"] // 32
    return np.broadcast_to(np.arange(case["n"]) % T, (case["batch"], case["n"])), "k low 8 bits", lambda c: c % T


def _thread_of_pass_a(case):
    """256-point pass A: 16 points per thread, thread K1 mod 16"""
    assert oc.digits(case) == [8, 8]
    return np.broadcast_to(np.arange(case["n"]) % 256 % 16, (case["batch"], case["n"])), "K1", lambda c: c % 16


def _thread_of_chunk(case):
    return oc.chunk_maps(case["n"], case["batch"])["chunk thread"], "chunk thread", lambda c: c


@pytest.mark.parametrize("row,thread_of,thread", [("small32_10", _thread_of_small32, 5), ("tile_2^16x4", _thread_of_pass_a, 3),
                                                  ("chunk_64", _thread_of_chunk, 77)])
def test_one_class_at_twice_its_error_passes_the_whole_buffer_rule_and_fails_its_class(oracle, row, thread_of, thread):
    case = CASES[row]
    n = case["n"]
    x, ref = _input_and_reference(oracle, case)
    y = oc.model_fft(x, n, oc.digits(case))
    (rel_l2, max_rel), errors = _measured(case, y, ref)
    record = _own_record(case, errors)
    assert eb.check_classes(case, errors, record) == []

    threads, map_name, thread_of_class = thread_of(case)
    hit = (threads == thread).reshape(-1)
    doctored = y.astype(np.complex128)
    doctored[hit] = ref[hit] + 2.0 * (doctored[hit] - ref[hit])
    (bad_l2, _), bad_errors = _measured(case, doctored, ref)
    # the whole-buffer layer sees nothing: under the cap, inside the pin of the undoctored figure
    assert rel_l2 < bad_l2 <= min(eb.cap(n), eb.PIN_REL_L2 * rel_l2), (rel_l2, bad_l2, eb.cap(n))
    assert eb.check(case, dict(rel_l2=bad_l2, max_rel=max_rel), dict(rel_l2=rel_l2, max_rel=max_rel)) == []
    # the class layer names the map and classes of the doctored thread, and no other
    bad = eb.check_classes(case, bad_errors, record)
    assert bad, (row, oc.spread(bad_errors, eb.cap(n)))
    named = [re.search(r"^%s \[%s\], class (\d+) of '([^']+)': rel_l2 " % (re.escape(case["id"]), re.escape(case["kernels"])), m) for m in bad]
    assert all(named), bad
    assert map_name in {m.group(2) for m in named}
    own = [int(m.group(1)) for m in named if m.group(2) == map_name]
    assert own and all(thread_of_class(c) == thread for c in own), bad
    # every class of the doctored thread sits at twice its undoctored error in that map
    classes = np.flatnonzero(thread_of_class(np.arange(len(errors[map_name]))) == thread)
    assert np.allclose(bad_errors[map_name][classes], 2.0 * errors[map_name][classes], rtol=1e-6)


# ---- the rule's messages -----------------------------------------------------------------------------------------------------
def test_class_rule_messages_name_case_kernels_map_class_value_record_and_cap():
    case = CASES["small32_9"]
    c = eb.cap(case["n"])
    names = sorted(oc.maps_of(case))
    assert names == ["k high 8 bits", "k low 8 bits", "workgroup slot"]
    got = {"k high 8 bits": np.full(256, 0.5 * c), "k low 8 bits": np.full(256, 0.5 * c), "workgroup slot": np.full(16, 0.5 * c)}
    rec = {"class_maps": {name: [0.45, 0.5] for name in names}}
    assert eb.check_classes(case, got, rec) == []
    got["k low 8 bits"][200] = 0.63 * c                                  # 1.26 x the recorded worst class
    bad = eb.check_classes(case, got, rec)
    assert len(bad) == 1 and bad[0].startswith("small32_9/Forward [k_small32<9>], class 200 of 'k low 8 bits': rel_l2 %.4g > 1.25 x" % (0.63 * c))
    assert "%.4g" % (0.5 * c) in bad[0] and "%.2f x %.4g" % (oc.CLASS_FACTOR, c) in bad[0]
    got["k low 8 bits"][200] = 0.62 * c
    assert eb.check_classes(case, got, rec) == []
    loose = {"class_maps": {name: [0.45, 2.0] for name in names}}        # a bad record: the cap is the backstop
    got["workgroup slot"][3] = 1.01 * oc.CLASS_FACTOR * c
    bad = eb.check_classes(case, got, loose)
    assert len(bad) == 1 and "class 3 of 'workgroup slot'" in bad[0] and "above the class cap" in bad[0]
    got["k high 8 bits"][:] = np.nan                                       # a NaN fails, and the first 8 are kept
    assert len(eb.check_classes(case, got, loose)) == 8
    assert "no recorded entry" in eb.check_classes(case, got, None)[0]
    del rec["class_maps"]["workgroup slot"]
    assert "class maps" in eb.check_classes(case, got, rec)[0]


def test_class_sums_agree_with_the_side_libraries_metric(oracle):
    """ClassSums through eb.metrics against side_sweeps.class_errors on the written-out maps: one definition of rel-L2 per class"""
    for row in ("chunk_32", "small32_11", "factors_6_6_6_2^18x1"):
        case = CASES[row]
        x, ref = _input_and_reference(oracle, case)
        y = oc.model_fft(x, case["n"], oc.digits(case))
        _, errors = _measured(case, y, ref)
        shape = (case["batch"], case["n"])
        want = ss.class_errors(y.reshape(shape), ref.reshape(shape), oc.maps_of(case))
        assert sorted(errors) == sorted(want)
        for name in want:
            assert np.allclose(errors[name], want[name], rtol=1e-9), (row, name)


def test_class_sums_walk_the_blocks_of_a_transform_longer_than_one(monkeypatch):
    """n above the block size of the metric: the pieces of one transform land at their own k, also where a block ends inside
    a digit (one digit of 13 bits; 64 x 512 x 64 in blocks of 2^10)"""
    from oracle import device_run
    rng = np.random.default_rng(5)
    for case in (dict(id="x", n=1 << 13, batch=32, path=0, factors=13), dict(id="y", n=1 << 21, batch=1, path=7, factors=eb.pack_factors(6, 9, 6))):
        size = case["n"] * case["batch"]
        ref = rng.standard_normal(size) + 1j * rng.standard_normal(size)
        y = ref * (1 + 1e-7 * rng.standard_normal(size))
        with monkeypatch.context() as mp:
            _, whole = _measured(case, y, ref)
            mp.setattr(eb, "blocks", lambda y, r, n: _blocks_of(device_run, y, r, n, 1 << 10))
            _, pieces = _measured(case, y, ref)
        shape = (case["batch"], case["n"])
        want = ss.class_errors(y.reshape(shape), ref.reshape(shape), oc.maps_of(case))
        for name in want:
            assert np.allclose(pieces[name], want[name], rtol=1e-9) and np.allclose(whole[name], want[name], rtol=1e-9), (case["id"], name)
            assert len(want[name]) == 1 or np.ptp(want[name]) > 0


def _blocks_of(device_run, y, r, n, block):
    old, device_run.BLOCK = device_run.BLOCK, block
    try:
        yield from device_run.blocks(y, r, n)
    finally:
        device_run.BLOCK = old


def test_class_sums_refuse_thin_classes():
    with pytest.raises(AssertionError, match="fewer than 1024"):
        oc.ClassSums(dict(id="thin", n=1 << 10, batch=255, path=0, factors=10))
    oc.ClassSums(dict(id="full", n=1 << 10, batch=256, path=0, factors=10))


# ---- the maps against their prose ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << lg for lg in range(1, 9)])
def test_chunk_thread_map_is_what_the_kernel_header_says(n):
    """kernels_chunk.hip: a thread transforms 16 points of each half of its 64-KiB chunk: whole transforms up to n = 16; from
    32 on n / 16 threads share a transform and the last stage leaves thread t the outputs congruent to t mod n / 16"""
    batch = 3 * 8192 // n                                                # three chunks
    maps = oc.chunk_maps(n, batch)
    thread, half = maps["chunk thread"].reshape(3, 8192), maps["chunk half"].reshape(3, 8192)
    assert thread.min() == 0 and thread.max() == 255 and set(np.unique(half)) == {0, 1}
    assert (thread == thread[0]).all() and (half == half[0]).all()      # every chunk alike
    s = np.arange(8192)
    transform, k = s // n, s % n
    # a half is the first or the second 1024 samples of every wave's 2048
    assert np.array_equal(half[0], (s // 1024) % 2)
    for h in (0, 1):
        for t in range(256):
            mine = np.flatnonzero((thread[0] == t) & (half[0] == h))
            assert mine.size == 16, (n, t, h)
            if n <= 16:
                assert np.array_equal(mine, np.arange(mine[0], mine[0] + 16)) and mine[0] % 16 == 0     # 16 / n whole transforms
            else:
                assert len(set(transform[mine])) == 1 and len(set(k[mine] % (n // 16))) == 1
    if n >= 32:                                                          # the n / 16 threads of a transform are n / 16 different ones
        assert all(len(set(thread[0][transform == b])) == n // 16 for b in range(0, 8192 // n, 7))


@pytest.mark.parametrize("lg", range(9, 16))
def test_small32_thread_and_register_are_unions_of_window_classes(lg):
    """k_small32: output k belongs to thread k mod T and register k div T, T = n / 32.  The 32 registers and, up to T = 256,
    the threads are unions of whole classes of a window map; from T = 512 on a class of the low window is the threads
    congruent mod 256 -- 1024 threads of 2^18 samples would hold 256 samples each."""
    case = CASES["small32_%d" % lg]
    n, T = case["n"], case["n"] // 32
    maps = oc.maps_of(case)
    k = np.arange(n)

    def union_of(coarse, fine):
        """every class of `fine` lies inside one class of `coarse`"""
        return all(len(set(coarse[fine == c])) == 1 for c in np.unique(fine))
    assert union_of(k // T, maps["k high 8 bits"][0])
    if T <= 256:
        assert union_of(k % T, maps["k low 8 bits"][0])
    else:
        assert union_of(maps["k low 8 bits"][0], k % T) and np.array_equal(maps["k low 8 bits"][0], (k % T) % 256)
    if lg <= 13:
        slot = maps["workgroup slot"]
        assert slot.shape == (case["batch"], 1) and np.array_equal(slot[:, 0], np.arange(case["batch"]) % (256 // T))
    else:
        assert "workgroup slot" not in maps


def test_digit_windows_are_the_digits_of_the_output_index():
    for row, want in (("pipeline_2^20x4", [10, 10]), ("literal_2^20", [20]), ("tiled_2^24x1", [9, 7, 8]), ("chunk_16", [4]),
                      ("mid_tile_9_2^21x2", [6, 9, 6])):
        assert oc.digits(CASES[row]) == want
    case = CASES["mid_tile_9_2^21x2"]
    maps = oc.maps_of(case)
    k = np.arange(case["n"])
    K1, K2, K3 = k % 64, k // 64 % 512, k // (64 * 512)
    assert sorted(maps) == ["K1", "K2 high 8 bits", "K2 low 8 bits", "K3"]
    assert np.array_equal(maps["K1"][0], K1) and np.array_equal(maps["K3"][0], K3)
    assert np.array_equal(maps["K2 low 8 bits"][0], K2 % 256) and np.array_equal(maps["K2 high 8 bits"][0], K2 // 2)
    # the reduction the metric uses is bincount over those ids
    v = np.random.default_rng(1).standard_normal(case["n"])
    together = oc.all_window_sums(v, case)
    assert sorted(together) == sorted(maps)
    for name, w in oc.digit_windows(case).items():
        want = np.bincount(maps[name][0], weights=v)
        assert np.allclose(oc.window_sums(v, w), want, rtol=1e-9, atol=1e-9), name
        assert np.allclose(together[name], want, rtol=1e-9, atol=1e-9), name


@pytest.mark.parametrize("row", sorted(CASES))
def test_every_class_of_every_map_holds_enough_samples(row):
    case = CASES[row]
    counts = oc.class_counts(case)
    total = case["n"] * case["batch"]
    for name, count in counts.items():
        assert count.sum() == total and len(count) <= oc.MAX_CLASSES and count.min() >= oc.MIN_CLASS_SAMPLES, (row, name, count.min())
    oc.ClassSums(case)                                                   # ... so the metric does not refuse the row
    # map coverage: at least one map per digit; the kernel's own maps where the kernel has them
    lgs = oc.digits(case)
    for i in range(len(lgs)):
        prefix = "k" if len(lgs) == 1 else "K%d" % (i + 1)
        assert any(name == prefix or name.startswith(prefix + " ") for name in counts), (row, prefix)
    own = set(counts) - set(oc.digit_windows(case))
    if case["path"] == 0 and case["n"] <= 256:
        assert own == {"chunk thread", "chunk half"} and len(counts["chunk thread"]) == 256
    elif case["path"] == 0 and case["n"] <= 1 << 13:
        assert own == {"workgroup slot"}
    else:
        assert own == set()


# ---- the record --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    return eb.load_record(eb.CLASSES_RECORD_PATH)


def test_class_record_covers_the_matrix_under_the_stamp_of_the_tree(record):
    assert set(record) == {"_comment", "stamp", "cases"}
    assert sorted(record["cases"]) == sorted(c["id"] for c in eb.MATRIX)
    whole = eb.load_record()["stamp"]
    assert record["stamp"] == {k: whole[k] for k in ("commit", "kernel_sources", "kernel_source_sha256", "device", "library")}
    assert record["stamp"]["kernel_source_sha256"] == eb.kernel_source_sha256(), \
        "kernel sources changed since the per-class record was written: re-run tools/record_error_budget.py"


def test_recorded_classes_sit_under_the_class_cap(record):
    for c in eb.MATRIX:
        rec = record["cases"][c["id"]]
        assert set(rec) == {"per_class_min_of_cap", "per_class_max_of_cap", "class_maps"}, c["id"]
        assert set(rec["class_maps"]) == set(oc.digit_windows(c)) | set(oc.kernel_maps(c)), c["id"]
        for name, (lo, hi) in rec["class_maps"].items():
            assert 0.0 <= lo <= hi <= oc.CLASS_FACTOR and hi > 0.0, (c["id"], name, lo, hi)      # n = 2: output 0 is exact
        assert rec["per_class_max_of_cap"] == max(v[1] for v in rec["class_maps"].values())
        assert rec["per_class_min_of_cap"] == min(v[0] for v in rec["class_maps"].values())
