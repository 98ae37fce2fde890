"""not-gpu: the error-budget record (tests/golden/error_budget.json) and the rule of oracle/error_budget.py.

The record must cover the whole matrix, sit under the cap, say which plan each case took and belong to the kernel sources
in the tree; the rule must have resolution: a numpy fp32 radix-2 FFT with correctly rounded twiddles passes the cap, the
same FFT with its twiddle angle evaluated in f32 -- 2-3x less accurate, yet 13-40x inside the flat 1e-5 -- fails it.
"""
import math
import re

import numpy as np
import pytest

from oracle import error_budget as eb


@pytest.fixture(scope="module")
def record():
    return eb.load_record()


def test_every_case_of_the_matrix_has_a_record(record):
    ids = [c["id"] for c in eb.MATRIX]
    assert len(ids) == len(set(ids))
    missing = [i for i in ids if i not in record["cases"]]
    assert not missing, "no record for %s: run tools/record_error_budget.py" % missing
    assert not set(record["cases"]) - set(ids), "entries of cases the matrix no longer has"


def test_matrix_covers_every_family_kind_and_sample_count():
    assert {c["kind"] for c in eb.MATRIX} == {"Forward", "Inverse", "Onlyinverse"}
    rows = {c["case"] for c in eb.MATRIX}
    for row in rows:
        assert sorted(c["kind"] for c in eb.MATRIX if c["case"] == row) == ["Forward", "Inverse", "Onlyinverse"]
    for c in eb.MATRIX:
        assert c["n"] > 1 and c["n"] & (c["n"] - 1) == 0
        assert c["n"] > 1 << 18 or c["n"] * c["batch"] >= eb.MIN_SAMPLES, c["id"]
    assert {c["n"] for c in eb.MATRIX if c["path"] == 0} == {1 << lg for lg in range(1, 16)}
    assert {c["n"] for c in eb.MATRIX if c["path"] == 2} == {1 << 10, 1 << 20}
    assert any(c["path"] == 1 for c in eb.MATRIX)
    assert {1 << 24, 1 << 25, 1 << 26} <= {c["n"] for c in eb.MATRIX if c["batch"] == 1}


def test_recorded_values_sit_under_the_cap(record):
    over = []
    for c in eb.MATRIX:
        rec = record["cases"][c["id"]]
        for key, top in (("rel_l2", eb.cap(c["n"])), ("max_rel", eb.MAX_REL_CAP_FACTOR * eb.cap(c["n"]))):
            if not 0.0 < rec[key] <= top:
                over.append((c["id"], key, rec[key], top))
    assert not over, over


def test_recorded_plans_are_the_ones_the_matrix_names(record):
    for c in eb.MATRIX:
        rec = record["cases"][c["id"]]
        assert (rec["path"], rec["factors"], rec["launches_per_exec"]) == (c["path"], c["factors"], c["launches_per_exec"]), c["id"]


def test_record_schema_and_stamp(record):
    assert set(record) == {"_comment", "stamp", "cases"}
    st = record["stamp"]
    assert re.fullmatch(r"[0-9a-f]{7,40}\+?", st["commit"]), st["commit"]
    assert st["kernel_sources"] == eb.KERNEL_SOURCE_DIR + "/*"
    assert re.fullmatch(r"[0-9a-f]{64}", st["kernel_source_sha256"])
    assert st["library"] == "product" and "gfx950" in st["device"]
    for cid, rec in record["cases"].items():
        assert set(rec) == {"rel_l2", "max_rel", "path", "factors", "launches_per_exec"}, cid
        assert all(isinstance(rec[k], float) and math.isfinite(rec[k]) for k in ("rel_l2", "max_rel")), cid
        assert all(isinstance(rec[k], int) for k in ("path", "factors", "launches_per_exec")), cid


def test_record_belongs_to_the_kernel_sources_in_the_tree(record):
    """A change under fft_wgpu_amd/csrc without a new record fails here, before the GPU suite has to find out."""
    assert record["stamp"]["kernel_source_sha256"] == eb.kernel_source_sha256(), \
        "kernel sources changed since the error budget was recorded: re-run tools/record_error_budget.py"


def test_rule_messages_name_case_value_record_and_cap():
    case = next(c for c in eb.MATRIX if c["id"] == "pipeline_2^20x4/Forward")
    rec = {"rel_l2": 1.0e-7, "max_rel": 2.0e-7}
    assert eb.check(case, {"rel_l2": 1.2e-7, "max_rel": 2.9e-7}, rec) == []
    bad = eb.check(case, {"rel_l2": 1.3e-7, "max_rel": 2.0e-7}, rec)
    assert len(bad) == 1 and "pipeline_2^20x4/Forward" in bad[0] and "1.3e-07" in bad[0] and "1e-07" in bad[0] and "cap" in bad[0]
    assert len(eb.check(case, {"rel_l2": 1.0e-7, "max_rel": 3.1e-7}, rec)) == 1
    assert len(eb.check(case, {"rel_l2": float("nan"), "max_rel": 2.0e-7}, rec)) == 2
    big = {"rel_l2": 1.0, "max_rel": 1.0}
    assert any("above the cap" in m for m in eb.check(case, {"rel_l2": 3e-7, "max_rel": 1e-7}, big))
    assert "no recorded entry" in eb.check(case, rec, None)[0]


def test_metric_matches_the_oracle_definition(oracle):
    n, batch = 256, 37
    x = oracle.gen_input(n, batch)
    r = oracle.dft_f64(x, n, -1)
    y = (r * (1 + 3e-7j) + 1e-6).astype(np.complex64)
    rel_l2, max_rel = eb.metrics(y, r, n)
    per = [oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n]) for t in range(batch)]
    assert max_rel == pytest.approx(max(p[0] for p in per), rel=1e-12)
    d = np.abs(y.astype(np.complex128) - r)
    assert rel_l2 == pytest.approx(np.sqrt((d ** 2).sum() / (np.abs(r) ** 2).sum()), rel=1e-12)
    y[5] = np.nan
    assert all(math.isnan(v) for v in eb.metrics(y, r, n))


def _model_fft(x, n, angle_f32):
    """fp32 radix-2 decimation-in-time FFT of the rows of x; twiddles f32(f64 cos / sin) as tables.cpp tw_f64 does, or
    (angle_f32) with the angle and cos / sin evaluated in f32."""
    lg = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(lg):
        rev |= ((idx >> b) & 1) << (lg - 1 - b)
    a = x.reshape(-1, n)[:, rev].astype(np.complex64)
    k = np.arange(n // 2)
    if angle_f32:
        th = np.float32(-2 * np.pi) * k.astype(np.float32) / np.float32(n)
        tw = (np.cos(th) + 1j * np.sin(th)).astype(np.complex64)
    else:
        th = -2 * np.pi * k / n
        tw = (np.cos(th).astype(np.float32) + 1j * np.sin(th).astype(np.float32)).astype(np.complex64)
    m = 1
    while m < n:
        a = a.reshape(a.shape[0], n // (2 * m), 2, m)
        t = a[:, :, 1, :] * tw[::n // (2 * m)][:m]
        u = a[:, :, 0, :]
        a = np.stack([u + t, u - t], axis=2)
        m *= 2
    return a.reshape(-1)


def test_cap_resolves_a_twiddle_angle_in_f32(oracle):
    for lg in range(10, 21):
        n = 1 << lg
        batch = max(1, eb.MIN_SAMPLES // n)
        x = oracle.gen_input(n, batch)
        r = np.fft.fft(x.astype(np.complex128).reshape(batch, n), axis=1).reshape(-1)
        good, _ = eb.metrics(_model_fft(x, n, False), r, n)
        assert good <= 0.7 * eb.cap(n), (lg, good, eb.cap(n))
        if lg >= 13:
            bad, bad_max = eb.metrics(_model_fft(x, n, True), r, n)
            assert bad > eb.cap(n), (lg, bad, eb.cap(n))
            assert bad_max < 1e-5 / 10                   # ... where the flat bound sees nothing
