"""GPU parity tests (run on a real MI355X: `pytest -m gpu`).

Every transform goes through the C ABI (include/fft_wgpu_amd.h) via the thin
ctypes mirror; the CPU oracle (oracle/) is only the checker.

Tolerance (BASELINE.json north_star): <= 1e-5 relative fp32, measured per
transform as max_k|y-r| / max_k|r| and rel-L2 against the fp64 DFT (SURVEY.md
8(c)).  Integer/layout facts (result-buffer rule, generator) are bit-exact.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REF_ABS_TOL, REL_TOL
from oracle.device_run import open_gpu, upload
from parity_cases import check as _check, fixture_sizes_body, hip_runtime, run as _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


# ---- K1: the reference's own known answers, through the reference's call sequence ----
def test_reference_known_answers(gpu, known_answers):
    fw, dev, queue = gpu
    batch = 500 * 5  # examples/basic_inverse.rs:160 uses 512*500*5 samples
    for case in known_answers["cases"]:
        n = case["n"]
        c = np.complex64(complex(*case["c"]))
        x = np.full(n * batch, c, dtype=np.complex64)
        expect = np.zeros(n * batch, dtype=np.complex64)
        if case["plan"] == "Forward":
            y, which, _ = _run(fw, dev, queue, "Forward", x, n)
            expect[::n] = c * n
        elif case["plan"] == "Inverse":
            y, which, _ = _run(fw, dev, queue, "Inverse", x, n)
            expect[::n] = c
        else:
            # examples/basic_inverse2.rs:76-92: Onlyinverse then Normalize in one encoder
            src = upload(dev, queue, x)
            src2 = dev.create_buffer(x.nbytes)
            oi = fw.Onlyinverse(dev, queue, src, src2, n)
            nm = fw.Normalize(dev, queue, src, src2, n)
            enc = dev.create_command_encoder()
            out1 = oi.proc(enc)
            out2 = nm.proc(enc)
            queue.submit(enc.finish())
            y = out2.map_read(stream=enc)
            which = 0 if out1 is src else 1
            # processor.rs:433-439: normalize writes the buffer the inverse did NOT end in
            assert (out2 is src2) == (out1 is src)
            expect[::n] = c
        err = max(np.abs(y.real - expect.real).max(), np.abs(y.imag - expect.imag).max())
        assert err < REF_ABS_TOL, (case, err)  # examples/basic_inverse.rs:238-253
        assert which == int(np.log2(n)) % 2    # processor.rs:153-157


# ---- K4: numpy float64 fixtures, every power of two 2..1024 (parity_cases.fixture_sizes_body) ----
@pytest.mark.parametrize("path,small_reg", [(None, 1), (2, None)])
def test_fixture_sizes(gpu, oracle, k4, path, small_reg):
    fixture_sizes_body(gpu, k4, path, small_reg)


def test_literal_recurrence_matches_restatement_bitwise_shape(gpu, oracle):
    """path=2 is the reference recurrence one launch per stage (fft.wgsl:27-62); its distance to the
    CPU restatement of the same recurrence is pure fma-contraction noise."""
    fw, dev, queue = gpu
    n, batch = 4096, 3
    x = oracle.gen_input(n, batch)
    y, _, _ = _run(fw, dev, queue, "Forward", x, n, path=2)
    yr, _ = oracle.forward_ref(x, n)
    d = np.abs(y.astype(np.complex128) - yr.astype(np.complex128)).max() / np.abs(yr).max()
    assert d <= 2e-6, d


# ---- size sweep incl. ragged batches, 64-bit-free small cases ----
@pytest.mark.parametrize("lg,batch", [(0, 5), (1, 7), (2, 1), (3, 1000), (4, 1), (5, 33), (6, 129), (9, 2500),
                                      (10, 1), (11, 5), (12, 3), (13, 2), (14, 3), (15, 3), (16, 2), (17, 5), (18, 1),
                                      (19, 3), (20, 1), (20, 3), (21, 1), (22, 3), (23, 1), (25, 1), (26, 1)])
def test_size_sweep(gpu, oracle, lg, batch):
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    y, which, _ = _run(fw, dev, queue, "Forward", x, n)
    assert which == lg % 2
    _check(y, oracle.dft_f64(x, n, -1), n)
    # K5: forward then scaled inverse is the identity
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n)
    _check(z, x.astype(np.complex128), n)


# ---- C1 / C2 / C5 shapes ----
def test_config_c1_n1024_batch1(gpu, oracle):
    fw, dev, queue = gpu
    x = oracle.gen_input(1024, 1)
    y, which, _ = _run(fw, dev, queue, "Forward", x, 1024)
    assert which == 0
    mx, l2 = _check(y, oracle.dft_f64(x, 1024, -1), 1024)
    yr, _ = oracle.forward_ref(x, 1024)
    print("C1 max_rel %.3g rel_l2 %.3g; vs fp32 restatement %.3g" % (
        mx, l2, np.abs(y - yr).max() / np.abs(yr).max()))


# the 2^20 two-pass pipeline: (batch, group, streams, tile width); batches below 4 take the tiled path unless
# the plan is re-tuned, so C2 (batch 1) is checked on both
def _c2_n1m_body(gpu, oracle, batch, group, streams, tile_w):
    fw, dev, queue = gpu
    n = 1 << 20
    x = oracle.gen_input(n, batch)
    # a group holds at most the batch and there are at most as many chains as groups (build_pipeline): (4, 8, 2) and
    # (9, 16, 2) name one group on one chain, and the keys are set to what the plan will hold (they are read back)
    group = min(group, batch)
    streams = min(streams, -(-batch // group))
    kw = dict(group=group, streams=streams, tile_w=tile_w)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n, **kw)
    assert which == 0 and facts["path"] == 1 and facts["group"] == group
    r = oracle.dft_f64(x, n, -1)
    mx, l2 = _check(y, r, n)
    print("C2-shape batch %d: max_rel %.3g rel_l2 %.3g" % (batch, mx, l2))
    # K8 batch independence: transform b of the batch == the same data in a different batch position / geometry
    b = batch - 1
    y1, _, _ = _run(fw, dev, queue, "Forward", np.concatenate([x[b * n:(b + 1) * n]] * 4), n, tile_w=tile_w)
    assert np.array_equal(y1[:n].view(np.uint32), y[b * n:(b + 1) * n].view(np.uint32))
    # inverse family on the fast path
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n, **kw)
    _check(z, x.astype(np.complex128), n)


@pytest.mark.parametrize("batch,group,streams,tile_w", [(4, 8, 2, 16), (5, 2, 1, 16), (17, 4, 3, 16), (9, 16, 2, 16), (23, 3, 2, 16)])
def test_config_c2_n1m(gpu, oracle, batch, group, streams, tile_w):
    _c2_n1m_body(gpu, oracle, batch, group, streams, tile_w)


def test_config_c2_n1m_batch1(gpu, oracle):
    """BASELINE config C2: one 2^20 transform.  Too few tiles for the two-pass pipeline: the plan takes the
    three-pass tiled form (64 x 64 x 256); the result must match the pipeline's to rounding."""
    fw, dev, queue = gpu
    n = 1 << 20
    x = oracle.gen_input(n, 1)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n)
    assert which == 0 and facts["path"] == 7
    mx, l2 = _check(y, oracle.dft_f64(x, n, -1), n)
    print("C2 max_rel %.3g rel_l2 %.3g" % (mx, l2))
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n)
    _check(z, x.astype(np.complex128), n)


GEOMETRIES_16 = (dict(tile_w=16), dict(tile_w=16, xcd_swizzle=0), dict(tile_w=16, group=5, streams=3), dict(group=7, streams=1),
                 dict(group=32, streams=2), dict(group=3, streams=4),
                 # round 4: the pair map (xcd_swizzle bit 2: the two residents of a CU take adjacent tiles) -- the default (5);
                 # active when an XCD gets whole runs of 64 tiles (group 16, 8), plain mapping otherwise (group 7, 20)
                 dict(group=16, streams=1), dict(group=8, streams=1), dict(group=16, streams=2, xcd_swizzle=1),
                 dict(group=20, streams=1, xcd_swizzle=7), dict(group=16, streams=1, xcd_swizzle=1))


def _n1m_geometries_body(gpu, oracle, geometries):
    """Group size, stream count and tile width change how the intermediate is laid out and handed over, never
    the arithmetic: every geometry must reproduce the default result bit for bit, also when the buffer is much
    larger than L2 / Infinity Cache and execs run back to back (a stale-line hazard shows up as mismatching
    128-byte lines)."""
    fw, dev, queue = gpu
    n, batch = 1 << 20, 96                      # 768 MiB: far beyond L2 (32 MiB) and Infinity Cache (256 MiB)
    x = oracle.gen_input(n, batch, first_transform=5)
    ref, _, _ = _run(fw, dev, queue, "Forward", x, n)
    mx, _ = oracle.compare(ref[:n], oracle.dft_f64(x[:n], n, -1))
    assert mx <= REL_TOL
    for kw in geometries:
        for rep in range(2):
            y, _, _ = _run(fw, dev, queue, "Forward", x, n, **kw)
            bad = np.flatnonzero(y.view(np.uint64) != ref.view(np.uint64))
            assert bad.size == 0, (kw, rep, bad.size, bad[:8])


def test_n1m_pipeline_geometries_are_bit_identical(gpu, oracle):
    _n1m_geometries_body(gpu, oracle, GEOMETRIES_16)


@pytest.mark.parametrize("lg,batch", [(16, 600), (17, 300), (19, 70), (21, 19), (22, 9), (24, 3)])
def test_tiled_block_maps_are_bit_identical(gpu, oracle, lg, batch):
    """Key "xcd_swizzle" on the tiled plans (xcd_map, device_common.h: bit 0 = every XCD takes a contiguous run of tiles, bit 2 =
    the two residents of a CU take adjacent tiles; per-size defaults since round 4: 5 at 2^16 / 2^21, 1 at 2^17 .. 2^19, 0 elsewhere).
    A map only decides which workgroup takes which tile: every value gives the same bits, with full groups (runs of 64 per XCD:
    the pair map is active), ragged last groups (plain mapping) and both chains; the default agrees with the f64 DFT."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    ref, _, facts = _run(fw, dev, queue, "Forward", x, n)
    assert facts["path"] == 7 and facts["xcd_swizzle"] == {16: 5, 17: 1, 19: 1, 21: 5}.get(lg, 0)
    _check(ref[:2 * n], oracle.dft_f64(x[:2 * n], n, -1), n)
    for swz in (0, 1, 5):
        y, _, f = _run(fw, dev, queue, "Forward", x, n, xcd_swizzle=swz)
        assert f["xcd_swizzle"] == swz
        assert np.array_equal(y.view(np.uint64), ref.view(np.uint64)), (lg, swz)


def test_n1m_matches_literal_recurrence(gpu, oracle):
    fw, dev, queue = gpu
    n = 1 << 20
    x = oracle.gen_input(n, 4, first_transform=11)
    y_fast, _, _ = _run(fw, dev, queue, "Forward", x, n)
    y_lit, _, _ = _run(fw, dev, queue, "Forward", x, n, path=2)
    d = np.abs(y_fast.astype(np.complex128) - y_lit).max() / np.abs(y_lit).max()
    assert d <= REL_TOL, d


# ---- distance to the fp32 restatement of the reference (oracle/ref_fft.c), all three transforming plans ----
# One case per BASELINE.json config shape that fits the CPU restatement in seconds and per kernel family (VERDICT round 4,
# item 3): what each case runs is asserted through the plan's path / factors / launch count below.
_DISTANCE_CASES = [
    # (n, batch, expected (path, factors, launches per exec), kernels)
    (256, 40, (0, None, 1), "k_chunk"),
    (512, 20, (0, None, 1), "k_small32<9> (the reference's own length, examples/basic.rs:32)"),
    (1024, 1, (0, None, 1), "k_small32<10>: config C1's shape"),
    (1 << 13, 6, (0, None, 1), "k_small32<13>: two exchanges"),
    (1 << 15, 3, (0, None, 1), "k_small32<15>: 1024 threads"),
    (1 << 16, 2, (7, 8 | 8 << 8, 2), "latency regime: k_tile columns + k_tile rows (256 x 256)"),
    (1 << 17, 9, (7, 8 | 9 << 8, 2), "k_colsw<8,64> + k_rows32<9>"),
    (1 << 20, 1, (7, 6 | 6 << 8 | 8 << 16, 3), "config C2: three balanced k_tile passes"),
    (1 << 20, 4, (1, 10 | 10 << 8, 2), "k_p1_1m + k_p2_1m: config C3's pipeline"),
    (1 << 22, 2, (7, 10 | 12 << 8, 2), "k_p1_gen + k_rows32<12>"),
    (1 << 23, 1, (7, 11 | 12 << 8, 2), "k_cols32<11> + k_rows32<12>"),
    (1 << 24, 1, (7, 9 | 7 << 8 | 8 << 16, 3), "config C5: k_colsw<9,32> + k_tile columns + k_tile rows"),
]


@pytest.mark.parametrize("n,batch,shape,kernels", _DISTANCE_CASES, ids=["%dx%d" % (c[0], c[1]) for c in _DISTANCE_CASES])
def test_distance_to_reference_restatement(gpu, oracle, n, batch, shape, kernels):
    """HIP result vs the CPU restatement of the reference's own arithmetic -- forward: table twiddles
    (processor.rs:43-49, fft.wgsl:27-62); inverse: on-the-fly f32 cos/sin twiddles per butterfly and the fused 1/n of
    the last stage (ifft.wgsl:41-42,65-74) where this library uses conjugated f64-derived tables; Onlyinverse: the same
    without the scale (onlyifft.wgsl:25-64).  Bound: the north-star 1e-5 (max-abs error / max-abs reference, per
    transform), at every config shape and for every kernel family.  With FWA_DISTANCE_TABLE=<file> every case appends
    its numbers (BASELINE.md's table), the restatement's own distance to the fp64 DFT beside them."""
    import json
    fw, dev, queue = gpu
    x = oracle.gen_input(n, batch, first_transform=3)
    rows = []
    for kind, ref, direction in (("Forward", oracle.forward_ref, -1), ("Inverse", oracle.inverse_ref, 1),
                                 ("Onlyinverse", oracle.onlyinverse_ref, 1)):
        y, which, facts = _run(fw, dev, queue, kind, x, n)
        path, factors, launches = shape
        assert facts["path"] == path and facts["launches_per_exec"] == launches, (facts["path"], facts["launches_per_exec"])
        if factors is not None:
            assert facts["factors"] == factors, hex(facts["factors"])
        yr, which_ref = ref(x, n)
        assert which == which_ref == int(np.log2(n)) % 2   # processor.rs:153-157
        exact = oracle.dft_f64(x, n, direction)
        if kind == "Inverse":
            exact = exact / n
        worst = ours = theirs = 0.0
        for t in range(batch):
            a, r = y[t * n:(t + 1) * n].astype(np.complex128), yr[t * n:(t + 1) * n].astype(np.complex128)
            e = exact[t * n:(t + 1) * n]
            worst = max(worst, np.abs(a - r).max() / np.abs(r).max())
            ours = max(ours, np.abs(a - e).max() / np.abs(e).max())
            theirs = max(theirs, np.abs(r - e).max() / np.abs(e).max())
        assert worst <= REL_TOL, (kind, n, worst)
        print("%s n=%d x %d [%s]: max distance to the fp32 restatement of the reference %.3g (to the fp64 DFT: HIP %.3g, restatement %.3g)"
              % (kind, n, batch, kernels, worst, ours, theirs))
        rows.append({"n": n, "batch": batch, "plan": kind, "kernels": kernels, "hip_vs_restatement": worst,
                     "hip_vs_dft_f64": ours, "restatement_vs_dft_f64": theirs})
    if os.environ.get("FWA_DISTANCE_TABLE"):
        with open(os.environ["FWA_DISTANCE_TABLE"], "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


# ---- tiled path: several groups, two chains, ragged last group, 16- and 32-wide tiles ----
@pytest.mark.parametrize("lg,batch", [(16, 7), (17, 7), (18, 7), (19, 7), (22, 5), (21, 3)])
def test_tiled_groups_chains_ragged(gpu, oracle, lg, batch):
    """group = 2 with two internal streams and an odd batch: per-group slab rotation, fork/join of the chains,
    the ragged last group and in-place operation at group granularity (default plans have one group at these
    batch sizes)."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    r = oracle.dft_f64(x, n, -1)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n, group=2, streams=2)
    assert facts["path"] == 7 and facts["group"] == 2 and which == lg % 2
    assert (facts["factors"] >> 16 == 0) == (lg <= 19 or lg in (21, 22, 23))   # two passes up to 2^19 and at 2^21 .. 2^23
    _check(y, r, n)
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n, group=2, streams=2)
    _check(z, x.astype(np.complex128), n)
    # a different geometry computes the same bits
    y2, _, _ = _run(fw, dev, queue, "Forward", x, n, group=3, streams=1)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))


def test_tiled_default_group_with_many_groups(gpu, oracle):
    """Default geometry, batch > 2 x group: 2^16 x 600 (group = 256 transforms per 128-MiB slab)."""
    fw, dev, queue = gpu
    n, batch = 1 << 16, 600
    x = oracle.gen_input(n, batch, first_transform=1)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n)
    assert facts["path"] == 7 and facts["group"] == 256 and which == 0
    r = oracle.dft_f64(x, n, -1)
    for t in (0, 255, 256, 511, 512, 599):
        mx, l2 = oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n])
        assert mx <= REL_TOL and l2 <= REL_TOL, (t, mx, l2)


@pytest.mark.parametrize("lg,factors", [(18, (9, 9, 0)), (18, (6, 6, 6)), (20, (7, 7, 6)), (20, (10, 10, 0)),
                                        (16, (8, 8, 0)), (16, (10, 6, 0)), (24, (8, 8, 8)), (24, (10, 7, 7))])
def test_refactorised_plans_agree(gpu, oracle, lg, factors):
    """Key "factors": any factorisation of n into 64..1024-point passes computes the same transform."""
    fw, dev, queue = gpu
    n, batch = 1 << lg, 4 if lg <= 20 else 1
    x = oracle.gen_input(n, batch, first_transform=lg)
    packed = factors[0] | (factors[1] << 8) | (factors[2] << 16)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n, factors=packed)
    assert facts["path"] == 7 and facts["factors"] == packed and which == lg % 2
    _check(y, oracle.dft_f64(x, n, -1), n)


@pytest.mark.parametrize("lg,factors,batch", [(16, (10, 6, 0), 9), (18, (10, 8, 0), 7), (19, (10, 9, 0), 3), (20, (10, 10, 0), 2),
                                              (24, (10, 7, 7), 1), (26, (10, 8, 8), 1), (28, (10, 9, 9), 1)])
def test_first_pass_1024_column_kernel(gpu, oracle, lg, factors, batch):
    """Key "p1_gen": tiled plans whose first factor is 1024 run the 2^20 pipeline's column kernel at a run-time pitch
    (k_p1_gen, twiddles of domain n computed per tile) as pass A; p1_gen = 0 runs the generic tile kernel.  Both against
    the f64 DFT (up to 2^24) and against each other (every size; forward and inverse; ragged groups).  The 2^20 case runs on a
    context of its own, as that context's first plan: k_p1_gen has its own kernel family and needs no setup of the 2^20
    pipeline's kernels, which no plan of that context ever launches."""
    fw, dev, queue = gpu
    if lg == 20:
        dev = fw.Device(0)
        queue = fw.Queue(dev)
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    packed = factors[0] | (factors[1] << 8) | (factors[2] << 16)
    extra = dict(group=2, streams=2) if batch > 2 else {}
    for kind in ("Forward", "Inverse"):
        y1, which, facts = _run(fw, dev, queue, kind, x, n, factors=packed, p1_gen=1, **extra)
        assert facts["path"] == 7 and facts["p1_gen"] == 1 and which == lg % 2
        y0, _, facts0 = _run(fw, dev, queue, kind, x, n, factors=packed, p1_gen=0, **extra)
        assert facts0["p1_gen"] == 0
        mx, l2 = oracle.compare(y1, y0.astype(np.complex128))
        assert mx <= 2e-6 and l2 <= 1e-6, (lg, kind, mx, l2)
        if lg <= 24 and kind == "Forward":
            _check(y1, oracle.dft_f64(x, n, -1), n)
    if lg == 20:
        dev.destroy()


@pytest.mark.parametrize("lg,factors,batch", [(22, (11, 11, 0), 3), (21, (11, 10, 0), 2), (17, (11, 6, 0), 9), (24, (11, 6, 7), 1),
                                              (28, (11, 8, 9), 1)])
def test_first_pass_2048_column_kernel(gpu, oracle, lg, factors, batch):
    """k_cols32: pass A of plans whose first factor is 2048 (the default at 2^23 = 2048 x 4096; any other
    factorisation through the "factors" key), forward and inverse, ragged groups, against the f64 DFT up to 2^24 and
    against the default plan of the size above that."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    packed = factors[0] | (factors[1] << 8) | (factors[2] << 16)
    extra = dict(group=2, streams=2) if batch > 2 else {}
    y, which, facts = _run(fw, dev, queue, "Forward", x, n, factors=packed, **extra)
    assert facts["path"] == 7 and facts["factors"] == packed and which == lg % 2
    if lg <= 24:
        _check(y, oracle.dft_f64(x, n, -1), n)
    else:
        y0, _, _ = _run(fw, dev, queue, "Forward", x, n)
        mx, l2 = oracle.compare(y, y0.astype(np.complex128))
        assert mx <= 2e-6 and l2 <= 1e-6, (lg, mx, l2)
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n, factors=packed, **extra)
    _check(z, x.astype(np.complex128), n)


@pytest.mark.parametrize("lg,factors,batch,tile_ring", [(20, (9, 11, 0), 5, 1), (20, (9, 11, 0), 3, 0), (20, (8, 12, 0), 3, 1),
                                                        (20, (8, 12, 0), 2, 0), (19, (9, 10, 0), 5, 1), (19, (8, 11, 0), 3, 1),
                                                        (18, (9, 9, 0), 7, 1), (18, (8, 10, 0), 5, 1), (17, (9, 8, 0), 9, 1),
                                                        (16, (8, 8, 0), 9, 1), (21, (9, 12, 0), 3, 1), (24, (9, 7, 8), 1, 1),
                                                        (26, (8, 9, 9), 1, 1)])
def test_first_pass_short_wide_column_kernel(gpu, oracle, lg, factors, batch, tile_ring):
    """Key "colsw": k_colsw as pass A -- 512-row x 32-column or 256-row x 64-column tiles (256- / 512-byte HBM segments, 512
    threads, two workgroups per CU) -- with the tile-contiguous ring read back by k_rows32 ("tile_ring" = 1, where the
    last pass supports it) or the matrix layout.  Forward and inverse against the f64 DFT (up to 2^24; the default plan
    above), ragged groups and both chains; bit-identical between the two ring layouts."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    packed = factors[0] | (factors[1] << 8) | (factors[2] << 16)
    extra = dict(group=2, streams=2) if batch > 2 else {}
    y, which, facts = _run(fw, dev, queue, "Forward", x, n, factors=packed, colsw=1, tile_ring=tile_ring, **extra)
    assert facts["path"] == 7 and facts["factors"] == packed and facts["colsw"] == 1 and which == lg % 2
    if lg <= 24:
        _check(y, oracle.dft_f64(x, n, -1), n)
    else:
        y0, _, _ = _run(fw, dev, queue, "Forward", x, n)
        mx, l2 = oracle.compare(y, y0.astype(np.complex128))
        assert mx <= 2e-6 and l2 <= 1e-6, (lg, mx, l2)
    if tile_ring:
        y_m, _, _ = _run(fw, dev, queue, "Forward", x, n, factors=packed, colsw=1, tile_ring=0, **extra)
        assert np.array_equal(y.view(np.uint32), y_m.view(np.uint32))
    z, _, _ = _run(fw, dev, queue, "Inverse", y, n, factors=packed, colsw=1, tile_ring=tile_ring, **extra)
    _check(z, x.astype(np.complex128), n)


@pytest.mark.parametrize("lg,factors,batch", [(19, (10, 9, 0), 5), (20, (10, 10, 0), 3), (21, (10, 11, 0), 3), (18, (9, 9, 0), 7),
                                              (22, (10, 12, 0), 3), (23, (11, 12, 0), 2), (18, (6, 12, 0), 9),
                                              (17, (6, 11, 0), 9), (20, (9, 11, 0), 2)])
def test_last_pass_rows32_kernel(gpu, oracle, lg, factors, batch):
    """Key "rows32": two-pass tiled plans whose second factor is 512 / 1024 / 2048 run k_rows32 (32 points per thread, 16
    adjacent rows per workgroup, last register stage in the transposed role) as their last pass; rows32 = 0 runs the
    generic tile kernel (no 2048 there).  Forward and inverse against the f64 DFT, ragged groups and both chains."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=lg)
    packed = factors[0] | (factors[1] << 8)
    extra = dict(group=2, streams=2) if batch > 2 else {}
    r = oracle.dft_f64(x, n, -1)
    y1, which, facts = _run(fw, dev, queue, "Forward", x, n, factors=packed, rows32=1, **extra)
    assert facts["path"] == 7 and facts["rows32"] == 1 and facts["launches_per_exec"] == 2 * ((batch + facts["group"] - 1) // facts["group"])
    assert which == lg % 2
    _check(y1, r, n)
    if factors[1] <= 10:
        y0, _, facts0 = _run(fw, dev, queue, "Forward", x, n, factors=packed, rows32=0, **extra)
        assert facts0["rows32"] == 0
        mx, l2 = oracle.compare(y1, y0.astype(np.complex128))
        assert mx <= 2e-6 and l2 <= 1e-6, (lg, mx, l2)
    z, _, _ = _run(fw, dev, queue, "Inverse", y1, n, factors=packed, rows32=1, **extra)
    _check(z, x.astype(np.complex128), n)


@pytest.mark.parametrize("lg,batch,factors", [(16, 1, (8, 8, 0)), (16, 16, (8, 8, 0)), (16, 17, (8, 8, 0)), (17, 8, (8, 9, 0)),
                                              (17, 9, (8, 9, 0)), (18, 1, (6, 6, 6)), (18, 4, (6, 6, 6)), (18, 5, (8, 10, 0)), (19, 2, (6, 6, 7)),
                                              (19, 3, (9, 10, 0)), (20, 3, (6, 6, 8)), (21, 1, (7, 7, 7)), (21, 2, (10, 11, 0)),
                                              (22, 1, (7, 7, 8)), (22, 2, (10, 12, 0)), (23, 1, (11, 12, 0)), (24, 1, (9, 7, 8))])
def test_plan_picks_small_tiles_for_few_transforms(gpu, oracle, lg, batch, factors):
    """Latency regime (at most 2^20 samples per exec, a single 2^21, fewer than 4 of 2^20): balanced small tiles so that
    every CU gets work (k_tile, "colsw" = 0); above it fat 16 Ki-point first-pass tiles (k_colsw up to 2^19 and from 2^24,
    the 1024-point column kernels between).  Either way the transform is the same."""
    fw, dev, queue = gpu
    n = 1 << lg
    x = oracle.gen_input(n, batch, first_transform=100 + lg)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n)
    assert facts["path"] == 7 and which == lg % 2
    assert facts["factors"] == factors[0] | (factors[1] << 8) | (factors[2] << 16)
    few = (lg < 20 and batch <= (1 << 20 >> lg)) or (lg in (21, 22) and batch == 1) or (lg == 20 and batch < 4)
    assert facts["colsw"] == (0 if few else int(lg <= 19 or lg >= 24))
    _check(y, oracle.dft_f64(x, n, -1), n)


def test_config_c5_n16m_batch1(gpu, oracle):
    fw, dev, queue = gpu
    n = 1 << 24
    x = oracle.gen_input(n, 1)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n)
    assert which == 0 and facts["path"] == 7 and facts["factors"] == (9 | (7 << 8) | (8 << 16))  # tiled: 512 x 128 x 256 -- k_colsw (512 x 32 column tiles), then two k_tile passes
    mx, l2 = _check(y, oracle.dft_f64(x, n, -1), n)
    print("C5 max_rel %.3g rel_l2 %.3g" % (mx, l2))


# ---- properties ----
def test_impulse_tone_parseval_linearity(gpu, oracle):
    fw, dev, queue = gpu
    for n in (256, 1 << 20):
        k = np.arange(n)
        p, q = 5, 37
        x = np.zeros(n, np.complex64); x[p] = 1
        y, _, _ = _run(fw, dev, queue, "Forward", x, n)
        _check(y, np.exp(-2j * np.pi * ((p * k) % n) / n), n)            # K2
        x = np.exp(2j * np.pi * ((q * k) % n) / n).astype(np.complex64)
        y, _, _ = _run(fw, dev, queue, "Forward", x, n)
        e = np.zeros(n, np.complex128); e[q] = n
        mx, _ = oracle.compare(y, e)
        assert mx <= REL_TOL                                                      # K3
        a = oracle.gen_input(n, 1, first_transform=1)
        b = oracle.gen_input(n, 1, first_transform=2)
        ya, _, _ = _run(fw, dev, queue, "Forward", a, n)
        yb, _, _ = _run(fw, dev, queue, "Forward", b, n)
        yab, _, _ = _run(fw, dev, queue, "Forward", (a + 2 * b).astype(np.complex64), n)
        mx, _ = oracle.compare(yab, ya.astype(np.complex128) + 2 * yb.astype(np.complex128))
        assert mx <= REL_TOL                                                      # linearity
        ea = np.sum(np.abs(a.astype(np.complex128)) ** 2)
        eya = np.sum(np.abs(ya.astype(np.complex128)) ** 2) / n
        assert abs(ea - eya) <= 1e-5 * ea                                         # K7 Parseval


def test_onlyinverse_plus_normalize_equals_inverse(gpu, oracle):
    fw, dev, queue = gpu
    # one size per kernel family and plan regime, odd and even log2 n (the (a, b) rule of processor.rs:433-439)
    for n, batch in ((8, 4000), (16, 1000), (512, 40), (1 << 13, 9), (1 << 17, 20), (1 << 19, 1), (1 << 19, 5), (1 << 20, 2),
                     (1 << 20, 6), (1 << 21, 3), (1 << 24, 1)):
        x = oracle.gen_input(n, batch)
        src = upload(dev, queue, x)
        src2 = dev.create_buffer(x.nbytes)
        oi = fw.Onlyinverse(dev, queue, src, src2, n)
        nm = fw.Normalize(dev, queue, src, src2, n)
        enc = dev.create_command_encoder()
        oi.proc(enc)
        out = nm.proc(enc)
        y2 = out.map_read(stream=enc)
        y1, _, _ = _run(fw, dev, queue, "Inverse", x, n)
        assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))             # K6, bit for bit


@pytest.mark.parametrize("batch", [1, 3, 4, 15, 16, 17, 61, 4099])
def test_n512_the_references_own_length_at_ragged_batches(gpu, oracle, batch):
    """n = 512, the reference's own length (examples/basic.rs:32,66), through k_small32<9> (16 threads per transform, 16
    transforms per workgroup), all three transforming plans, against the fp64 DFT; batches that leave a wave (4 transforms),
    a workgroup (16) and the last workgroup ragged; the result lands in the second buffer (odd log2 n, processor.rs:153-157)."""
    fw, dev, queue = gpu
    n = 512
    x = oracle.gen_input(n, batch, first_transform=batch)
    for kind, direction in (("Forward", -1), ("Inverse", 1), ("Onlyinverse", 1)):
        r = oracle.dft_f64(x, n, direction)
        if kind == "Inverse":
            r = r / n
        y, which, facts = _run(fw, dev, queue, kind, x, n)
        assert which == 1 and facts["path"] == 0 and facts["launches_per_exec"] == 1
        _check(y, r, n)


# ---- the workgroup -> chunk map of the one-launch kernels on RAGGED grids ----
# one_launch_block() (csrc/device_common.h) maps the largest prefix of the grid that is whole runs of 64 workgroups per XCD
# (a multiple of 512 blocks) and leaves the remainder on the plain map.  Every other parity case has fewer than 512 blocks
# (map inactive) or an exact multiple of 512 (no remainder): these grids have 513 .. 1023 blocks, i.e. a mapped prefix, a
# plain-map tail AND a partial last chunk at once.  Every transform is checked: a chunk visited twice or not at all shows.
@pytest.mark.parametrize("n,batch,blocks", [
    (2, 700 * 4096 + 5, 701),       # k_chunk, 8192 samples per workgroup
    (64, 700 * 128 + 3, 701),       # k_chunk, radix 16 x 4
    (256, 33 * 513 + 7, 530),       # k_chunk at its largest length (32 transforms per workgroup)
    (512, 16 * 700 + 5, 701),       # k_small32<9>: 16 transforms per workgroup
    (1024, 8 * 600 + 3, 601),       # k_small32<10>: 8
    (4096, 2 * 650 + 1, 651),       # k_small32<12>: 2
    (8192, 700, 700),               # k_small32<13>: one transform per workgroup (ragged grid, whole chunks)
    (16384, 600, 600),              # k_small32<14>: 512 threads
    (32768, 520, 520),              # k_small32<15>: 1024 threads
])
def test_one_launch_block_map_on_ragged_grids(gpu, oracle, n, batch, blocks):
    fw, dev, queue = gpu
    per_wg = 8192 // n if n <= 256 else max(1, 256 // (n // 32))      # transforms per workgroup (launch_chunk / small32_xpw)
    assert 512 < -(-batch // per_wg) == blocks < 1024
    x = oracle.gen_input(n, batch, first_transform=17)
    y, which, facts = _run(fw, dev, queue, "Forward", x, n)
    assert facts["path"] == 0 and facts["launches_per_exec"] == 1 and which == (n.bit_length() - 1) % 2
    _check(y, oracle.dft_f64(x, n, -1), n)      # every transform (up to 2.9 M here)


def test_normalize_and_calibration_copy_on_ragged_grids(gpu, oracle):
    """k_scale (Normalize, normalize.wgsl:9-12; and the in-place form of fwa_calib_copy) and k_copy on 701-block grids with a
    partial last chunk: bit-exact against the oracle's normalize / the input."""
    fw, dev, queue = gpu
    n, batch = 64, 700 * 128 + 3                     # 701 workgroups of 8192 samples, the last one holds 3 transforms
    x = oracle.gen_input(n, batch, first_transform=5)
    a = upload(dev, queue, x)
    b = dev.create_buffer(x.nbytes)
    enc = dev.create_command_encoder()
    out = fw.Normalize(dev, queue, a, b, n).proc(enc)        # log2 n even: reads buffer1, writes and returns buffer2
    assert out is b
    got = out.map_read(stream=enc)
    assert np.array_equal(got.view(np.uint32), oracle.normalize_ref(x, n).view(np.uint32))
    # out-of-place calibration copy of the same bytes: 700 whole 64-KiB chunks (k_copy: mapped prefix of 512 + plain tail of
    # 188) + 96 16-byte vectors (k_copy_tail)
    nbytes = x.nbytes
    assert nbytes // 65536 == 700 and nbytes % 65536 == 1536
    dst = dev.create_buffer(nbytes)
    dev.calib_copy(dst, a, nbytes, encoder=enc)
    assert np.array_equal(dst.map_read(stream=enc).view(np.uint32), x.view(np.uint32))
    # in place (dst == src): k_scale with scale 1 over 700 chunks + a partial one
    dev.calib_copy(a, a, nbytes, encoder=enc)
    assert np.array_equal(a.map_read(stream=enc).view(np.uint32), x.view(np.uint32))


def test_calibration_copy_is_a_copy(gpu, oracle):
    """fwa_calib_copy (the measured-ceiling kernel of bench.py): chunked body + 16-byte tail, byte-exact."""
    fw, dev, queue = gpu
    count = (3 * 65536 + 4096 + 16) // 8          # three full 64-KiB chunks, a partial one and one last vector
    x = oracle.gen_input(count, 1, first_transform=9)
    a = upload(dev, queue, x)
    b = dev.create_buffer(x.nbytes)
    dev.calib_copy(b, a, x.nbytes)
    dev.poll()
    assert np.array_equal(b.map_read().view(np.uint32), x.view(np.uint32))


def test_device_generator_is_bit_identical_to_oracle(gpu, oracle):
    fw, dev, queue = gpu
    n, batch = 4096, 9
    buf = dev.create_buffer(n * batch * 8)
    dev.fill_synthetic(buf, n, first_transform=3, scale=2.0 ** -7)
    dev.poll()
    got = buf.map_read()
    want = oracle.gen_input(n, batch, first_transform=3, scale=2.0 ** -7)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- C3: the headline shape, full size, 64-bit offsets ----
def test_config_c3_full_size_sampled(gpu, oracle):
    fw, dev, queue = gpu
    n, batch = 1 << 20, 4096
    info = dev.info()
    if info["hbm_bytes"] < 48 * 2 ** 30:
        pytest.skip("needs a 32 GiB buffer")
    buf = dev.create_buffer(n * batch * 8)            # 32 GiB, element offsets exceed 2^32
    enc = dev.create_command_encoder()
    dev.fill_synthetic(buf, n, encoder=enc)
    plan = fw.Forward(dev, queue, buf, n)
    out = plan.proc(enc)
    enc.synchronize()
    assert out is buf and plan.get("path") == 1
    rng = np.random.default_rng(7)
    sample = [0, batch - 1] + sorted(rng.choice(np.arange(1, batch - 1), 14, replace=False).tolist())
    worst = 0.0
    for t in sample:
        y = out.map_read(offset=t * n * 8, size=n * 8, stream=enc)
        x = oracle.gen_input(n, 1, first_transform=t)
        mx, l2 = oracle.compare(y, oracle.dft_f64(x, n, -1))
        assert mx <= REL_TOL and l2 <= REL_TOL, (t, mx, l2)
        worst = max(worst, mx)
    print("C3 sampled transforms %s worst max_rel %.3g" % (sample, worst))
    # size-independent property at full size: forward then scaled inverse restores the generator output
    inv = fw.Inverse(dev, queue, buf, n)
    out2 = inv.proc(enc)
    enc.synchronize()
    for t in (0, 2049, batch - 1):
        z = out2.map_read(offset=t * n * 8, size=n * 8, stream=enc)
        x = oracle.gen_input(n, 1, first_transform=t)
        mx, _ = oracle.compare(z, x.astype(np.complex128))
        assert mx <= REL_TOL


@pytest.mark.parametrize("lg", [9, 6, 12])
def test_one_launch_kernels_at_the_full_footprint_sampled(gpu, oracle, lg):
    """The one-launch kernels at C3's footprint (2^32 samples = 32 GiB: byte offsets beyond 2^32, half a million workgroups,
    the pair block map over the whole grid): n = 512 (2^23 transforms through k_small32<9>; the result
    lands in the plan's second buffer), k_chunk (64) and k_small32 with its look-ups ahead of the data (4096).  Sampled transforms -- the first, the last, some in between, one beyond every 4-GiB
    boundary -- against the fp64 DFT of the generator's output, then the scaled inverse restores the input at full size."""
    fw, dev, queue = gpu
    n, batch = 1 << lg, 1 << (32 - lg)
    if dev.info()["hbm_bytes"] < 80 * 2 ** 30:
        pytest.skip("needs 32 GiB buffers")
    buf = dev.create_buffer(n * batch * 8)
    enc = dev.create_command_encoder()
    dev.fill_synthetic(buf, n, encoder=enc)
    plan = fw.Forward(dev, queue, buf, n)
    out = plan.proc(enc)
    enc.synchronize()
    assert plan.get("path") == 0 and plan.get("launches_per_exec") == 1 and (out is buf) == (lg % 2 == 0)
    per_4g = (1 << 32) // (n * 8)                        # transforms per 4 GiB
    rng = np.random.default_rng(lg)
    sample = sorted({0, batch - 1, 1, batch // 2 + 3} | {k * per_4g + int(rng.integers(0, per_4g)) for k in range(8)})
    for t in sample:
        y = out.map_read(offset=t * n * 8, size=n * 8, stream=enc)
        x = oracle.gen_input(n, 1, first_transform=t)
        mx, l2 = oracle.compare(y, oracle.dft_f64(x, n, -1))
        assert mx <= REL_TOL and l2 <= REL_TOL, (lg, t, mx, l2)
    inv = fw.Inverse(dev, queue, out, n)
    back = inv.proc(enc)
    enc.synchronize()
    for t in (sample[0], sample[len(sample) // 2], sample[-1]):
        z = back.map_read(offset=t * n * 8, size=n * 8, stream=enc)
        x = oracle.gen_input(n, 1, first_transform=t)
        mx, _ = oracle.compare(z, x.astype(np.complex128))
        assert mx <= REL_TOL, (lg, t, mx)
    inv.destroy()
    plan.destroy()
    buf.destroy()


# ---- the reference's benchmark loop, pipelined over two streams with pinned staging ----
@pytest.mark.parametrize("slots", [2, 3])
def test_host_transfer_pipeline_matches_oracle(gpu, oracle, slots):
    """examples/basic.rs:72-127 (write_buffer -> proc -> copy_buffer_to_buffer -> read back, every iteration) through
    fft_wgpu_amd.HostPipeline: upload of iteration i+1, transform of i and read-back of i-1 overlap.  Every iteration
    gets different data and EVERY read-back sample is compared with the oracle."""
    fw, dev, queue = gpu
    n, batch = 512, 2500                                   # the reference's own benchmark shape (basic.rs:32,66)
    count = n * batch
    pipe = fw.HostPipeline(dev, queue, lambda d, q, b: fw.Forward(d, q, b, n), count, slots=slots)
    iters = 7
    inputs = [oracle.gen_input(n, batch, first_transform=1000 * it) for it in range(iters)]
    results = {}
    pending = []
    for it in range(iters):
        s = pipe.submit(inputs[it])
        pending.append((it, s))
        if len(pending) == slots:                          # read a slot back before it is reused
            j, sj = pending.pop(0)
            results[j] = pipe.result(sj).copy()
    for j, sj in pending:
        results[j] = pipe.result(sj).copy()
    pipe.drain()
    for it in range(iters):
        r = oracle.dft_f64(inputs[it], n, -1)
        _check(results[it], r, n)
    # the serial form of the same loop (the reference's literal call order, default-stream read-back) agrees bit for bit
    src = dev.create_buffer(count * 8)
    staging = dev.create_buffer(count * 8)
    plan = fw.Forward(dev, queue, src, n)
    queue.write_buffer(src, 0, inputs[3])
    enc = dev.create_command_encoder()
    out = plan.proc(enc)
    enc.copy_buffer_to_buffer(out, 0, staging, 0, count * 8)
    queue.submit(enc.finish())
    ans = staging.map_read()                                # no stream given: device.poll(wait) semantics
    assert np.array_equal(ans.view(np.uint32), results[3].view(np.uint32))


def test_plan_cache_shares_tables_and_rings(gpu):
    """Second plan of a length on the same context: no table build, no upload; a destroyed plan's ring is reused
    (examples/basic_inverse2.rs creates two plans per size)."""
    fw, dev, queue = gpu
    n = 1 << 20
    buf = dev.create_buffer(n * 8 * 8)
    buf2 = dev.create_buffer(n * 8 * 8)
    before = dev.stats()
    p1 = fw.Forward(dev, queue, buf, n)
    mid = dev.stats()
    p2 = fw.Inverse(dev, queue, buf2, n)                    # tables hold forward twiddles; the inverse conjugates on use
    after = dev.stats()
    assert mid["table_builds"] - before["table_builds"] <= 1
    assert after["table_builds"] == mid["table_builds"] and after["table_cache_hits"] == mid["table_cache_hits"] + 1
    assert p2.get("tables_shared") >= 2                     # the cache and p1
    first_us, second_us = mid["last_plan_create_us"], after["last_plan_create_us"]
    print("plan create 2^20: first %d us, second (cached tables) %d us" % (first_us, second_us))
    p1.destroy()
    p3 = fw.Forward(dev, queue, buf, n)
    end = dev.stats()
    assert end["ring_reuses"] == after["ring_reuses"] + 1 and end["ring_allocs"] == after["ring_allocs"]
    print("plan create 2^20 with cached tables and pooled ring: %d us" % end["last_plan_create_us"])
    p2.destroy(); p3.destroy()


# ---- error behaviour of the boundary ----
def test_rejects_bad_arguments(gpu):
    fw, dev, queue = gpu
    buf = dev.create_buffer(8 * 1000)
    with pytest.raises(fw.FwaError) as e:
        fw.Forward(dev, queue, buf, 1000)            # not a power of two
    assert e.value.status == 1
    with pytest.raises(fw.FwaError):
        fw.Forward(dev, queue, buf, 16)              # 1000 % 16 != 0
    with pytest.raises(fw.FwaError):
        fw.Forward(dev, queue, buf, 0)
    ok = dev.create_buffer(8 * 1024)
    small = dev.create_buffer(8 * 512)
    with pytest.raises(fw.FwaError):
        fw.Onlyinverse(dev, queue, ok, small, 512)   # size mismatch
    with pytest.raises(fw.FwaError):
        fw.Onlyinverse(dev, queue, ok, ok, 512)      # same buffer twice
    empty = dev.create_buffer(0)
    p = fw.Forward(dev, queue, empty, 1024)           # empty batch is legal and a no-op
    assert p.get("batch") == 0
    enc = dev.create_command_encoder()
    assert p.proc(enc) is empty
    for n in (1, 2, 16, 4096, 1 << 15, 1 << 16, 1 << 19, 1 << 20, 1 << 21, 1 << 24, 1 << 30):   # every plan family, empty
        for mk in (fw.Forward, fw.Inverse):
            q = mk(dev, queue, empty, n)
            assert q.get("batch") == 0
            q.proc(enc)
            for key, val in (("group", 4), ("streams", 2)):
                if q.get("path") in (1, 7):
                    q2 = mk(dev, queue, empty, n)
                    q2.set(key, val)
                    q2.proc(enc)
    enc.synchronize()
    with pytest.raises(fw.FwaError):
        fw.Forward(dev, queue, empty, 1 << 31)       # above 2^30


def test_product_library_rejects_laboratory_settings(gpu):
    """The product library ships one kernel per (size class, pass, direction): the laboratory paths and variants answer
    FWA_ERR_UNSUPPORTED (6) and leave the plan as it was."""
    fw, dev, queue = gpu
    assert not dev.lab
    buf = dev.create_buffer(8 << 20 << 3)      # 2^20 x 8
    p = fw.Forward(dev, queue, buf, 1 << 20)
    for key, val in (("path", 5), ("tile_w", 32), ("depth", 4), ("ring_slots", 6), ("wgs", 512), ("ring_rotate", 2),
                     ("inject_launch_failure", 0)):
        with pytest.raises(fw.FwaError) as e:
            p.set(key, val)
        assert e.value.status == 6, (key, e.value.status)
    with pytest.raises(fw.FwaError) as e:
        p.set("max_teams", 2)                   # a key of the team path, which left the tree in round 6
    assert e.value.status == 1
    assert p.get("path") == 1 and p.get("tile_w") == 16
    p.set("tile_w", 16)
    small = fw.Forward(dev, queue, dev.wrap_buffer(buf.device_ptr, 8 * 4096), 64)
    for val in (2, 3):
        with pytest.raises(fw.FwaError) as e:
            small.set("small_reg", val)
        assert e.value.status == 6
    small.set("small_reg", 1)
    mid = fw.Forward(dev, queue, dev.wrap_buffer(buf.device_ptr, 8 << 16 << 5), 1 << 16)
    with pytest.raises(fw.FwaError) as e:
        mid.set("path", 8)                      # no such path any more (it was the team path)
    assert e.value.status == 6 and mid.get("path") == 7


def test_failed_retune_leaves_the_plan_as_it_was(gpu, oracle):
    """a re-factorisation that cannot get its ring (device memory exhausted) must leave path, factors,
    TABLES and results exactly as they were -- the tables of the new factorisation are handed to the plan only after its
    pipeline has been built (before, the plan kept the old factors with the new tables)."""
    fw, dev, queue = gpu
    n, batch = 1 << 18, 53   # one group of 53 transforms: a 106-MiB ring, a size no earlier test has left in the ring pool
    x = oracle.gen_input(n, batch, first_transform=3)
    src = dev.create_buffer(x.nbytes)
    plan = fw.Forward(dev, queue, src, n)
    f0, path0, shared0 = plan.get("factors"), plan.get("path"), plan.get("tables_shared")
    assert path0 == 7 and f0 == 8 | (10 << 8)
    hog = []
    try:
        # exhaust the device memory down to fragments below 64 MiB (hipMemGetInfo is too coarse to stop at a byte count):
        # the 106-MiB ring of the re-factorised plan cannot be allocated, its few KiB of tables can
        for chunk in (64 << 30, 8 << 30, 1 << 30, 128 << 20, 64 << 20):
            while True:
                try:
                    hog.append(dev.create_buffer(chunk))
                except fw.FwaError as oom:
                    assert oom.status == 2
                    break
        with pytest.raises(fw.FwaError) as e:
            plan.set("factors", 9 | (9 << 8))
        assert e.value.status == 2, e.value.status      # FWA_ERR_OUT_OF_MEMORY
    finally:
        for h in hog:
            h.destroy()
    assert (plan.get("factors"), plan.get("path"), plan.get("tables_shared")) == (f0, path0, shared0)
    queue.write_buffer(src, 0, x)
    enc = dev.create_command_encoder()
    y = plan.proc(enc).map_read(stream=enc)
    r = oracle.dft_f64(x, n, -1)
    for t in (0, 1, 31, 52):
        mx, l2 = oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n])
        assert mx <= REL_TOL and l2 <= REL_TOL, (t, mx, l2)


@pytest.mark.parametrize("example", ["example_basic_inverse2", "example_basic_inverse"])
def test_cpp_mirror_replays_reference_example(gpu, tmp_path, example):
    """include/fft_wgpu.hpp: C++ replays of the reference's two asserting tests -- examples/basic_inverse2.rs (Onlyinverse +
    Normalize) and examples/basic_inverse.rs (Inverse, result in the plan's second buffer, copied to staging): n = 512,
    constant input, max error < 1e-5 -- through the C ABI."""
    import subprocess
    from conftest import ROOT
    exe = tmp_path / "example"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", example + ".cpp"),
                           "-L" + os.path.join(ROOT, "fft_wgpu_amd"), "-lfft_wgpu_amd", "-pthread", "-o", str(exe)])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "fft_wgpu_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "max error 0" in r.stdout


def test_cpp_host_pipeline_replays_reference_benchmark_loop(gpu, tmp_path):
    """include/fft_wgpu.hpp::HostPipeline, the C++ twin of fft_wgpu_amd.HostPipeline: the reference's benchmark loop
    (examples/basic.rs:72-127, n = 512 x 2500, upload + proc + copy + read-back every iteration) with pinned staging, two
    streams and host-guarded slot reuse, EVERY read-back sample checked against the analytic DFT of its impulse input."""
    import re
    import subprocess
    from conftest import ROOT
    exe = tmp_path / "example_basic_pipeline"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_basic_pipeline.cpp"),
                           "-L" + os.path.join(ROOT, "fft_wgpu_amd"), "-lfft_wgpu_amd", "-pthread", "-o", str(exe)])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "fft_wgpu_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe), "200", "3"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    print(r.stdout)
    m = re.search(r"samples checked (\d+) max abs error ([0-9.e+-]+)", r.stdout)
    assert m and int(m.group(1)) == 200 * 512 * 2500 and float(m.group(2)) <= REF_ABS_TOL
    rate = float(re.search(r"pipeline only: [0-9.]+ iterations/s, ([0-9.]+) GB/s each way", r.stdout).group(1))
    link = float(re.search(r"link only \(both directions busy, no transform\): ([0-9.]+) GB/s each way", r.stdout).group(1))
    # judged against the link rate the SAME child measures right after the pipeline (same
    # transfer size, both directions busy, no transform) -- standalone 43.5 of 47-48 GB/s each way
    # (profiles/round3/host_pipeline_cpp.txt); a child of this pytest process sees less of both, in the same proportion
    assert rate >= 0.8 * link and link >= 10.0, r.stdout


def test_plan_owned_result_buffer_outlives_temporary_plan(gpu, oracle):
    """Forward/Inverse with odd log2 n return a view of the plan's own second buffer (processor.rs:13,153-157);
    the view must keep the plan alive, as the Rust borrow does."""
    import gc
    fw, dev, queue = gpu
    x = oracle.gen_input(512, 4)
    src = upload(dev, queue, x)
    enc = dev.create_command_encoder()
    out = fw.Forward(dev, queue, src, 512).proc(enc)   # the plan object is a temporary
    gc.collect()
    y = out.map_read(stream=enc)
    _check(y, oracle.dft_f64(x, 512, -1), 512)


@pytest.mark.parametrize("lg,p1_gen", [(27, 1), (28, 1), (28, 10), (29, 1), (29, 0), (30, 1)])
def test_large_single_transform_properties(gpu, lg, p1_gen):
    """n = 2^27 .. 2^30 (1 - 8 GiB per transform, three passes, 64-bit offsets inside ONE transform; from 2^29 a tile
    spans >= 4 GiB: k_p1_gen addresses a transform through four descriptors, k_tile (p1_gen = 0 for pass A, always for
    the later passes) runs in its 64-bit-pointer form, BUF = false): no CPU FFT of that size in seconds, so
    size-independent properties instead -- an impulse at p transforms to exp(-2*pi*i*p*k/n) (every output checked, in
    chunks), and forward followed by the scaled inverse restores the input to <= 1e-5."""
    fw, dev, queue = gpu
    n = 1 << lg
    if dev.info()["hbm_bytes"] < 4 * n * 8 + (8 << 30):
        pytest.skip("needs ~4 buffers of the transform size in device memory")
    p = 3 * 5 * 7 * 11 * 13 + 2 ** 20
    src = dev.create_buffer(n * 8)
    zeros = np.zeros(1 << 24, dtype=np.complex64)
    for off in range(0, n, 1 << 24):                      # zero-fill in 128-MiB pieces (keeps host memory small)
        queue.write_buffer(src, off * 8, zeros)
    queue.write_buffer(src, p * 8, np.ones(1, dtype=np.complex64))
    plan = fw.Forward(dev, queue, src, n)
    if p1_gen == 10:  # the 1024-point first pass (k_p1_gen) at a size whose default is the 512 x 32 tile of k_colsw
        plan.set("factors", 10 | (9 << 8) | (9 << 16))
        p1_gen = 1
    plan.set("p1_gen", p1_gen)
    first = plan.get("factors") & 255
    assert plan.get("path") == 7 and plan.get("factors") >> 16 != 0
    assert (first, plan.get("colsw")) == ((9, 1) if lg <= 28 and first != 10 else (10, 0 if lg > 28 else plan.get("colsw")))
    enc = dev.create_command_encoder()
    out = plan.proc(enc)
    enc.synchronize()
    assert (out.device_ptr == src.device_ptr) == (lg % 2 == 0)
    chunk = 1 << 24
    worst = 0.0
    for off in range(0, n, chunk):
        y = out.map_read(offset=off * 8, size=chunk * 8, stream=enc)
        k = np.arange(off, off + chunk, dtype=np.int64)
        ph = ((p * k) % n).astype(np.float64) * (-2.0 * np.pi / n)
        worst = max(worst, np.abs(y.real - np.cos(ph)).max(), np.abs(y.imag - np.sin(ph)).max())
    assert worst <= REL_TOL, worst
    inv = fw.Inverse(dev, queue, out, n)
    back = inv.proc(enc)
    enc.synchronize()
    worst = 0.0
    for off in range(0, n, chunk):
        z = back.map_read(offset=off * 8, size=chunk * 8, stream=enc)
        if off <= p < off + chunk:
            z[p - off] -= 1
        worst = max(worst, np.abs(z).max())
    assert worst <= REL_TOL, worst


def test_seeded_fuzz_over_sizes_kinds_and_batches(gpu, oracle):
    """60 seeded random (n, batch, plan kind) combinations, ragged batches included, against the fp64 DFT."""
    fw, dev, queue = gpu
    rng = np.random.default_rng(20251004)
    for case in range(60):
        lg = int(rng.integers(0, 19))
        n = 1 << lg
        batch = int(rng.integers(1, max(2, min(3000, (1 << 21) >> lg) + 1)))
        kind = ("Forward", "Inverse", "Onlyinverse")[int(rng.integers(0, 3))]
        x = oracle.gen_input(n, batch, first_transform=case)
        y, which, _ = _run(fw, dev, queue, kind, x, n)
        assert which == lg % 2, (case, lg, batch, kind)
        r = oracle.dft_f64(x, n, -1 if kind == "Forward" else +1)
        if kind == "Inverse":
            r = r / n
        for t in (0, batch // 2, batch - 1):
            mx, l2 = oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n])
            assert mx <= REL_TOL and l2 <= REL_TOL, (case, lg, batch, kind, t, mx, l2)


def test_seeded_fuzz_multipass_sizes_kinds_and_batches(gpu, oracle):
    """30 seeded random (n = 2^16 .. 2^23, batch, kind) combinations on the default plans: both regimes (small balanced
    tiles for few transforms, 1024-point first pass + 32-point rows otherwise), ragged groups, every kind, against the
    fp64 DFT (all transforms)."""
    fw, dev, queue = gpu
    rng = np.random.default_rng(20261004)
    seen = set()
    for case in range(30):
        lg = int(rng.integers(16, 24))
        n = 1 << lg
        batch = int(rng.integers(1, max(2, (1 << 25) >> lg) + 1))
        kind = ("Forward", "Inverse", "Onlyinverse")[int(rng.integers(0, 3))]
        x = oracle.gen_input(n, batch, first_transform=1000 + case)
        y, which, facts = _run(fw, dev, queue, kind, x, n)
        seen.add((facts["path"], facts["factors"]))
        assert which == lg % 2, (case, lg, batch, kind)
        r = oracle.dft_f64(x, n, -1 if kind == "Forward" else +1)
        if kind == "Inverse":
            r = r / n
        for t in range(batch):
            mx, l2 = oracle.compare(y[t * n:(t + 1) * n], r[t * n:(t + 1) * n])
            assert mx <= REL_TOL and l2 <= REL_TOL, (case, lg, batch, kind, t, mx, l2)
    assert len(seen) >= 8, seen   # the draw reaches both regimes of several sizes


def test_two_contexts_interleaved_and_from_two_threads(gpu, oracle):
    """Two contexts on the device (the C ABI's unit of isolation: own twiddle cache, ring pool, streams), used
    interleaved from one thread and then concurrently from two host threads (one context each: the header's rule for
    threads).  Each context's results must be those of a fresh single context."""
    import threading
    fw, dev, queue = gpu
    _, dev2, queue2 = open_gpu()
    cases = [(1 << 12, 37, "Forward"), (1 << 20, 5, "Forward"), (1 << 17, 40, "Inverse"), (256, 1000, "Forward")]
    want = {}
    for n, batch, kind in cases:
        x = oracle.gen_input(n, batch, first_transform=n % 97)
        y, _, _ = _run(fw, dev, queue, kind, x, n)
        want[(n, batch, kind)] = (x, y)
    # interleaved: plan on ctx 2, plan on ctx 1, exec on 2, exec on 1
    for n, batch, kind in cases:
        x, y = want[(n, batch, kind)]
        b2 = upload(dev2, queue2, x)
        b1 = upload(dev, queue, x)
        mk = {"Forward": fw.Forward, "Inverse": fw.Inverse}[kind]
        p2, p1 = mk(dev2, queue2, b2, n), mk(dev, queue, b1, n)
        e2, e1 = dev2.create_command_encoder(), dev.create_command_encoder()
        o2 = p2.proc(e2)
        o1 = p1.proc(e1)
        assert np.array_equal(o2.map_read(stream=e2).view(np.uint32), y.view(np.uint32))
        assert np.array_equal(o1.map_read(stream=e1).view(np.uint32), y.view(np.uint32))
    assert dev2.stats()["table_builds"] >= 3 and dev2.stats()["table_cache_hits"] == 0   # its own cache
    # two threads, one context each, 20 rounds over the cases
    errors = []

    def worker(d, q):
        try:
            for rnd in range(20):
                n, batch, kind = cases[rnd % len(cases)]
                x, y = want[(n, batch, kind)]
                got, _, _ = _run(fw, d, q, kind, x, n)
                if not np.array_equal(got.view(np.uint32), y.view(np.uint32)):
                    errors.append((rnd, n, batch, kind))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(dev, queue)), threading.Thread(target=worker, args=(dev2, queue2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:4]


@pytest.mark.parametrize("n,batch", [(512, 2500), (1 << 20, 40), (1 << 18, 70), (1 << 22, 3)])
def test_exec_captures_into_a_hip_graph(gpu, oracle, n, batch):
    """fwa_plan_exec is stream-ordered and allocates nothing, so a caller can capture it into a hipGraph (a HIP stream
    of the caller's, wrapped with fwa_stream_wrap, captured in hipStreamCaptureModeGlobal).  Replaying the graph on fresh
    input gives the bits of a direct exec.  All four shapes resolve to ONE chain (fewer than 4 groups: default_chains), so
    their groups run on the caller's stream and nothing forks; the plans that fork to the chain streams and join back with
    events are captured in tests/test_gpu_ordering.py (graph_forked/*)."""
    fw, dev, queue = gpu
    hip = hip_runtime()
    x = oracle.gen_input(n, batch, first_transform=n % 89)
    ref, _, _ = _run(fw, dev, queue, "Forward", x, n)
    src = upload(dev, queue, x)
    plan = fw.Forward(dev, queue, src, n)
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0          # hipStreamNonBlocking
    enc = dev.create_command_encoder(hip_stream=stream)
    plan.proc(enc)                                                              # first-use work outside the capture
    enc.synchronize()
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0                            # hipStreamCaptureModeGlobal
    out = plan.proc(enc)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    for rep in range(2):
        queue.write_buffer(src, 0, x, encoder=enc)
        assert hip.hipGraphLaunch(gexec, stream) == 0
        y = out.map_read(stream=enc)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), (n, batch, rep)
    assert hip.hipGraphExecDestroy(gexec) == 0 and hip.hipGraphDestroy(graph) == 0
    del enc
    assert hip.hipStreamDestroy(stream) == 0


def test_plan_churn_does_not_leak_device_memory(gpu, oracle):
    """300 plans of random sizes and kinds created, run and destroyed (buffers too): afterwards the device has its memory
    back, up to what the context keeps on purpose -- the ring pool (<= 1 GiB, reported) and the twiddle tables of the
    lengths seen (a few MiB)."""
    fw, dev, queue = gpu
    rng = np.random.default_rng(7)
    enc = dev.create_command_encoder()
    dev.poll()
    before = dev.stats()
    for i in range(300):
        lg = int(rng.integers(1, 25))
        n = 1 << lg
        batch = int(rng.integers(1, max(2, (1 << 25) >> lg) + 1))
        kind = ("Forward", "Inverse", "Onlyinverse", "Normalize")[int(rng.integers(0, 4))]
        src = dev.create_buffer(n * batch * 8)
        src2 = dev.create_buffer(n * batch * 8) if kind in fw.SECOND_BUFFER_KINDS else None
        plan = fw.plan_of_kind(kind, dev, queue, src, src2, n)
        dev.fill_synthetic(src, n, scale=1e-3, encoder=enc)
        plan.proc(enc)
        enc.synchronize()
        plan.destroy()
        src.destroy()
        if src2 is not None:
            src2.destroy()
    dev.poll()
    after = dev.stats()
    kept = before["mem_free_bytes"] - after["mem_free_bytes"]
    assert after["pooled_ring_bytes"] <= 1 << 30
    assert kept <= after["pooled_ring_bytes"] - before["pooled_ring_bytes"] + (256 << 20), (kept, after)
