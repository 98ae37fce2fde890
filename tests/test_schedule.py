"""The host-side scheduling decisions (fft_wgpu_amd/csrc/schedule.h), pinned exhaustively without a device.

tools/schedule_table.cpp prints choose_path over every length and the batches around its thresholds, and for every factor
triple with entries 0 .. 13 of the lengths 2^12 .. 2^30 whether the key "factors" accepts it and what resolve_tiled picks
under each of the 16 settings of "colsw" / "rows32" / "p1_gen" / "tile_ring".  tests/golden/tiled_schedule.txt holds that
output as the hand-written logic before schedule.h existed produced it: a change to a kernel limit, a default or a pass
alternative shows up here as a diff of decisions, not as a launch failure or a silent switch of kernels on a GPU.
"""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiled_schedule.txt")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("schedule") / "schedule_table"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "fft_wgpu_amd", "csrc"),
                           os.path.join(ROOT, "tools", "schedule_table.cpp"), "-o", str(exe)])
    return str(exe)


def test_decision_table_matches_the_golden(tool):
    got = subprocess.run([tool], capture_output=True, text=True, check=True).stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    diff = ["line %d: golden %r, now %r" % (i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff and len(got) == len(want), "%d lines now, %d in the golden; first differences:\n%s" % (
        len(got), len(want), "\n".join(diff[:10]))


def test_golden_covers_the_domain():
    lines = open(GOLDEN).read().splitlines()
    assert os.path.getsize(GOLDEN) < 100_000
    assert sum(ln.startswith("D ") for ln in lines) == 31 * 9
    triples = [ln.split()[1:3] for ln in lines if ln.startswith("T ")]
    want = [(lg, a, b, lg - a - b) for lg in range(12, 31) for a in range(14) for b in range(14) if 0 <= lg - a - b <= 13]
    assert [(int(lg), *map(int, f.split(","))) for lg, f in triples] == want
    # every default factorisation of a tiled plan is one the "factors" key would accept
    valid = {tuple(ln.split()[1:3]) for ln in lines if ln.startswith("T ") and not ln.endswith(" invalid")}
    defaults = {(d[1], d[4]) for d in (ln.split() for ln in lines if ln.startswith("D ")) if d[3] == "7"}
    assert defaults and defaults <= valid, sorted(defaults - valid)


def test_chosen_kernels_lie_inside_the_families_set_up(tool):
    """families(lg, lf) is what setup_path prepares at plan creation / re-factorisation; no setting of the flag keys may
    reach a kernel outside it (its dynamic-LDS limit would never have been raised)."""
    out = subprocess.run([tool, "families"], capture_output=True, text=True, check=True).stdout.splitlines()
    valid = [ln.split()[1:3] for ln in open(GOLDEN).read().splitlines() if ln.startswith("T ") and not ln.endswith(" invalid")]
    assert [ln.split()[1:3] for ln in out] == valid and valid
    for ln in out:
        head, chosen = ln.split(" : ")
        fam = int(head.split()[3], 16)
        chosen = [int(c, 16) for c in chosen.split()]
        assert len(chosen) == 16 and all(c and not c & ~fam for c in chosen), ln
        assert fam == functools.reduce(int.__or__, chosen), ln   # and nothing unreachable is set up
