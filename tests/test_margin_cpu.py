"""The margin checks on the CPU: the host threshold function (csrc/smp_paths.cpp: margin_threshold) through a stand-alone
ASAN / UBSAN driver, and the conditions test_gpu_margin.py rests on, asserted on the restatement alone
(margin_restatement.py: the CPU oracle's validity and clearance_restatement.py's clearances)."""
import os
import subprocess

import numpy as np
import pytest

import clearance_restatement as C
import margin_restatement as G
import repair_restatement as P
import shortcut_restatement as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")


# ------------------------------------------------------------------------------------------ host threshold
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("margin") / "margin_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "margin_table.cpp"), os.path.join(CSRC, "smp_paths.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_threshold(table, orobot):
    """S is the largest double with fl(fl(sqrt(S)) - r) <= m: it satisfies the property, the next double does not."""
    radii = sorted(set(float(r) for r in orobot.sph_r[:orobot.n_sph])) + [0.0]  # (0: a primitive)
    margins = [1e-3, 2e-3, 5e-3, 0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.3, 0.5]
    cases = [(r, m) for r in radii for m in margins]
    text = "".join("%s %s\n" % (r.hex(), float(m).hex()) for r, m in cases)
    p = subprocess.run([table], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    for (r, m), line in zip(cases, lines):
        S, d, du = (float.fromhex(t) for t in line.split())
        up = np.nextafter(S, np.inf)
        # numpy's sqrt is correctly rounded too: the same two values, formed again here
        assert float(np.sqrt(S)) - r == d and float(np.sqrt(up)) - r == du, (r, m)
        assert d <= m < du, (r, m, S, d, du)
        assert abs(S - (r + m) ** 2) <= 1e-12, (r, m, S)


# ------------------------------------------------------------------------------------------ non-vacuity
@pytest.mark.parametrize("name,n_valid,n_wide,n_both", [("c2", 31, 18, 10), ("room3", 34, 18, 12)])
def test_poses_hold_every_answer(name, n_valid, n_wide, n_both):
    valid = R.oracle_for(name).check_configs(C.poses(name)).astype(bool)
    assert valid.sum() == n_valid
    wide, both = G.poses_expected(name, 0.1, 0.0).astype(bool), G.poses_expected(name, 0.05, 0.03).astype(bool)
    assert wide.sum() == n_wide and both.sum() == n_both
    assert not (wide & ~valid).any() and not (both & ~valid).any()
    # each flag alone and the disabled link change the answer somewhere, so those GPU cases are not the full check again
    for mm, ms in G.POSE_MARGINS:
        full = G.poses_expected(name, mm, ms)
        assert 0 < full.sum() < len(full)
    assert (G.poses_expected(name, 0.05, 0.03, True, False) != both).any()
    assert (G.poses_expected(name, 0.05, 0.03, False, True) != both).any()


@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("mm,ms", G.EDGE_MARGINS)
def test_edges_hold_every_answer(name, mm, ms):
    plain = G.edges_plain(name)
    first, M = G.edges_expected(name, mm, ms)
    assert (first != plain).sum() >= 4
    assert (first < 0).any()
    assert (first > R.CT - 1).any()  # a first unclear point in a second tile
    assert ((first >= 0) | (plain < 0)).all()  # an edge that is not free is not clear
    assert ((plain < 0) | (first <= plain)).all()
    if (name, mm, ms) == ("c2", 0.0, 0.02):
        assert first[7] == 199


def test_pipeline():
    """The 12-waypoint C2 path at a map margin of 2 cm: the shortcut alone is blocked, the repair closes both gaps in
    round 0, the shortcut of the repaired rows stays more than 2 cm clear and costs more than the plain one."""
    alone, rep = G.pipeline_alone(), G.pipeline_repair()
    cut, cut_plain = G.pipeline_shortcut(), G.pipeline_shortcut(False)
    assert alone["path"] is None and alone["first_blocked"] == 3
    assert (alone["first"][[i == j - 1 for i, j in alone["pairs"]]] >= 0).sum() == 4
    assert rep["status"] == P.OK and rep["n_gaps"] == 2
    assert [g[:2] for g in rep["gaps"]] == [[3, 5], [7, 9]] and rep["closed_round"] == [0, 0]
    assert rep["n_items"] == 128 and rep["n_free"] == 6 and len(rep["path"]) == 26
    assert round(rep["cost_in"], 3) == 10.817 and round(rep["cost_out"], 3) == 11.538
    assert cut["n_edges"] == 325 and cut["n_valid"] == 119 and cut_plain["n_valid"] == 124
    assert round(cut["cost_out"], 4) == 9.7746 and round(cut_plain["cost_out"], 4) == 9.7455
    # every dense point of the final route is more than 2 cm clear
    w = cut["path"]
    e = C.edge_clearance("c2", w[:-1], w[1:], 0.3, with_self=False)
    assert e["map"].min() > G.PIPE_MARGIN[0]


def test_unclear_start():
    rep = G.repair(C.path12(), 0.05, 0.0)
    assert rep["status"] == P.ERR_START_INVALID


def test_no_solution():
    rep = G.repair(C.path12(), 0.03, 0.02, samples=64, rounds=4)
    assert rep["status"] == P.ERR_NO_SOLUTION and rep["first_blocked"] == 0
    assert [g[:2] for g in rep["gaps"]] == [[0, 11]] and rep["n_items"] == 256 and rep["n_free"] == 0


def test_detours_differ():
    """The detour cases of the GPU test: at (0.02, 0) the two free items of the plain call stay free; at (0.02, 0.02)
    the margin takes one of them away."""
    plain = P.detour_expected("a_blocked_gap")
    d = G.detours_expected()
    assert np.array_equal(d["v"], plain["v"]) and np.array_equal(d["M1"], plain["M1"])
    assert plain["free"].sum() == 2 and d["free"].sum() == 2
    assert G.detours_expected("a_blocked_gap", 0.02, 0.02)["free"].sum() == 1


def test_valid_is_positive_clearance():
    """Condition 1 of the definition is implied by 2 and 3 on these inputs: valid == (map > 0 and self > 0)."""
    for name in G.SCENES:
        q = C.poses(name)
        c = C.clearance(name, q, 0.05)
        valid = R.oracle_for(name).check_configs(q).astype(bool)
        assert np.array_equal(valid, (c["map"] > 0) & (c["self"] > 0))
