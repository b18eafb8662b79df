"""The far-goal stage on the CPU: the host logic (csrc/smp_route.cpp: the lattice fit, the route search, the handover)
through a stand-alone ASAN / UBSAN driver against lattice_restatement.py's heapq Dijkstra -- chain, rows, cost and status
bit for bit --, and the conditions test_gpu_lattice.py rests on, asserted on the restatement alone."""
import math
import os
import subprocess

import numpy as np
import pytest

import lattice_restatement as T
import shortcut_restatement as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")
hx = lambda v: float(v).hex()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "route_table.cpp"), os.path.join(CSRC, "smp_route.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(table, text):
    p = subprocess.run([table], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout.split()


# ------------------------------------------------------------------------------------------ the cases
def layer(rows):
    """A free map from text, one string per y (ascending), '.' free."""
    return np.array([[ch == "." for ch in r] for r in rows], bool)[None]


def grid_lattice(nx, ny, nt=1, wrap=0, pitch=0.25, dtheta=math.pi / 4):
    return T.Lattice(-1.0, 0.5, pitch, nx, ny, 0.1, dtheta, nt, wrap, T.ARM)


def at(lat, ix, iy, t=0):
    return tuple(T.node_config(lat, ix, iy, t)[:3])


def synthetic_cases():
    ring = grid_lattice(7, 7)
    blocked = ["#######"] * 7
    put = lambda cells: layer(["".join("." if (x, y) in cells else "#" for x in range(7)) for y in range(7)])
    c = {}
    one = grid_lattice(1, 1)
    c["one_node"] = (one, layer(["."]), at(one, 0, 0), at(one, 0, 0), 2)
    c["one_node_blocked"] = (one, layer(["#"]), at(one, 0, 0), at(one, 0, 0), 2)
    free7 = put({(x, y) for x in range(7) for y in range(7)})
    c["from_is_to"] = (ring, free7, at(ring, 2, 5), at(ring, 2, 5), 2)
    c["straight_and_diagonal"] = (ring, free7, at(ring, 0, 1), at(ring, 6, 4), 0)
    # rings about the blocked centre (3, 3); the goal (6, 6) is free
    c["ring1_least_distance"] = (ring, put({(4, 3), (2, 2), (6, 6), (5, 4), (6, 5), (5, 3)}), at(ring, 3, 3), at(ring, 6, 6), 2)
    c["ring1_tie_to_lower_node"] = (ring, put({(3, 2), (2, 3), (4, 3), (3, 4), (6, 6)}), at(ring, 3, 3), at(ring, 3, 4), 1)
    c["ring2"] = (ring, put({(5, 3), (1, 1), (6, 3), (6, 4), (6, 5), (6, 6)}), at(ring, 3, 3), at(ring, 6, 6), 2)
    c["ring2_out_of_reach"] = (ring, put({(5, 3), (1, 1), (6, 6)}), at(ring, 3, 3), at(ring, 6, 6), 1)
    c["blocked_start_no_snap"] = (ring, put({(4, 3), (6, 6)}), at(ring, 3, 3), at(ring, 6, 6), 0)
    c["blocked_goal_no_snap"] = (ring, put({(4, 3), (6, 6)}), at(ring, 4, 3), at(ring, 5, 6), 0)
    c["goal_snaps"] = (ring, put({(4, 3), (5, 3), (5, 4), (5, 5), (6, 6)}), at(ring, 4, 3), at(ring, 5, 6), 1)
    c["all_blocked"] = (ring, layer(blocked), at(ring, 3, 3), at(ring, 6, 6), 7)
    c["outside"] = (ring, free7, (-5.0, 0.5, 0.1), at(ring, 6, 6), 2)
    c["heading_outside"] = (ring, free7, at(ring, 1, 1), (0.0, 1.0, 2.0), 2)
    c["nan"] = (ring, free7, (float("nan"), 0.5, 0.1), at(ring, 6, 6), 2)
    # a diagonal forbidden by one occupied axis cell: (0, 0) -> (1, 1) goes round by (0, 1)
    two = grid_lattice(2, 2)
    c["diagonal_forbidden"] = (two, layer([".#", ".."]), at(two, 0, 0), at(two, 1, 1), 0)
    c["diagonal_allowed"] = (two, layer(["..", ".."]), at(two, 0, 0), at(two, 1, 1), 0)
    # eight headings at one place: 0 -> 7 is one step through the wrap, seven without it
    for wrap in (0, 1):
        turn = grid_lattice(1, 1, 8, wrap)
        c["turn_wrap%d" % wrap] = (turn, np.ones((8, 1, 1), bool), at(turn, 0, 0, 0), at(turn, 0, 0, 7), 0)
    spin = grid_lattice(3, 3, 8, 1)
    c["wrap_snaps_heading"] = (spin, np.ones((8, 3, 3), bool), at(spin, 0, 0, 1), (at(spin, 2, 2)[0], at(spin, 2, 2)[1],
                                                                                  0.1 - 3.0 * math.pi / 4), 0)
    # a wall in one layer with a door in another: the route turns, passes, turns back
    door = np.ones((3, 3, 5), bool)
    door[0, :, 2] = door[1, :, 2] = False
    c["door_in_another_layer"] = (grid_lattice(5, 3, 3, 0), door, at(grid_lattice(5, 3, 3, 0), 0, 1, 0),
                                  at(grid_lattice(5, 3, 3, 0), 4, 1, 0), 0)
    return c


def scene_cases():
    c = {}
    lat = T.scene_lattice("c2", 4)
    f = T.expected_free("c2", lat)
    sc, _ = R.scene("c2")
    c["c2_diagonal"] = (lat, f, (-3.0, -3.0, 0.0), (3.0, 3.0, 0.0), 2)
    c["c2_scene_goal"] = (lat, f, sc.start[:3], sc.goal[:3], 2)
    c["c2_strip_outside_the_walls"] = (lat, f, (-3.0, -3.0, 0.0), (-5.8, -3.0, 0.0), 2)
    lat4 = T.scene_lattice("c4", 4)
    c["c4_across_the_wall"] = (lat4, T.expected_free("c4", lat4), (-0.9, 0.0, 0.0), (2.0, 0.0, 0.0), 2)
    lat3 = T.scene_lattice("room3", 4)
    sc3, _ = R.scene("room3")
    c["room3"] = (lat3, T.expected_free("room3", lat3), sc3.start[:3], (-4.0, 6.5, 3.0), 2)
    lat1 = T.scene_lattice("c2", 1)
    fm = T.expected_free("c2", lat1, T.MARGIN)
    c["c2_margin_from_the_floor_patch"] = (lat1, fm, (-3.0, -3.0, 0.0), (3.0, 3.0, 0.0), 2)
    c["c2_margin"] = (lat1, fm, (3.4, -3.0, 0.0), (-4.0, 3.0, 0.0), 2)
    c["c2_margin_plain"] = (lat1, f[:1], (3.4, -3.0, 0.0), (-4.0, 3.0, 0.0), 2)
    return c


HANDOVER = 2.0


def case_text(lat, free, frm, to, snap, want_chain=1):
    words = T.pack(free)
    head = [hx(lat.x0), hx(lat.y0), hx(lat.pitch), lat.nx, lat.ny, hx(lat.theta0), hx(lat.dtheta), lat.n_theta,
            lat.wrap_theta] + [hx(a) for a in lat.arm] + [hx(v) for v in frm] + [hx(v) for v in to] + \
        [snap, want_chain, hx(HANDOVER), len(words)]
    return "R " + " ".join(str(v) for v in head) + "\n" + " ".join(str(int(w)) for w in words) + "\n"


def take_case(tok, want_chain=1):
    """One case's answer off the front of the token list."""
    st = int(tok.pop(0))
    nodes = [int(tok.pop(0)) for _ in range(6)]
    n_chain, n_settled = int(tok.pop(0)), int(tok.pop(0))
    cost = float.fromhex(tok.pop(0))
    n_out, j = int(tok.pop(0)), int(tok.pop(0))
    chain = [[int(tok.pop(0)) for _ in range(3)] for _ in range(n_chain if want_chain and st == 0 else 0)]
    rows = [[float.fromhex(tok.pop(0)) for _ in range(8)] for _ in range(n_out)]
    return dict(status=st, from_node=tuple(nodes[:3]), to_node=tuple(nodes[3:]), n_chain=n_chain, n_settled=n_settled,
                cost=cost, j=j, chain=np.array(chain, np.int32).reshape(-1, 3), rows=np.array(rows).reshape(-1, 8))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compare(name, got, exp, lat):
    assert got["status"] == exp["status"], (name, got["status"], exp["status"])
    none = (-1, -1, -1)
    assert got["from_node"] == (exp["from_node"] or none) and got["to_node"] == (exp["to_node"] or none), name
    assert got["n_settled"] == exp["n_settled"], name
    if exp["status"] != T.OK:
        assert got["n_chain"] == 0 and len(got["rows"]) == 0, name
        return
    assert np.array_equal(got["chain"], exp["chain"]), name
    assert same_bits(got["rows"], exp["rows"]), name
    assert got["cost"].hex() == float(exp["cost"]).hex(), name
    assert got["j"] == T.handover(lat, exp["chain"], HANDOVER), name


@pytest.mark.parametrize("which", ["synthetic", "scenes"])
def test_route_table(table, which):
    cases = synthetic_cases() if which == "synthetic" else scene_cases()
    tok = run(table, "".join(case_text(*c) for c in cases.values()))
    for name, (lat, free, frm, to, snap) in cases.items():
        compare(name, take_case(tok), T.route(lat, free, frm, to, snap), lat)
    assert not tok


def test_route_without_chain(table):
    """out_chain = NULL: the rows and the record alone."""
    lat, free, frm, to, snap = synthetic_cases()["straight_and_diagonal"]
    got = take_case(run(table, case_text(lat, free, frm, to, snap, 0)), 0)
    exp = T.route(lat, free, frm, to, snap)
    assert got["status"] == 0 and got["n_chain"] == len(exp["chain"]) and same_bits(got["rows"], exp["rows"])


def test_lattice_fit(table):
    sc, _ = R.scene("c2")
    arm = " ".join(hx(a) for a in T.ARM)
    good = [(sc.env_x, sc.env_y, 0.2, 4, 0.0), (sc.env_x, sc.env_y, 0.05, 16, -0.3), ((0.0, 0.0), (0.0, 1.0), 0.3, 1, 0.0)]
    bad = [((0, 1), (0, 1), 0.0, 4, 0.0), ((0, 1), (0, 1), float("nan"), 4, 0.0), ((0, 1), (0, 1), 0.1, 0, 0.0),
           ((1, 0), (0, 1), 0.1, 4, 0.0), ((0, float("inf")), (0, 1), 0.1, 4, 0.0), ((0, 1), (0, 1), 0.1, 4, float("nan"))]
    huge = [((0, 1e5), (0, 1e5), 0.1, 4, 0.0), ((0, 1e12), (0, 1), 0.1, 1, 0.0)]
    text = "".join("F %s %s %s %s %s %d %s %s\n" % (hx(ex[0]), hx(ex[1]), hx(ey[0]), hx(ey[1]), hx(p), nt, hx(t0), arm)
                   for ex, ey, p, nt, t0 in good + bad + huge)
    tok = run(table, text)
    for ex, ey, p, nt, t0 in good:
        exp = T.fit(ex, ey, p, nt, t0)
        got = [tok.pop(0) for _ in range(10)]
        assert int(got[0]) == 0
        assert [float.fromhex(got[k]).hex() for k in (1, 2, 3, 6, 7)] == [hx(exp.x0), hx(exp.y0), hx(exp.pitch),
                                                                         hx(exp.theta0), hx(exp.dtheta)]
        assert [int(got[k]) for k in (4, 5, 8, 9)] == [exp.nx, exp.ny, exp.n_theta, 1]
    for _ in bad:
        assert int([tok.pop(0) for _ in range(10)][0]) == -1
    for _ in huge:
        assert int([tok.pop(0) for _ in range(10)][0]) == -7
    assert not tok


# ------------------------------------------------------------------------------------------ non-vacuity
def test_synthetic_cases_hold_every_answer():
    c = synthetic_cases()
    r = {k: T.route(*v) for k, v in c.items()}
    assert len(r["one_node"]["rows"]) == 1 and r["one_node"]["cost"] == 0.0 and len(r["from_is_to"]["rows"]) == 1
    assert r["one_node_blocked"]["status"] == T.ERR_START_INVALID
    assert r["ring1_least_distance"]["from_node"] == (4, 3, 0) and r["ring1_tie_to_lower_node"]["from_node"] == (3, 2, 0)
    assert r["ring2"]["from_node"] == (5, 3, 0) and r["ring2_out_of_reach"]["status"] == T.ERR_START_INVALID
    assert r["blocked_start_no_snap"]["status"] == T.ERR_START_INVALID
    assert r["blocked_goal_no_snap"]["status"] == T.ERR_GOAL_INVALID and r["goal_snaps"]["to_node"] == (5, 5, 0)
    assert r["all_blocked"]["status"] == T.ERR_START_INVALID
    assert [r[k]["status"] for k in ("outside", "heading_outside", "nan")] == [T.ERR_ARG] * 3
    lat = c["diagonal_forbidden"][0]
    assert r["diagonal_forbidden"]["cost"] == lat.pitch + lat.pitch and len(r["diagonal_forbidden"]["chain"]) == 3
    assert r["diagonal_allowed"]["cost"] == math.sqrt(lat.pitch * lat.pitch + lat.pitch * lat.pitch)
    assert len(r["turn_wrap1"]["chain"]) == 2 and len(r["turn_wrap0"]["chain"]) == 8
    assert r["turn_wrap1"]["cost"] < r["turn_wrap0"]["cost"]
    assert r["wrap_snaps_heading"]["to_node"] == (2, 2, 5)
    assert sorted(set(r["door_in_another_layer"]["chain"][:, 2].tolist())) == [0, 1, 2]
    # a merged row set is shorter than its chain, and a straight-then-diagonal route keeps exactly its corner
    s = r["straight_and_diagonal"]
    assert len(s["chain"]) == 7 and len(s["rows"]) == 3


def test_scenes_hold_what_the_issue_states():
    """Pitch 0.2 over the scenes' own bounds, arm folded, map only."""
    lat = T.scene_lattice("c2", 4)
    f = T.expected_free("c2", lat)
    assert (lat.nx, lat.ny) == (56, 56) and int(f[0].sum()) == 1992 and int(f.sum()) == 7908 and f.size == 12544
    full = T.route(lat, f, (-3.0, -3.0, 0.0), (3.0, 3.0, 0.0), full=True)
    assert full["status"] == T.OK and full["from_node"] == (15, 15, 0)
    # the strip at x < -5 outside the walls is free but unreachable
    assert f[:, :, :3].any() and full["reached"] < int(f.sum())
    assert T.route(lat, f, (-3.0, -3.0, 0.0), (-5.8, -3.0, 0.0))["status"] == T.ERR_NO_SOLUTION
    lat4 = T.scene_lattice("c4", 4)
    assert T.route(lat4, T.expected_free("c4", lat4), (-0.9, 0.0, 0.0), (2.0, 0.0, 0.0))["status"] == T.ERR_NO_SOLUTION
    lat3 = T.scene_lattice("room3", 4)
    f3 = T.expected_free("room3", lat3)
    sc3, _ = R.scene("room3")
    r3 = T.route(lat3, f3, sc3.start[:3], sc3.goal[:3], full=True)
    assert int(f3[0].sum()) == 3432 and r3["reached"] == int(f3.sum())  # every free node is reachable


def test_margin_case():
    """A map margin of 0.1 on C2, one heading.  Both answers occur and nodes flip against margin 0.  The base rides 2 cm
    above the floor patch the node inserts around the start, so at every positive map margin of
    margin_restatement.POSE_MARGINS (0.1, 0.05) the whole patch, the scene's start at (-3, -3) included, is unclear and
    no route leaves it: the route the tests use joins two nodes off the patch, and it is longer than the plain one."""
    lat = T.scene_lattice("c2", 1)
    plain, wide = T.expected_free("c2", T.scene_lattice("c2", 4))[:1], T.expected_free("c2", lat, T.MARGIN)
    assert 0 < wide.sum() < wide.size and not (wide & ~plain).any()
    assert int((wide != plain).sum()) == 833
    assert T.route(lat, wide, (-3.0, -3.0, 0.0), (3.0, 3.0, 0.0))["status"] == T.ERR_START_INVALID
    a, b = T.route(lat, wide, (3.4, -3.0, 0.0), (-4.0, 3.0, 0.0)), T.route(lat, plain, (3.4, -3.0, 0.0), (-4.0, 3.0, 0.0))
    assert a["status"] == T.OK and b["status"] == T.OK and a["cost"] > b["cost"]


def test_small_lattices_hold_both_answers():
    for n, lat in T.small_lattices().items():
        f = T.expected_free("c2", lat)
        assert f.size == (n if n != "3x" else 231)
        assert n == 1 or 0 < f.sum() < f.size, n
    assert T.expected_free("c2", T.small_lattices()[1]).all()
    lat = T.small_lattices()["3x"]
    assert lat.nx % 32 and lat.n_theta == 3 and (lat.nx * lat.ny) % 32  # tiles straddle rows and layers
    # the disabled-link case flips nodes
    lat = T.scene_lattice("c2", 4)
    assert int((T.expected_free("c2", lat) != T.expected_free("c2", lat, disabled=T.DISABLED_LINK)).sum()) == 5


def test_far_plan_conditions():
    """What the plan_far tests rest on: on C2 at the call's default lattice the handover at 2 m leaves a base stage, and
    one at 50 m leaves none."""
    lat, f, r, j, rows = T.far_case()
    assert 0 < j < len(r["chain"]) - 1
    assert T.handover(lat, r["chain"], 50.0) == 0
    assert r["from_node"] == (30, 30, 0) and np.allclose(rows[0], rows[1], atol=1e-12)  # the start is on its node
    assert len(rows) >= 3
    # The nodes of a route are free, its edges need not be: the base is not round, and a turn in place between two free
    # headings can sweep through a blocked one.  At the call's lattice the dense check finds one such turn (edge 4 -> 5)
    # and the all-pairs shortcut goes round it; at 20 cm the turn at edge 9 -> 10 has no way round: stage 3.
    orc, rev = R.oracle_for("c2"), R.orobot().rev
    fine = R.shortcut(orc, rows, rev, R.N_SEG, R.STEP)
    assert fine["path"] is not None and len(fine["path"]) == 19
    blocked = [p for e, p in enumerate(fine["pairs"]) if p[1] == p[0] + 1 and fine["first"][e] >= 0]
    assert blocked == [(4, 5)] and same_bits(rows[4][:2], rows[5][:2])
    coarse = R.shortcut(orc, T.far_case(pitch=T.COARSE_OPTS["pitch"])[4], rev, R.N_SEG, R.STEP)
    assert coarse["path"] is None and coarse["first_blocked"] == 9


def test_stage3_start():
    """The unfolded start of the stage-3 case: its node is free with the arm folded, a route and a base stage exist,
    and the first edge -- folding the arm in place -- collides at its first point, the start itself, with the map."""
    start = T.stage3_start()
    lat, f, r, j, rows = T.far_case(start)
    assert r["from_node"] == T.STAGE3_NODE and f[0, 64, 86] and j > 0
    assert same_bits(rows[0], start) and same_bits(rows[1][:3], start[:3])
    rev = R.orobot().rev
    _, M = R.density(rows[:1], rows[1:2], rev, R.N_SEG, R.STEP)
    orc = R.oracle_for("c2")
    assert R.first_invalid(orc, rows[:1], rows[1:2], M)[0] == 0
    assert orc.check_configs([start], True, False)[0] == 1 and orc.check_configs([start], False, True)[0] == 0
