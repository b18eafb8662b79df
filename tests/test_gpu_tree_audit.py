"""The tree audit (tree_audit.py) on the GPU planner's own state: GpuPlanner.export_state() and the plan's result dict,
checked by plain tree arithmetic.  No oracle takes part: a rule written alike in the kernels and in the oracle passes
every parity test, and does not pass here unless it also leaves a tree whose costs follow from its configurations.

Each case is one single-query plan with path_optimality_threshold = -inf; the switches of each path through the kernels
(helpers, scouts, early ask, distributed scans, segment counts) are the ones the parity tests set."""
import math
import os

import numpy as np
import pytest

import attach_restatement as A
import tree_audit as TA
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REV = np.array([0, 0, 1, 1, 1, 1, 1, 1], bool)  # joint_is_revolute of the model JSON (checked below)
_SCENES = {}


def scene(name):
    """The scenes of test_gpu_parity.scene_pair, without the oracle's grid."""
    if name not in _SCENES:
        if name.startswith("room"):
            f = np.load(os.path.join(GOLD, name + "_keys.npz"))
            keys = np.concatenate([f["keys"].astype(np.int64), scenes.floor_keys([0.0, 0.0], 0.05, 3.0)])
            sc = scenes.Scene(name, keys, 0.05, [0, 0, 0] + scenes.ARM_FOLDED, [1, 1, 0] + scenes.ARM_UNFOLDED,
                              (0, 0), (0, 0))
            sc.env_x, sc.env_y = sc.bounds()
        else:
            sc = {"c1": scenes.empty_room, "c2": scenes.box_room, "c4": scenes.narrow_passage}[name]()
        _SCENES[name] = (sc, Scene.from_keys(sc.keys, sc.res))
    return _SCENES[name]


@pytest.fixture(scope="module")
def robot():
    import json
    assert np.array_equal(np.array(json.load(open(L.MODEL_JSON))["joint_is_revolute"], bool), REV)
    return Robot()


def plan_and_audit(robot, name, params=None, **query):
    """One plan on scene `name` by a fresh planner with `params`, audited: (result, report)."""
    sc, gscene = scene(name)
    gp = GpuPlanner(robot, path_optimality_threshold=-math.inf, **(params or {}))
    gp.set_scene(gscene)
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, **query))
    assert r["status"] in (0, L.SMP_ERR_NO_SOLUTION)
    rep = TA.audit(gp.export_state(), r, sc.start, sc.goal, gp.params.num_traj_segments, gp.params.near_threshold, REV)
    print(name, params, query, rep)
    assert rep.info["have_sol"] == (r["status"] == 0)
    assert rep.ok and rep.skipped == [], str(rep)
    return r, rep


def test_default_provisioning_a_bent_connection(robot):
    """Box room, seed 5, 3000 iterations: trees rewired 700 times and 15 deep, and a connection whose via chain is bent
    -- c_best's total is the straight edge's (birrt_star.cpp:2651-2668, 3267), 0.1085 below the returned path's length,
    the revolute and prismatic parts are the path's own.  The audit is not trivially clean on such a run."""
    r, rep = plan_and_audit(robot, "c2", iterations=3000, seed=5)
    assert r["status"] == 0 and r["scout"] >= 1 and r["helpers"] > 0
    assert max(rep.info["rewires[start]"], rep.info["rewires[goal]"]) >= 500
    assert max(rep.info["depth[start]"], rep.info["depth[goal]"]) >= 15
    assert rep.info["c_best_below_tree_sum"] > 1e-3 and abs(rep.info["c_best_below_tree_sum"] - 0.1085) < 1e-4
    assert rep.residuals["A5.cbest_parts"] <= rep.info["tol_c[start]"] + rep.info["tol_c[goal]"]
    assert rep.residuals["A6.last_is_goal"] == 0.0


def test_a_straight_connection(robot):
    """Box room, seed 8, 600 iterations: here c_best's total equals the tree sum."""
    r, rep = plan_and_audit(robot, "c2", iterations=600, seed=8)
    assert r["status"] == 0
    assert abs(rep.info["c_best_below_tree_sum"]) <= rep.info["tol_c[start]"] + rep.info["tol_c[goal]"]


def test_alone_on_its_workgroup(robot):
    r, rep = plan_and_audit(robot, "c2", dict(helpers=-1), iterations=1500, seed=8)
    assert r["status"] == 0 and max(rep.info["rewires[start]"], rep.info["rewires[goal]"]) > 100


@pytest.mark.parametrize("scouts", [2, 4, 8])
def test_scout_counts(robot, scouts):
    r, rep = plan_and_audit(robot, "c2", dict(helpers=63, scout=scouts), iterations=2000, seed=5)
    assert r["status"] == 0 and r["scout"] == scouts


def test_early_ask(robot, monkeypatch):
    for k in ("SMP_PRE_REFRESH", "SMP_PRE_COMMIT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SMP_EARLY_ASK", "1")
    r, rep = plan_and_audit(robot, "c2", iterations=3000, seed=1)
    assert r["status"] == 0 and 0 <= r["first_solution_iter"] < 1000


@pytest.mark.parametrize("scan_min,helpers,scouts,iters,seed", [(64, 0, 1, 3000, 5), (64, 63, 0, 1500, 9),
                                                               (600, 0, 1, 3000, 13)])
def test_distributed_scans(robot, monkeypatch, scan_min, helpers, scouts, iters, seed):
    monkeypatch.setenv("SMP_SCAN_MIN", str(scan_min))
    r, rep = plan_and_audit(robot, "c2", dict(helpers=helpers, scout=scouts), iterations=iters, seed=seed)
    assert max(r["nodes_start"], r["nodes_goal"]) > scan_min


@pytest.mark.parametrize("n_pts", [10, 21, 22, 32])
def test_segment_counts(robot, n_pts):
    r, rep = plan_and_audit(robot, "c2", dict(num_traj_segments=n_pts), iterations=1500, seed=7)
    assert r["status"] == 0 and r["scout"] >= 1
    assert (len(r["path"]) - 1) % n_pts == 0


def test_relaunched_in_chunks(robot, monkeypatch):
    """Launches of 64 iterations (SMP_CHUNK0, as test_single_query_relaunched_equals_one_launch): the loop state, the
    nB / nA copies among it, goes through QState and back eleven times."""
    monkeypatch.setenv("SMP_CHUNK0", "64")
    r, rep = plan_and_audit(robot, "c2", iterations=700, seed=3)
    assert r["status"] == 0


def test_sample_budget(robot):
    r, rep = plan_and_audit(robot, "c2", samples=30000, seed=11)
    assert r["configs_checked"] >= 30000


def test_budget_too_small_for_a_solution(robot):
    r, rep = plan_and_audit(robot, "c2", iterations=5, seed=3)
    assert r["status"] == L.SMP_ERR_NO_SOLUTION and len(r["path"]) == 0
    assert "A5.cbest_total" not in rep.residuals and "A3.edge_cost[start]" in rep.residuals


def test_direct_connection_before_the_loop(robot):
    """room3 connects start and goal before the first iteration (birrt_star.cpp:1072-1075): the goal tree is its root,
    the path is the start tree's via chain and, as in the reference (birrt_star.cpp:6246-6273), ends one interpolation
    point before the goal."""
    r, rep = plan_and_audit(robot, "room3", iterations=300, seed=4)
    assert r["status"] == 0 and r["iterations"] == 0 and r["nodes_goal"] == 1
    assert rep.info["path_edges"][1] == 0 and "A6.last_is_goal" not in rep.residuals
    assert len(r["path"]) == rep.info["path_edges"][0] * 20


@pytest.mark.parametrize("name,seed,iters", [("c1", 1, 50), ("c4", 2, 400)])
def test_other_scenes(robot, name, seed, iters):
    r, rep = plan_and_audit(robot, name, iterations=iters, seed=seed)
    assert r["status"] == 0


def test_attached_bar(robot):
    """The robot with the 10-sphere bar on its hand (66 collision items: two per lane, the flat self lists)."""
    r, rep = plan_and_audit(Robot().attach(A.HAND, *A.bar(10)), "c2", iterations=1500, seed=20)
    assert r["nodes_start"] + r["nodes_goal"] > 200


def test_large_trees(robot):
    """20 000 iterations: trees of 13 282 and 11 496 nodes, rewired 1419 and 1183 times."""
    r, rep = plan_and_audit(robot, "c2", iterations=20000, seed=7)
    assert r["status"] == 0 and min(r["nodes_start"], r["nodes_goal"]) > 10000
    assert min(rep.info["rewires[start]"], rep.info["rewires[goal]"]) > 1000
