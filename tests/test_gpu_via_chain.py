"""Via chains (choose-parent's and connectGraphs' stepping from a node towards a target without collision checks,
via_chain in smp_kernels.hip) against the CPU oracle, bit for bit: trees, costs, counters, path and cost rows, as
assert_same_run of test_gpu_parity.py compares them.

Wave 0 takes the steps of a chain alone, in batches of VIA_B = 16 rows kept in LDS; after each batch the whole workgroup
forms the steps' segment norms, their ordered sums, the nodes' costs (a prefix over the steps) and the ViaNode rows.
At the default step factor 0.5 a C2 chain has at most 9 steps, so the long chains get their own inputs (chain length
read from the oracle's trees: the longest run of nodes whose parent is the previous id):

  C2, step factor 0.1, 700 iterations   chains of 17 and more steps (longer than the scouts' PRE_VIA, so the leader steps
                                        them itself before the first solution) and of 33 and more (several batches), at
                                        20 / 21 / 22 / 32 / 10 interpolation segments: 21 | 22 are the two lane layouts
                                        of the norms, 32 is MAX_PTS;
  C1, step factor 0.02                  the run starts with one chain of about 90 steps (more than two batches of 32);
  the C2 seed-2 case with helpers=-1 and with scout=0: the leader computes every chain and every edge cost itself;
  C2 at the default step factor         with the via-step counter asserted, so that a plan that never enters the chain
                                        cannot pass as parity."""
import math

import numpy as np
import pytest

from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Scene

pytestmark = pytest.mark.gpu

# (num_traj_segments, seed): the oracle's first path comes at iteration 150 / 244 / 288 / 270 / 208
C2_LONG = ((20, 2), (21, 3), (22, 4), (32, 4), (10, 1))
C2_ITERS = 700


@pytest.fixture(scope="module")
def pairs():
    from oracle import oracle as O
    out = {}
    for name, sc in (("c1", scenes.empty_room()), ("c2", scenes.box_room())):
        out[name] = (sc, Scene.from_keys(sc.keys, sc.res), O.OracleScene(sc.keys, sc.res))
    return out


_ORACLE = {}


def oracle_plan(orobot, pairs, name, seed, iters, step, n_pts):
    """The oracle's plan of a case, computed once and shared (read-only) by the tests that compare against it."""
    from oracle import oracle as O
    key = (name, seed, iters, step, n_pts)
    if key not in _ORACLE:
        sc, _, osc = pairs[name]
        _ORACLE[key] = O.Oracle(orobot, osc).plan(sc.start, sc.goal, env_x=sc.env_x, env_y=sc.env_y, max_iter=iters,
                                                  seed=seed, opt_thresh=-math.inf, step=step, n_pts=n_pts)
    return _ORACLE[key]


def gpu_plan(pairs, name, seed, iters, step, n_pts, **prov):
    sc, gscene, _ = pairs[name]
    gp = GpuPlanner(path_optimality_threshold=-math.inf, step_factor=step, num_traj_segments=n_pts, **prov)
    gp.set_scene(gscene)
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, iterations=iters, seed=seed))
    return gp, r


def chain_lengths(o):
    """Lengths of the runs of nodes whose parent is the previous id, over both of the oracle's trees."""
    runs = []
    for name in ("start", "goal"):
        par = np.asarray(o[name + "_parent"])
        run = 0
        for i in range(1, len(par)):
            if par[i] == i - 1:
                run += 1
            else:
                if run:
                    runs.append(run)
                run = 0
        if run:
            runs.append(run)
    return np.array(runs)


def assert_same_run(gp, r, o):
    assert r["status"] == {0: 0, 1: L.SMP_ERR_NO_SOLUTION}[o["status"]]
    assert r["iterations"] == o["iterations"]
    assert r["first_solution_iter"] == o["first_iter"]
    assert r["configs_checked"] == o["checked"]
    assert r["configs_valid"] == o["valid"]
    assert r["nodes_start"] == o["n_start"] and r["nodes_goal"] == o["n_goal"]
    assert r["rewires_start"] == o["rewires_start"] and r["rewires_goal"] == o["rewires_goal"]
    assert r["edges_start"] == o["edges_start"] and r["edges_goal"] == o["edges_goal"]
    for w, name in ((0, "start"), (1, "goal")):
        par, conf, cost = gp.tree(w)
        assert np.array_equal(par, o[name + "_parent"]), name
        assert np.array_equal(conf, o[name + "_conf"]), (name, np.abs(conf - o[name + "_conf"]).max())
        assert np.array_equal(cost, o[name + "_cost"]), name
    assert r["cost_best"] == o["cost"]
    if r["status"] == 0:
        assert r["connected_tree_is_start"] == o["conn_start"]
        assert r["conn_node_b"] == o["conn_b"] and r["conn_node_a"] == o["conn_a"]
        assert r["path"].shape == o["path"].shape
        assert np.array_equal(r["path"], o["path"])
    assert np.array_equal(r["cost_rows"][:, [0, 2, 3, 4]], o["cost_rows"][:, [0, 2, 3, 4]])


@pytest.mark.parametrize("n_pts,seed", C2_LONG)
def test_long_chains_c2(orobot, pairs, n_pts, seed):
    o = oracle_plan(orobot, pairs, "c2", seed, C2_ITERS, 0.1, n_pts)
    runs = chain_lengths(o)
    assert 0 <= o["first_iter"] <= C2_ITERS - 350  # the chains before and after the first solution
    assert (runs >= 17).sum() >= 50 and (runs >= 33).sum() >= 9, (runs.max(), (runs >= 17).sum(), (runs >= 33).sum())
    gp, r = gpu_plan(pairs, "c2", seed, C2_ITERS, 0.1, n_pts)
    assert r["scout"] >= 1
    assert r["phases"]["n_via_steps"] > 0
    assert_same_run(gp, r, o)


@pytest.mark.parametrize("prov", [{"helpers": -1}, {"scout": 0}], ids=["helpers=-1", "scout=0"])
def test_long_chains_c2_leader_alone(orobot, pairs, prov):
    n_pts, seed = C2_LONG[0]
    o = oracle_plan(orobot, pairs, "c2", seed, C2_ITERS, 0.1, n_pts)
    gp, r = gpu_plan(pairs, "c2", seed, C2_ITERS, 0.1, n_pts, **prov)
    assert r["scout"] == 0
    assert_same_run(gp, r, o)


@pytest.mark.parametrize("step,n_pts,longest", [(0.02, 20, 65), (0.03, 22, 60), (0.05, 20, 36)])
def test_one_long_chain_c1(orobot, pairs, step, n_pts, longest):
    """The empty room's first connect is one chain: about 90 steps at 0.02 (more than two batches of up to 32), 61 at
    0.03 with the three-norms-per-lane layout, 37 at 0.05."""
    o = oracle_plan(orobot, pairs, "c1", 3, 200, step, n_pts)
    assert chain_lengths(o).max() >= longest
    gp, r = gpu_plan(pairs, "c1", 3, 200, step, n_pts)
    assert_same_run(gp, r, o)
    assert r["nodes_start"] + r["nodes_goal"] >= longest + 2  # the chain's nodes are in the tree


def test_default_step_factor_takes_via_steps(orobot, pairs):
    o = oracle_plan(orobot, pairs, "c2", 1, 600, 0.5, 20)
    gp, r = gpu_plan(pairs, "c2", 1, 600, 0.5, 20)
    assert r["scout"] >= 1
    assert r["phases"]["n_via_steps"] > 0
    assert_same_run(gp, r, o)
