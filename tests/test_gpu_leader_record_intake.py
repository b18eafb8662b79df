"""The leader's post-solution connect takes the rows of tree_B's nearest node and of its near candidates from the scout's
connect record instead of loading them, and the node a via chain starts from out of the candidate batch it already
holds ("Round 12").  A row taken from the wrong place, a row that a rewire commit has rewritten since, or
a barrier removed between a writer and its reader would give trees that differ from the CPU oracle's, so every case
compares trees, parents, costs, counters, path and connection ids with the oracle bit for bit.  The counters
scout_conn_row_hits / scout_conn_batch_hits count the connects that took the record's rows, so that a build that never
does cannot pass as parity.

  provisionings   C2, 600 iterations, three seeds whose first path comes before iteration 300, under the default
                  provisioning (two scouts after the first path: SC_CONN records), 12 / 7 / 15 helpers (one scout: no
                  SC_CONN record, the leader loads connect's rows itself), no job board, no scout;
  appended nodes  C2 at step factor 0.1 across the first solution: via chains of up to 49 nodes, so that more nodes are
                  appended between a record's snapshot and its use than the 64 a one-wave scan of the appended nodes
                  takes (the leader reads appended nodes from memory, as before: the scans of few and of many);
  rewires         the C2 runs commit rewires on both trees (asserted): a row kept from before a commit must not be used;
  C1 direct       the empty room, 50 iterations: connect has no near candidates (and, as it turns out, no record)."""
import math

import numpy as np
import pytest

from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Scene

pytestmark = pytest.mark.gpu

ITERATIONS = 600
SEEDS = (1, 2, 3)  # as tests/test_gpu_scout_record_order.py: the oracle's first path comes before iteration 300
PROVISIONINGS = ({}, {"helpers": 12}, {"helpers": 7}, {"helpers": -1}, {"scout": 0}, {"helpers": 15})
LONG = dict(seed=2, iters=700, step=0.1, n_pts=20)  # tests/test_gpu_via_chain.py: first path at iteration 150


@pytest.fixture(scope="module")
def rooms():
    from oracle import oracle as O
    out = {}
    for name, sc in (("c1", scenes.empty_room()), ("c2", scenes.box_room())):
        out[name] = (sc, Scene.from_keys(sc.keys, sc.res), O.OracleScene(sc.keys, sc.res))
    return out


_ORACLE = {}


def oracle_plan(orobot, rooms, name, seed, iters, **kw):
    """The oracle's plan of a case, computed once and shared (read-only) by the tests that compare against it."""
    from oracle import oracle as O
    key = (name, seed, iters, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        sc, _, osc = rooms[name]
        _ORACLE[key] = O.Oracle(orobot, osc).plan(sc.start, sc.goal, env_x=sc.env_x, env_y=sc.env_y, max_iter=iters,
                                                  seed=seed, opt_thresh=-math.inf, **kw)
    return _ORACLE[key]


def gpu_plan(rooms, name, seed, iters, **params):
    sc, gscene, _ = rooms[name]
    gp = GpuPlanner(path_optimality_threshold=-math.inf, **params)
    gp.set_scene(gscene)
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, iterations=iters, seed=seed))
    return gp, r


def assert_same_run(gp, r, o, what=None):
    assert r["status"] == {0: 0, 1: L.SMP_ERR_NO_SOLUTION}[o["status"]], what
    assert r["iterations"] == o["iterations"] and r["first_solution_iter"] == o["first_iter"], what
    assert r["configs_checked"] == o["checked"] and r["configs_valid"] == o["valid"], what
    assert r["nodes_start"] == o["n_start"] and r["nodes_goal"] == o["n_goal"], what
    assert r["rewires_start"] == o["rewires_start"] and r["rewires_goal"] == o["rewires_goal"], what
    assert r["edges_start"] == o["edges_start"] and r["edges_goal"] == o["edges_goal"], what
    for w, name in ((0, "start"), (1, "goal")):
        par, conf, cost = gp.tree(w)
        assert np.array_equal(par, o[name + "_parent"]), (what, name)
        assert np.array_equal(conf, o[name + "_conf"]) and np.array_equal(cost, o[name + "_cost"]), (what, name)
    assert r["cost_best"] == o["cost"], what
    if r["status"] == 0:
        assert r["connected_tree_is_start"] == o["conn_start"], what
        assert r["conn_node_b"] == o["conn_b"] and r["conn_node_a"] == o["conn_a"], what
        assert r["path"].shape == o["path"].shape and np.array_equal(r["path"], o["path"]), what
    assert np.array_equal(r["cost_rows"][:, [0, 2, 3, 4]], o["cost_rows"][:, [0, 2, 3, 4]]), what


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


@pytest.mark.parametrize("prov", PROVISIONINGS, ids=lambda p: ",".join("%s=%d" % kv for kv in p.items()) or "default")
@pytest.mark.parametrize("seed", SEEDS)
def test_provisionings_answer_as_the_oracle(orobot, rooms, seed, prov):
    o = oracle_plan(orobot, rooms, "c2", seed, ITERATIONS)
    assert 0 <= o["first_iter"] < 300
    # rewire commits on both trees: they rewrite a node's row, which the leader may hold a copy of
    assert o["rewires_start"] > 0 and o["rewires_goal"] > 0
    gp, r = gpu_plan(rooms, "c2", seed, ITERATIONS, **prov)
    print("seed %d %s (%d helpers, %d scouts): scout hits nn %d near %d edge %d, edge misses %d" % (
        seed, prov, r["helpers"], r["scout"], r["scout_nn_hits"], r["scout_near_hits"], r["scout_edge_hits"],
        r["scout_edge_misses"]))
    assert_same_run(gp, r, o, (seed, prov))
    assert r["rewires_start"] > 0 and r["rewires_goal"] > 0
    if prov.get("scout", 1) == 0 or prov.get("helpers", 0) < 0:
        assert r["scout"] == 0
    elif prov:
        assert r["scout"] == 1  # one scout: no SC_CONN record, connect's rows are the leader's own loads
        assert r["scout_conn_row_hits"] == 0 and r["scout_conn_batch_hits"] == 0
    else:
        # the benched provisioning: the records (connect's among them) must be taken, or parity proves nothing
        assert r["scout"] >= 2
        assert r["scout_nn_hits"] > 0 and r["scout_near_hits"] > 0
        assert r["scout_edge_hits"] > r["scout_edge_misses"]
        # ... and the rows of connect's nearest node and of its candidate batch taken from them
        print("   connect rows from the record: nearest %d, batch %d" % (r["scout_conn_row_hits"],
                                                                        r["scout_conn_batch_hits"]))
        assert r["scout_conn_row_hits"] > 0 and r["scout_conn_batch_hits"] > 0


@pytest.mark.parametrize("prov", [{}, {"helpers": 12}], ids=["default", "helpers=12"])
def test_more_appended_nodes_than_one_wave_scans(orobot, rooms, prov):
    o = oracle_plan(orobot, rooms, "c2", LONG["seed"], LONG["iters"], step=LONG["step"], n_pts=LONG["n_pts"])
    runs = chain_lengths(o)
    assert 0 <= o["first_iter"] <= LONG["iters"] - 350  # chains before and after the first solution
    # an iteration appends up to two chains (choose-parent's and connect's) and a record is used two iterations after
    # its snapshot: chains of 33 and more nodes put more than 64 nodes between them
    assert (runs >= 33).sum() >= 9, (runs.max(), (runs >= 33).sum())
    assert o["rewires_start"] > 0 and o["rewires_goal"] > 0
    gp, r = gpu_plan(rooms, "c2", LONG["seed"], LONG["iters"], step_factor=LONG["step"],
                     num_traj_segments=LONG["n_pts"], **prov)
    assert r["scout"] >= 1 and r["scout_nn_hits"] > 0
    assert_same_run(gp, r, o, prov)


def test_c1_direct_without_near_candidates(orobot, rooms):
    o = oracle_plan(orobot, rooms, "c1", 1, 50)
    assert 0 <= o["first_iter"] < 10  # the empty room connects at once: the rest are post-solution iterations
    gp, r = gpu_plan(rooms, "c1", 1, 50)
    assert r["scout"] >= 2  # two scouts after the first solution: connect records
    assert_same_run(gp, r, o)
    # This query's direct path is optimal from iteration 0 on: no later iteration inserts a node (5 and 1 nodes at the
    # end, at 50 as at 400 iterations), and its leader takes no scout record of any stage, on the parent commit as
    # well -- so the case pins the paths without a record and without near candidates, and the counters are printed,
    # not asserted.  Connect records are asserted on in the default-provisioning cases of C2 above.
    print("c1: connect rows from the record: nearest %d, batch %d, near hits %d" % (
        r["scout_conn_row_hits"], r["scout_conn_batch_hits"], r["scout_near_hits"]))
