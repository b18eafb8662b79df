"""Batched dense edge checks (smp_check_edges, edges_kernel) against the numpy restatement of the density rule in
shortcut_restatement.py, with the validity of every point taken from the CPU oracle: first invalid index and point
count per edge, exactly."""
import numpy as np
import pytest

import gpu_info
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def robot():
    return Robot()


@pytest.fixture(scope="module")
def gp(robot):
    return GpuPlanner(robot)


_GSCENES = {}


def use_scene(gp, name):
    if name not in _GSCENES:
        sc, _ = R.scene(name)
        _GSCENES[name] = Scene.from_keys(sc.keys, sc.res)
    gp.set_scene(_GSCENES[name])
    gp.set_disabled_map_links([])
    return R.scene(name)[0]


@pytest.mark.parametrize("n", [20, 21])
def test_short_edges_of_an_oracle_path(robot, n):
    """The m = 1 edges between consecutive nodes of the oracle's C2 path (seed 3, 300 iterations; the path holds n + 1
    configurations per tree edge, so its nodes are every n-th row): n + 1 points each, and free wherever the oracle
    finds the restated points free.  n = 21 gives 22 points, a ragged tile.  A few of these edges do collide by the
    oracle: after the planner truncates an edge at its last valid point it interpolates the shorter edge anew and does
    not check it again (the reference's behaviour); those must be reported at the oracle's index."""
    rev = R.orobot().rev
    nodes = R.oracle_path("c2", 3, 300, n)[::n]
    m, M = R.density(nodes[:-1], nodes[1:], rev, n, R.STEP)
    a, b = nodes[:-1][m == 1], nodes[1:][m == 1]
    want = R.first_invalid(R.oracle_for("c2"), a, b, M[m == 1])
    assert (want < 0).sum() >= 10
    g = GpuPlanner(robot, num_traj_segments=n)
    use_scene(g, "c2")
    first, npts = g.check_edges(a, b)
    print("n", n, "edges", len(a), "free by the oracle", (want < 0).sum(), "first", first.tolist())
    assert (npts == n + 1).all()
    assert (first[want < 0] == -1).all()
    assert np.array_equal(first, want)


@pytest.mark.parametrize("name", ["c2", "room3"])
def test_long_edges(gp, name):
    """64 long random edges (R.long_edges): first invalid index and point count equal the restatement's.  The seed is
    chosen on the CPU so that the oracle alone gives free edges, colliding ones, collisions in a later tile, one at
    index 0 and an edge of 8 hops or more."""
    a, b = R.long_edges(name)
    m, M = R.density(a, b, R.orobot().rev, R.N_SEG, R.STEP)
    want = R.first_invalid(R.oracle_for(name), a, b, M)
    assert (want < 0).sum() >= 8 and (want >= 0).sum() >= 8
    assert (want >= R.CT).sum() >= 4 and (want == 0).sum() >= 1 and m.max() >= 8
    use_scene(gp, name)
    first, npts = gp.check_edges(a, b)
    print(name, "first", first.tolist(), "points", npts.tolist())
    assert first.dtype == np.int64 and npts.dtype == np.int32
    assert np.array_equal(npts, M + 1)
    assert np.array_equal(first, want)


def test_flags_and_disabled_links(gp):
    """The same batch without the map check, without the self check, and with one arm link's map collisions disabled,
    each against the oracle built with the same setting; every setting changes some edge's answer."""
    name = "c2"
    a, b = R.long_edges(name)
    _, M = R.density(a, b, R.orobot().rev, R.N_SEG, R.STEP)
    use_scene(gp, name)
    base = R.first_invalid(R.oracle_for(name), a, b, M)
    for self_, map_ in ((True, False), (False, True)):
        want = R.first_invalid(R.oracle_for(name), a, b, M, self_, map_)
        assert (want != base).any()
        first, _ = gp.check_edges(a, b, check_self=self_, check_map=map_)
        print("self", self_, "map", map_, "changed", int((want != base).sum()))
        assert np.array_equal(first, want)
    link = "arm_link4"
    names = R.orobot().link_names
    me = np.array([0 if n == link else 1 for n in names], np.uint8)
    want = R.first_invalid(R.oracle_for(name, map_enabled=me), a, b, M)
    assert (want != base).any()
    gp.set_disabled_map_links([link])
    try:
        first, _ = gp.check_edges(a, b)
    finally:
        gp.set_disabled_map_links([])
    assert np.array_equal(first, want)


def test_edge_cases(gp, robot):
    sc = use_scene(gp, "c2")
    n, f = R.N_SEG, R.STEP
    first, npts = gp.check_edges(np.zeros((0, 8)), np.zeros((0, 8)))
    assert len(first) == 0 and len(npts) == 0
    start = np.array(sc.start)
    goal = np.array(sc.goal)
    # one edge
    _, Mg = R.density([start], [goal], R.orobot().rev, n, f)
    want = R.first_invalid(R.oracle_for("c2"), [start], [goal], Mg)
    first, npts = gp.check_edges([start], [goal])
    assert first.tolist() == want.tolist() and npts.tolist() == [Mg[0] + 1]
    # a == b: m = 1, n + 1 identical points, the answer of check_configs (a valid and an invalid configuration)
    q = R.random_configs(sc, 64, 5)
    v = R.oracle_for("c2").check_configs(q)
    assert 0 < v.sum() < len(v)
    first, npts = gp.check_edges(q, q)
    assert (npts == n + 1).all()
    assert np.array_equal(first, np.where(v, -1, 0))
    assert np.array_equal(gp.check_configs(q), v)
    # max(L) / f an exact integer: a pure x move of 3 f is 3 hops, not 4
    to = start.copy()
    to[0] = start[0] + 3 * f
    assert to[0] - start[0] == 3 * f
    m, M = R.density([start], [to], R.orobot().rev, n, f)
    assert m.tolist() == [3]
    want = R.first_invalid(R.oracle_for("c2"), [start], [to], M)
    first, npts = gp.check_edges([start], [to])
    assert npts.tolist() == [3 * n + 1] and first.tolist() == want.tolist()
    # map checks without a scene are refused; the self check alone runs
    bare = GpuPlanner(robot)
    with pytest.raises(L.SmpError) as e:
        bare.check_edges([start], [goal])
    assert e.value.status == L.SMP_ERR_ARG
    first, _ = bare.check_edges([start], [goal], check_map=False)
    assert first.tolist() == R.first_invalid(R.oracle_for("c2"), [start], [goal], Mg, True, False).tolist()


def test_more_edges_than_workgroups(gp):
    """A table of more edges than twice the CU count, so that every workgroup goes round the work loop more than once
    (one workgroup per CU): the 64 long edges of C2, then a == b edges of random configurations, 21 points each, whose
    answer is check_configs' of that configuration (test_edge_cases).  The expectation is the oracle's alone."""
    name = "c2"
    cus = gpu_info.device_cus()
    sc = use_scene(gp, name)
    la, lb = R.long_edges(name)
    q = R.random_configs(sc, 2 * cus + 1, 11)
    a, b = np.concatenate([la, q]), np.concatenate([lb, q])
    assert len(a) > 2 * cus
    orc = R.oracle_for(name)
    _, M = R.density(la, lb, R.orobot().rev, R.N_SEG, R.STEP)
    v = orc.check_configs(q)
    assert 0 < v.sum() < len(v)
    want = np.concatenate([R.first_invalid(orc, la, lb, M), np.where(v, -1, 0)])
    want_pts = np.concatenate([M + 1, np.full(len(q), R.N_SEG + 1)])
    first, npts = gp.check_edges(a, b)
    print("CUs", cus, "edges", len(a), "valid configurations", int(v.sum()), "of", len(v))
    assert np.array_equal(npts, want_pts)
    assert np.array_equal(first, want)


def test_deterministic(gp):
    a, b = R.long_edges("room3")
    use_scene(gp, "room3")
    f1, n1 = gp.check_edges(a, b)
    f2, n2 = gp.check_edges(a, b)
    assert np.array_equal(f1, f2) and np.array_equal(n1, n2)
