"""Clearance queries (smp_clearance_configs, smp_clearance_edges) against the numpy restatement in
clearance_restatement.py: values bit for bit, indices exactly.  test_clearance_cpu.py pins, on the CPU, that these
inputs hold every kind of answer."""
import ctypes

import numpy as np
import pytest

import clearance_restatement as C
import gpu_info
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
_pd = ctypes.POINTER(ctypes.c_double)
FIELDS = ("map", "self", "map_link", "self_a", "self_b")


@pytest.fixture(scope="module")
def gp():
    return GpuPlanner(Robot())


_GSCENES = {}


def use_scene(gp, name, disabled=()):
    if name not in _GSCENES:
        sc, _ = R.scene(name)
        _GSCENES[name] = Scene.from_keys(sc.keys, sc.res)
    gp.set_scene(_GSCENES[name])
    gp.set_disabled_map_links(list(disabled))


def same(got, exp, fields=FIELDS):
    for f in fields:
        bad = np.flatnonzero(got[f] != exp[f])
        assert len(bad) == 0, (f, bad[:8], got[f][bad[:8]], exp[f][bad[:8]])


@pytest.mark.parametrize("name", C.SCENES)
@pytest.mark.parametrize("D", [0.05, 0.3])
@pytest.mark.parametrize("n", [1, 33, 97])
def test_configs(gp, name, D, n):
    exp = C.expected(name, n, D)
    use_scene(gp, name)
    got = gp.clearance(C.poses(name)[:n], D)
    print(name, D, n, "kernel ms", gp.clearance_info["kernel_ms"])
    same(got, exp)
    assert (got["pad"] == 0).all()
    assert gp.clearance_info["n_points"] == n
    assert gp.clearance_info["kernel_ms"] > 0 and gp.clearance_info["total_ms"] >= gp.clearance_info["kernel_ms"]


@pytest.mark.parametrize("name", C.SCENES)
def test_wide_query_distance(gp, name):
    q = C.poses(name)[:8]
    exp = C.clearance(name, q, 1.0)
    assert (exp["map"] > 0.3).any()
    use_scene(gp, name)
    same(gp.clearance(q, 1.0), exp)


@pytest.mark.parametrize("name", C.SCENES)
def test_each_flag_alone(gp, name):
    D, n = 0.3, 33
    use_scene(gp, name)
    q = C.poses(name)[:n]
    full = C.expected(name, n, D)
    got = gp.clearance(q, D, with_self=False)
    same(got, C.expected(name, n, D, False, True))
    assert np.array_equal(got["map"], full["map"]) and np.isposinf(got["self"]).all()
    assert (got["self_a"] == -1).all() and (got["self_b"] == -1).all()
    got = gp.clearance(q, D, with_map=False)
    same(got, C.expected(name, n, D, True, False))
    assert np.array_equal(got["self"], full["self"]) and (got["map"] == D).all() and (got["map_link"] == -1).all()
    got = gp.clearance(q, D, with_self=False, with_map=False)
    assert (got["map"] == D).all() and np.isposinf(got["self"]).all()


@pytest.mark.parametrize("name", C.SCENES)
def test_disabled_arm_link(gp, name):
    D = 0.3
    exp = C.expected(name, C.N_POSES, D, disabled=True)
    use_scene(gp, name, [C.DISABLED_LINK])
    try:
        got = gp.clearance(C.poses(name), D)
        ea, eb = C.edges(name)
        ge = gp.edge_clearance(ea[:2], eb[:2], D)
    finally:
        gp.set_disabled_map_links([])
    same(got, exp)
    link = R.orobot().link_names.index(C.DISABLED_LINK)
    assert (got["map_link"] != link).all()
    ee = C.edge_clearance(name, ea[:2], eb[:2], D, map_enabled=C.map_enabled_for(True))
    same(ge, ee, C.EDGE_FIELDS)


@pytest.mark.parametrize("name", C.SCENES)
def test_edges(gp, name):
    D = 0.3
    a, b = C.edges(name)
    exp = C.edges_expected(name, D)
    use_scene(gp, name)
    got = gp.edge_clearance(a, b, D)
    print(name, "points", exp["points"], "kernel ms", gp.clearance_info["kernel_ms"])
    same(got, exp, C.EDGE_FIELDS)
    assert np.array_equal(got["n_points"], exp["M"] + 1)
    assert gp.clearance_info["n_points"] == exp["points"]
    # the booleans of the same edges: an edge is free exactly when both minima are positive
    first, npts = gp.check_edges(a, b)
    assert np.array_equal(npts, got["n_points"])
    assert np.array_equal(first < 0, (got["map"] > 0) & (got["self"] > 0))
    # an edge of one tile and of one point short of two
    one = gp.edge_clearance(a[:1], a[:1], D)
    assert one["n_points"][0] == R.N_SEG + 1
    c0 = C.clearance(name, a[:1], D)
    assert one["map"][0] == c0["map"][0] and one["self"][0] == c0["self"][0]
    assert one["map_point"][0] == (0 if c0["map"][0] < D else -1) and one["self_point"][0] == 0


def test_more_edges_than_workgroups(gp):
    """A table of more edges than twice the CU count, so that every workgroup goes round the work loop more than once
    (one workgroup per CU): a == b edges over the 97 cached poses, repeated.  Such an edge is 21 identical points, so its
    minima and links are the pose's record and the lowest point attaining them is point 0."""
    name, D = "c2", 0.3
    cus = gpu_info.device_cus()
    exp = C.expected(name, C.N_POSES, D)
    idx = np.arange(2 * cus + 1) % C.N_POSES
    q = C.poses(name)[idx]
    assert len(q) > 2 * cus
    use_scene(gp, name)
    got = gp.edge_clearance(q, q, D)
    print("CUs", cus, "edges", len(q), "kernel ms", gp.clearance_info["kernel_ms"])
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != exp[f][idx])
        assert len(bad) == 0, (f, bad[:8], got[f][bad[:8]], exp[f][idx][bad[:8]])
    assert (got["n_points"] == R.N_SEG + 1).all()
    assert np.array_equal(got["map_point"], np.where(exp["map"][idx] < D, 0, -1))
    assert (got["self_point"] == 0).all()
    assert gp.clearance_info["n_points"] == len(q) * (R.N_SEG + 1)


def test_edges_flags_alone(gp):
    name, D = "c2", 0.3
    a, b = C.edges(name)
    a, b = a[:3], b[:3]
    use_scene(gp, name)
    got = gp.edge_clearance(a, b, D, with_self=False)
    same(got, C.edge_clearance(name, a, b, D, with_self=False), C.EDGE_FIELDS)
    assert np.isposinf(got["self"]).all() and (got["self_point"] == -1).all() and (got["self_a"] == -1).all()
    got = gp.edge_clearance(a, b, D, with_map=False)
    same(got, C.edge_clearance(name, a, b, D, with_map=False), C.EDGE_FIELDS)
    assert (got["map"] == D).all() and (got["map_point"] == -1).all() and (got["map_link"] == -1).all()


def test_path_clearance(gp):
    D = 0.3
    w = C.path12()
    use_scene(gp, "c2")
    edges, s = gp.path_clearance(w, D)
    exp = C.edge_clearance("c2", w[:-1], w[1:], D)
    same(edges, exp, C.EDGE_FIELDS)
    names = gp.robot.link_names
    im, is_ = int(np.argmin(exp["map"])), int(np.argmin(exp["self"]))
    assert s["map"] == exp["map"].min() and s["self"] == exp["self"].min()
    assert s["map_edge"] == (im if exp["map"][im] < D else -1) and s["map_point"] == exp["map_point"][im]
    assert s["map_link"] == (names[exp["map_link"][im]] if exp["map_link"][im] >= 0 else None)
    assert s["self_edge"] == is_ and s["self_point"] == exp["self_point"][is_]
    assert s["self_links"] == (names[exp["self_a"][is_]], names[exp["self_b"][is_]])
    assert s["n_points"] == exp["points"]


def test_errors_and_empty_input(gp):
    name = "c2"
    use_scene(gp, name)
    lib = L.lib()
    q = np.ascontiguousarray(C.poses(name)[:2])
    qp = q.ctypes.data_as(_pd)
    c = (L.Clearance * 2)()
    e = (L.EdgeClearance * 2)()
    info = L.ClearanceInfo()
    A = L.SMP_ERR_ARG
    # n = 0
    assert lib.smp_clearance_configs(gp.h, None, 0, 0.3, 1, 1, None, ctypes.byref(info)) == L.SMP_OK
    assert lib.smp_clearance_edges(gp.h, None, None, 0, 0.3, 1, 1, None, None) == L.SMP_OK
    assert info.n_points == 0
    assert len(gp.clearance(np.zeros((0, 8)))) == 0 and len(gp.edge_clearance(np.zeros((0, 8)), np.zeros((0, 8)))) == 0
    # a NULL output
    assert lib.smp_clearance_configs(gp.h, qp, 2, 0.3, 1, 1, None, None) == A
    assert lib.smp_clearance_edges(gp.h, qp, qp, 2, 0.3, 1, 1, None, None) == A
    # max_dist not finite or not positive, or reaching the clamp of the box-gap field
    for bad in (0.0, -0.1, float("inf"), float("nan"), 13.0):
        assert lib.smp_clearance_configs(gp.h, qp, 2, bad, 1, 1, c, None) == A, bad
        assert lib.smp_clearance_edges(gp.h, qp, qp, 2, bad, 1, 1, e, None) == A, bad
    assert lib.smp_clearance_configs(gp.h, qp, 2, 12.0, 1, 0, c, None) == L.SMP_OK
    # a non-finite coordinate
    for v in (float("nan"), float("inf")):
        qb = q.copy()
        qb[1, 3] = v
        bp = qb.ctypes.data_as(_pd)
        assert lib.smp_clearance_configs(gp.h, bp, 2, 0.3, 1, 1, c, None) == A
        assert lib.smp_clearance_edges(gp.h, qp, bp, 2, 0.3, 1, 1, e, None) == A
        assert lib.smp_clearance_edges(gp.h, bp, qp, 2, 0.3, 1, 1, e, None) == A
    # an edge of more than SMP_EDGE_MAX_POINTS points
    far = q.copy()
    far[:, 0] += 1.0e6
    assert lib.smp_clearance_edges(gp.h, qp, far.ctypes.data_as(_pd), 2, 0.3, 1, 1, e, None) == A
    # more than SMP_EDGE_TABLE_MAX items: refused before the rows are read
    assert lib.smp_clearance_configs(gp.h, qp, L.SMP_EDGE_TABLE_MAX + 1, 0.3, 1, 1, c, None) == L.SMP_ERR_CAPACITY
    assert lib.smp_clearance_edges(gp.h, qp, qp, L.SMP_EDGE_TABLE_MAX + 1, 0.3, 1, 1, e, None) == L.SMP_ERR_CAPACITY
    # with_map without a scene; the self part alone is answered
    bare = GpuPlanner(gp.robot)
    assert lib.smp_clearance_configs(bare.h, qp, 2, 0.3, 1, 1, c, None) == A
    assert lib.smp_clearance_edges(bare.h, qp, qp, 2, 0.3, 1, 1, e, None) == A
    got = bare.clearance(q, 0.3, with_map=False)
    assert np.array_equal(got["self"], C.expected(name, 2, 0.3)["self"])
    # the planner still answers after the refusals
    same(gp.clearance(q, 0.3), C.expected(name, 2, 0.3))
