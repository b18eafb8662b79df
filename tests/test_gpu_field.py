"""The cost field on the GPU (smp_base_cost_field, smp_base_route_gpu, smp_plan_far's route_device) against
field_restatement.py: costs as bit patterns, parents, reached counts, and the device route against the host route in
every output.  No tolerance is involved: the field has one solution.  test_field_cpu.py pins, on the CPU,
that the maps hold every kind of case."""
import ctypes

import numpy as np
import pytest

import field_restatement as F
import lattice_restatement as T
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene, base_route

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    return GpuPlanner(Robot())


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def route_or_error(fn):
    """(status, rows, chain, info) of a route call."""
    try:
        out = fn()
        return (L.SMP_OK,) + tuple(out[:3])
    except L.SmpError as e:
        return e.status, None, None, e.info


def check_field(gp, lat, free, src, cost_exp, parent_exp, reached_exp):
    cost, parent, info = gp.base_cost_field(lat, free, src)
    print(info)
    assert info["fell_back"] == 0 and info["n_nodes"] == cost.size
    bad = np.flatnonzero(cost.reshape(-1).view(np.uint64) != cost_exp.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    assert np.array_equal(parent.reshape(-1), parent_exp)
    assert info["n_reached"] == reached_exp
    assert info["rounds"] <= info["launches"] and info["tile_runs"] >= info["rounds"] - 1
    return info


def check_route(gp, lat, free, frm, to, snap):
    """base_route_gpu equals base_route on the same bits in every output."""
    h = route_or_error(lambda: base_route(lat, free, frm, to, snap))
    d = route_or_error(lambda: gp.base_route_gpu(lat, free, frm, to, snap))
    assert d[0] == h[0]
    assert d[3] == h[3], (d[3], h[3])   # from_node, to_node, n_chain, n_settled, cost
    if h[0] == L.SMP_OK:
        assert np.array_equal(d[2], h[2]) and same_bits(d[1], h[1])
    return d


# ------------------------------------------------------------------------------------------ the synthetic maps
@pytest.mark.parametrize("name", list(F.maps()))
def test_maps(gp, name):
    lat, free, frm, to, snap = F.maps()[name]
    e = F.expected(name)
    info = check_field(gp, lat, free, e["route"]["from_node"], e["cost"], e["parent"], len(e["order"]))
    d = check_route(gp, lat, free, frm, to, snap)
    assert d[0] == e["route"]["status"] and d[3]["n_settled"] == e["route"]["n_settled"]
    if name in F.ONE_TILE:
        assert info["rounds"] == 2   # one working round and the certificate
    if name == "maze":
        assert info["rounds"] >= 3
    if name == "isolated_source":
        assert info["n_reached"] == 1


def test_parent_may_be_left_out(gp):
    lat, free = F.maps()["door_in_another_layer"][:2]
    e = F.expected("door_in_another_layer")
    cost, parent, _ = gp.base_cost_field(lat, free, e["route"]["from_node"], want_parent=False)
    assert parent is None and same_bits(cost.reshape(-1), e["cost"])


def test_fallback_to_the_host_search(gp):
    """A pitch of 2^60 and a heading step of 1e-3: one axis step away from the source a heading step no longer moves
    the cost, the field has more than one solution, and both calls answer with the host search (fell_back = 1)."""
    lat = F.grid_lattice(3, 3, 2, 1, 2.0 ** 60, 1e-3)
    free = np.ones((2, 3, 3), bool)
    free[0, 1, 1] = False
    frm, to = F.at(lat, 0, 0, 0), F.at(lat, 2, 2, 1)
    exp = T.route(lat, free, frm, to, 0)
    assert exp["status"] == T.OK and exp["from_node"] == (0, 0, 0) and exp["to_node"] == (2, 2, 1)
    cost_exp, parent_exp, order = F.dijkstra(lat, free, (0, 0, 0))
    assert not F.unique(float(cost_exp[np.isfinite(cost_exp)].max()), lat)
    cost, parent, info = gp.base_cost_field(lat, free, (0, 0, 0))
    assert info["fell_back"] == 1 and info["n_reached"] == len(order)
    assert same_bits(cost.reshape(-1), cost_exp) and np.array_equal(parent.reshape(-1), parent_exp)
    d = check_route(gp, lat, free, frm, to, 0)
    rows, chain, rinfo, finfo = gp.base_route_gpu(lat, free, frm, to, 0)
    assert finfo["fell_back"] == 1 and d[0] == L.SMP_OK
    assert np.array_equal(chain, exp["chain"]) and same_bits(rows, exp["rows"]) and rinfo["cost"] == exp["cost"]
    assert rinfo["n_settled"] == exp["n_settled"]


def test_larger_then_smaller(gp):
    """Two calls in a row, the larger lattice first: the buffers only grow, and no flag of the first call survives."""
    for name in ("random", "door_in_another_layer", "maze", "from_is_to"):
        lat, free, frm, to, snap = F.maps()[name]
        e = F.expected(name)
        check_field(gp, lat, free, e["route"]["from_node"], e["cost"], e["parent"], len(e["order"]))
        check_route(gp, lat, free, frm, to, snap)


# ------------------------------------------------------------------------------------------ C2
_GSCENES = {}


def use_scene(gp, name):
    if name not in _GSCENES:
        sc, _ = R.scene(name)
        _GSCENES[name] = Scene.from_keys(sc.keys, sc.res)
    gp.set_scene(_GSCENES[name])
    gp.set_disabled_map_links([])


@pytest.mark.parametrize("which", ["scene_lattice", "far_case"])
def test_c2(gp, which):
    """The GPU's own free map of C2 as input: route and field equal the host route and the restatement."""
    use_scene(gp, "c2")
    sc, _ = R.scene("c2")
    if which == "scene_lattice":
        lat, frm = T.scene_lattice("c2", 4), sc.start[:3]
        exp_free = T.expected_free("c2", lat)
    else:
        lat, exp_free = T.far_case()[:2]
        frm = T.FAR_START[:3]
    free, _ = gp.base_free_map(lat)
    assert np.array_equal(free, exp_free)
    d = check_route(gp, lat, free, frm, sc.goal[:3], 2)
    assert d[0] == L.SMP_OK
    exp = T.route(lat, exp_free, frm, sc.goal[:3], 2)
    assert np.array_equal(d[2], exp["chain"]) and same_bits(d[1], exp["rows"]) and d[3]["cost"] == exp["cost"]
    cost, parent, order = F.dijkstra(lat, exp_free, exp["from_node"])
    check_field(gp, lat, free, exp["from_node"], cost, parent, len(order))


def far_query():
    sc, _ = R.scene("c2")
    return GpuPlanner.make_query(T.FAR_START, sc.goal, sc.env_x, sc.env_y, **T.FAR_BUDGET)


@pytest.mark.parametrize("opts", [T.FAR_OPTS, T.COARSE_OPTS], ids=["far_case", "blocked_turn"])
def test_plan_far_with_the_route_on_the_device(gp, opts):
    use_scene(gp, "c2")
    a = gp.plan_far(far_query(), route_device=0, **opts)
    b = gp.plan_far(far_query(), route_device=1, **opts)
    assert a["status"] == b["status"] and a["far"]["stage"] == b["far"]["stage"]
    assert a["far"]["stage"] == (0 if opts is T.FAR_OPTS else 3)
    assert same_bits(a["path"], b["path"])
    for k in ("route", "handover_node", "n_route_rows"):
        assert a["far"][k] == b["far"][k], k
    strip = lambda c: {k: v for k, v in c.items() if not k.endswith("_ms")}
    assert strip(a["far"]["check"]) == strip(b["far"]["check"])
    assert a["far"]["route"]["n_chain"] > 0


# ------------------------------------------------------------------------------------------ errors
def test_errors(gp):
    lat, free, frm, to, snap = F.maps()["door_in_another_layer"]
    for src in ((2, 1, 0), (5, 1, 0), (0, 3, 0), (0, 0, 3), (-1, 0, 0)):   # blocked, then outside
        with pytest.raises(L.SmpError) as e:
            gp.base_cost_field(lat, free, src)
        assert e.value.status == L.SMP_ERR_ARG, src
    with pytest.raises(L.SmpError) as e:
        gp.base_cost_field(lat._replace(pitch=0.0), free, (0, 1, 0))
    assert e.value.status == L.SMP_ERR_ARG
    blocked = np.zeros_like(free)
    blocked[0, 1, 4] = True
    for f, a, b, st in ((blocked, F.at(lat, 0, 1), F.at(lat, 4, 1), L.SMP_ERR_START_INVALID),
                        (blocked, F.at(lat, 4, 1), F.at(lat, 0, 1), L.SMP_ERR_GOAL_INVALID),
                        (free, (-50.0, 0.5, 0.1), F.at(lat, 4, 1), L.SMP_ERR_ARG)):
        d = check_route(gp, lat, f, a, b, 1)
        assert d[0] == st
    # a NULL planner
    cl = ctypes.byref(L.BaseLattice(0.0, 0.0, 0.1, 2, 2, 0.0, 0.5, 1, 0, (ctypes.c_double * 5)(*T.ARM)))
    bits, src = (ctypes.c_uint32 * 1)(15), (ctypes.c_int32 * 3)(0, 0, 0)
    assert L.lib().smp_base_cost_field(None, cl, bits, src, None, None, None) == L.SMP_ERR_ARG
