"""The far-goal stage on the GPU (smp_base_free_map, smp_plan_far) against lattice_restatement.py: the free map's words
exactly against the CPU oracle's map check of every node (with a margin: margin_restatement.py's predicate), and against
the GPU's own check_configs / check_clear of the same host-formed configurations; the staged plan's route rows, handover
and tail bit for bit against the restatement and the calls it is made of.  test_lattice_cpu.py pins, on the CPU, that
these inputs hold every kind of answer."""
import numpy as np
import pytest

import gpu_info
import lattice_restatement as T
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene, base_lattice_fit, base_route

pytestmark = pytest.mark.gpu


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


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_map(gp, name, lat, mm=0.0, disabled=None):
    """The free map of `lat` equals the restatement's, word for word."""
    exp = T.expected_free(name, lat, mm, disabled)
    free, info = gp.base_free_map(lat, margin=mm if mm > 0 else None)
    bad = np.argwhere(free != exp)
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    assert np.array_equal(gp.base_map_bits, T.pack(exp))  # (the unused bits of the last word are 0)
    assert info["n_nodes"] == exp.size and info["n_free"] == int(exp.sum())
    return free, info


# ------------------------------------------------------------------------------------------ the free map
@pytest.mark.parametrize("n", [1, 31, 32, 33, 97, "3x"])
def test_small_lattices(gp, n):
    """N = 1, 31, 32, 33 and 97 nodes, and nx = 11 with three headings: tiles straddle rows and layers."""
    use_scene(gp, "c2")
    lat = T.small_lattices()[n]
    free, _ = check_map(gp, "c2", lat)
    last = int(gp.base_map_bits[-1])
    assert last >> (free.size % 32 or 32) == 0


@pytest.mark.parametrize("name", ["c2", "room3", "c4"])
def test_scene_lattices(gp, name):
    use_scene(gp, name)
    _, info = check_map(gp, name, T.scene_lattice(name, 4))
    print(name, info)


def test_fit_is_the_restatement(gp):
    sc, _ = R.scene("c2")
    lat, exp = base_lattice_fit(sc.env_x, sc.env_y, T.PITCH, 4), T.scene_lattice("c2", 4)
    assert (lat.nx, lat.ny, lat.n_theta, lat.wrap_theta) == (exp.nx, exp.ny, 4, 1)
    assert same_bits([lat.x0, lat.y0, lat.pitch, lat.theta0, lat.dtheta] + list(lat.arm),
                     [exp.x0, exp.y0, exp.pitch, exp.theta0, exp.dtheta] + list(exp.arm))
    use_scene(gp, "c2")
    assert np.array_equal(gp.base_free_map(lat)[0], gp.base_free_map(exp)[0])


def test_margin(gp):
    use_scene(gp, "c2")
    lat = T.scene_lattice("c2", 1)
    free, info = check_map(gp, "c2", lat, T.MARGIN)
    print("margin", T.MARGIN, info)
    # the margin's self part is ignored
    assert np.array_equal(gp.base_free_map(lat, margin=(T.MARGIN, 0.5))[0], free)


def test_disabled_link(gp):
    use_scene(gp, "c2", [T.DISABLED_LINK])
    try:
        check_map(gp, "c2", T.scene_lattice("c2", 4), disabled=T.DISABLED_LINK)
    finally:
        gp.set_disabled_map_links([])


def test_more_tiles_than_workgroups(gp):
    """C2 with enough headings for more tiles than twice the CU count, so that every workgroup goes round the work loop
    more than once."""
    cus = gpu_info.device_cus()
    per_layer = T.n_nodes(T.scene_lattice("c2", 1))
    n_theta = (2 * cus * 32) // per_layer + 2
    lat = T.scene_lattice("c2", n_theta)
    assert (T.n_nodes(lat) + 31) // 32 > 2 * cus
    use_scene(gp, "c2")
    _, info = check_map(gp, "c2", lat)
    print("headings", n_theta, info)


@pytest.mark.parametrize("mm", [0.0, T.MARGIN])
def test_the_checkers_own_answer(gp, mm):
    """The API's own statement of the definition: check_configs / check_clear of the host-formed configurations."""
    use_scene(gp, "c2")
    lat = T.small_lattices()["3x"] if mm == 0.0 else T.sub_lattice(T.scene_lattice("c2", 1), 0, 28, 56, 8)
    q = T.node_configs(lat)
    free, _ = gp.base_free_map(lat, margin=mm if mm > 0 else None)
    if mm > 0:
        own = gp.check_clear(q, False, True, margin=(mm, 0.0))
    else:
        own = gp.check_configs(q, False, True)
    assert 0 < own.sum() < len(own)
    assert np.array_equal(free.reshape(-1), own.astype(bool))


def test_errors(gp):
    use_scene(gp, "c2")
    good = T.small_lattices()[33]
    nan = float("nan")
    bad = [good._replace(pitch=0.0), good._replace(pitch=-0.1), good._replace(nx=0), good._replace(ny=0),
           good._replace(n_theta=0), good._replace(x0=nan), good._replace(pitch=nan), good._replace(dtheta=float("inf")),
           good._replace(arm=(0.0, nan, 0.0, 0.0, 0.0))]
    for lat in bad:
        with pytest.raises(L.SmpError) as e:
            gp.base_free_map(lat)
        assert e.value.status == L.SMP_ERR_ARG, lat
    with pytest.raises(L.SmpError) as e:
        gp.base_free_map(good._replace(nx=8192, ny=8192, n_theta=2))  # 2^27 nodes
    assert e.value.status == L.SMP_ERR_CAPACITY
    for m in (nan, -0.01, 20.0):  # what smp_check_configs_margin refuses
        with pytest.raises(L.SmpError) as e:
            gp.base_free_map(good, margin=m)
        assert e.value.status == L.SMP_ERR_ARG, m
    with pytest.raises(L.SmpError) as e:
        GpuPlanner(Robot()).base_free_map(good)  # no scene
    assert e.value.status == L.SMP_ERR_ARG


def test_route_over_the_gpu_map(gp):
    """base_route over the GPU's own map: the restatement's chain, rows and cost."""
    use_scene(gp, "c2")
    lat = T.scene_lattice("c2", 4)
    free, _ = gp.base_free_map(lat)
    sc, _ = R.scene("c2")
    exp = T.route(lat, T.expected_free("c2", lat), sc.start[:3], sc.goal[:3], 2)
    rows, chain, info = base_route(lat, free, sc.start[:3], sc.goal[:3], 2)
    assert same_bits(rows, exp["rows"]) and np.array_equal(chain, exp["chain"])
    assert info["cost"] == exp["cost"] and info["n_settled"] == exp["n_settled"]


# ------------------------------------------------------------------------------------------ the staged plan
def far_query(start=T.FAR_START, goal=None):
    sc, _ = R.scene("c2")
    return GpuPlanner.make_query(start, sc.goal if goal is None else goal, sc.env_x, sc.env_y, **T.FAR_BUDGET)


def test_plan_far(gp):
    use_scene(gp, "c2")
    lat, free, r, j, rows = T.far_case()
    d = gp.plan_far(far_query(), handover_distance=2.0, **T.FAR_OPTS)
    far = d["far"]
    print({k: far[k] for k in ("stage", "handover_node", "n_route_rows", "route_ms", "total_ms")}, far["map"],
          "status", d["status"], "rows", len(d["path"]))
    n = far["n_route_rows"]
    assert n > 0
    assert far["map"]["n_nodes"] == free.size and far["map"]["n_free"] == int(free.sum())
    assert far["route"]["from_node"] == r["from_node"] and far["route"]["to_node"] == r["to_node"]
    assert far["route"]["n_chain"] == len(r["chain"]) and far["route"]["cost"] == r["cost"]
    assert far["route"]["n_settled"] == r["n_settled"]
    assert far["handover_node"] == tuple(int(v) for v in r["chain"][j])
    # the route rows: the restatement's rows through the GPU's own dense check
    short, sinfo = gp.shortcut_path(rows, True, True, window=0)
    assert n == len(short) and same_bits(d["path"][:n], short)
    for f in ("n_edges", "n_valid", "configs_checked", "cost_in", "cost_out", "first_blocked"):
        assert far["check"][f] == sinfo[f], f
    # the tail: the plain plan of the handover query
    tail = gp.plan(far_query(start=short[-1]))
    assert d["status"] == tail["status"] and far["stage"] == (0 if tail["status"] == L.SMP_OK else 4)
    assert d["status"] == L.SMP_OK, d["status"]
    assert same_bits(tail["path"][0], short[-1])
    assert same_bits(d["path"], T.stitch(short, tail["path"]))
    assert d["iterations"] == tail["iterations"] and d["configs_checked"] == tail["configs_checked"]
    assert np.array_equal(d["cost_rows"][:, [0, 2, 3, 4]], tail["cost_rows"][:, [0, 2, 3, 4]])
    # the joint row appears once
    assert same_bits(d["path"][n - 1], short[-1]) and not same_bits(d["path"][n], short[-1])
    # every adjacent edge of the route part passes the dense check
    first, _ = gp.check_edges(d["path"][:n - 1], d["path"][1:n])
    assert (first < 0).all()


def test_plan_far_with_a_long_handover_is_the_plain_plan(gp):
    use_scene(gp, "c2")
    d = gp.plan_far(far_query(), handover_distance=50.0, **T.FAR_OPTS)
    plain = gp.plan(far_query())
    assert d["far"]["n_route_rows"] == 0 and d["far"]["stage"] == (0 if plain["status"] == L.SMP_OK else 4)
    assert d["status"] == plain["status"] and same_bits(d["path"], plain["path"])
    assert d["far"]["handover_node"] == T.far_case()[2]["from_node"]


def test_plan_far_across_the_wall(gp):
    use_scene(gp, "c4")
    sc, _ = R.scene("c4")
    q = GpuPlanner.make_query(sc.start, [2.0, 0.0, 0.0] + list(T.ARM), sc.env_x, sc.env_y, **T.FAR_BUDGET)
    d = gp.plan_far(q, **T.FAR_OPTS)
    assert d["status"] == L.SMP_ERR_NO_SOLUTION and d["far"]["stage"] == 2
    assert d["far"]["n_route_rows"] == 0 and len(d["path"]) == 0


def test_plan_far_unfolded_start_in_collision(gp):
    """The first edge folds the arm; here it collides at the start itself, and the dense check says so."""
    use_scene(gp, "c2")
    d = gp.plan_far(far_query(start=T.stage3_start()), **T.FAR_OPTS)
    assert d["status"] == L.SMP_ERR_NO_SOLUTION and d["far"]["stage"] == 3
    assert d["far"]["check"]["first_blocked"] == 0 and len(d["path"]) == 0
    assert d["far"]["route"]["from_node"] == T.STAGE3_NODE


def test_plan_far_turn_in_place_blocked(gp):
    """At 20 cm the route turns in place between two free headings through a blocked one, and no pair of its rows goes
    round the turn: the dense check says so (test_lattice_cpu.py: edge 9)."""
    use_scene(gp, "c2")
    d = gp.plan_far(far_query(), **T.COARSE_OPTS)
    assert d["status"] == L.SMP_ERR_NO_SOLUTION and d["far"]["stage"] == 3
    assert d["far"]["check"]["first_blocked"] == 9 and len(d["path"]) == 0


def test_plan_far_argument_errors(gp):
    use_scene(gp, "c2")
    sc, _ = R.scene("c2")
    unconfined = GpuPlanner.make_query(T.FAR_START, sc.goal, **T.FAR_BUDGET)
    assert gp.plan_far(unconfined, **T.FAR_OPTS)["status"] == L.SMP_ERR_ARG
    for opts in (dict(pitch=0.0), dict(n_theta=0), dict(map_margin=-1.0), dict(handover_distance=float("nan"))):
        d = gp.plan_far(far_query(), **dict(T.FAR_OPTS, **opts))
        assert d["status"] == L.SMP_ERR_ARG and d["far"]["stage"] == 1, opts
