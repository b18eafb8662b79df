"""The scene built on the GPU from occupied keys (smp_planner_set_scene_keys / _bt / _ot / _octomap_msg) against the
host builders (smp_scene_from_* + smp_planner_set_scene): every case builds planner A's scene on the host and planner
B's on the device for the same robot and requires the device-resident arrays -- bricks, box-gap field, byte field,
slab fields -- and the layout to be equal.  The contract is equality: the host's EDT holds integers in doubles, the
device's saturating integer passes give the same numbers (DESIGN.md "Scene build")."""
import ctypes
import os

import numpy as np
import pytest

from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEY = 32768


@pytest.fixture(scope="module")
def robot():
    return Robot()


@pytest.fixture(scope="module")
def pair(robot):
    """(A, B): A takes host-built scenes, B builds on the device.  Shared by the cases, so B's buffers and scratch
    always hold an earlier scene."""
    return GpuPlanner(robot), GpuPlanner(robot)


@pytest.fixture(scope="module")
def c2():
    return scenes.box_room()


def same(a, b):
    """scene_arrays() of two planners: equal layout, equal arrays."""
    (la, ba, da, dba, sa), (lb, bb, db, dbb, sb) = a, b
    assert tuple(la.dims) == tuple(lb.dims) and tuple(la.origin) == tuple(lb.origin)
    assert la.resolution == lb.resolution
    assert (la.n_bricks, la.n_cells, la.n_prim, la.has_d2b) == (lb.n_bricks, lb.n_cells, lb.n_prim, lb.has_d2b)
    assert np.array_equal(ba, bb), "bricks"
    assert np.array_equal(da, db), "d2: %d cells differ" % np.count_nonzero(da != db)
    assert (dba is None) == (dbb is None)
    if dba is not None:
        assert np.array_equal(dba, dbb), "d2b"
    assert np.array_equal(sa, sb), "slab: %d cells differ" % np.count_nonzero(sa != sb)


def same_info(info, scene):
    i = scene.info()
    assert info["n_occupied"] == i["n_occupied"]
    assert info["dims"] == i["dims"] and info["origin"] == i["origin"] and info["resolution"] == i["res"]
    assert info["bbox_min"] == i["bbox_min"] and info["bbox_max"] == i["bbox_max"]
    assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"]


def keys_case(pair, keys, res, **kw):
    """Host build on A, device build on B, compared; returns (host scene, A's arrays, info)."""
    A, B = pair
    scene = Scene.from_keys(keys, res, **kw)
    A.set_scene(scene)
    info = B.set_scene_keys(keys, res, **kw)
    a = A.scene_arrays()
    same(a, B.scene_arrays())
    same_info(info, scene)
    return scene, a, info


def line(ext, dy=0, dz=0):
    """Two keys spanning `ext` cells along x (dy, dz: the second key's offset on the other axes)."""
    return np.array([[KEY, KEY, KEY], [KEY + ext - 1, KEY + dy, KEY + dz]], np.uint16)


def test_empty_scene_is_one_free_cell(pair):
    scene, a, info = keys_case(pair, np.zeros((0, 3), np.uint16), 0.05)
    assert tuple(a[0].dims) == (1, 1, 1) and a[2].tolist() == [65535] and a[1].tolist() == [0]
    assert info["n_occupied"] == 0


def test_single_voxel(pair):
    scene, a, info = keys_case(pair, [[KEY, KEY, KEY]], 0.05)
    assert tuple(a[0].dims) == (23, 23, 23) and info["n_occupied"] == 1
    assert a[2].min() == 0 and np.count_nonzero(a[2] == 0) == 27  # the voxel and its dilation


@pytest.mark.parametrize("ext,dy,dz,dims", [(42, 0, 0, (64, 23, 23)), (43, 0, 0, (65, 23, 23)),
                                            (44, 2, 2, (66, 25, 25))])
def test_word_and_brick_boundaries(pair, ext, dy, dz, dims):
    """nx a multiple of 64; one bit into a second word with nx % 4 == 1; ny % 4 and nz % 4 non-zero."""
    scene, a, info = keys_case(pair, line(ext, dy, dz), 0.05)
    assert tuple(a[0].dims) == dims
    assert info["n_occupied"] == 2 and sum(bin(int(w)).count("1") for w in a[1]) == 2


def test_clamp_and_wide_intermediates(pair):
    """Two keys 600 cells apart: cells at the 65535 clamp and cells between 255 and 65535 (their exact squared
    distances exceed 16 bits in the intermediate passes of a non-saturating transform)."""
    scene, a, info = keys_case(pair, line(600), 0.05)
    d2 = a[2]
    assert tuple(a[0].dims) == (622, 23, 23) and d2.size == 329038
    assert np.count_nonzero(d2 == 65535) == 45494
    assert np.count_nonzero((d2 > 255) & (d2 < 65535)) == 256032


def test_duplicates_and_floor(pair):
    rng = np.random.default_rng(5)
    k = (KEY + rng.integers(-20, 20, (300, 3))).astype(np.uint16)
    k[:, 2] = KEY - 1 + rng.integers(0, 3, 300)  # some map cells lie in the floor's layer (key of z = -res / 2)
    keys = np.concatenate([k, k])
    scene, a, info = keys_case(pair, keys, 0.05, floor_center=(0.1, -0.2), floor_distance=1.5)
    distinct = len(np.unique(k, axis=0))
    floor = (2 * int(1.5 / 0.05) + 1) ** 2
    assert distinct < info["n_occupied"] < distinct + floor  # floor cells overlap map cells, duplicates count once


def test_no_byte_field_at_fine_resolution(pair):
    """res 5 mm: the largest sphere's threshold is 324 >= 255, so the scene has no byte field."""
    A, B = pair
    scene, a, info = keys_case(pair, [[KEY, KEY, KEY]], 0.005)
    assert a[0].has_d2b == 0 and a[3] is None
    assert 180 <= a[0].dims[0] <= 190


@pytest.fixture(scope="module")
def patch_keys():
    rng = np.random.default_rng(9)
    return (KEY + rng.integers(0, [100, 100, 50], (20000, 3))).astype(np.uint16)


def test_byte_field_at_2cm(pair, patch_keys):
    scene, a, info = keys_case(pair, patch_keys, 0.02)
    assert a[0].has_d2b == 1 and tuple(a[0].dims) == (150, 150, 100)
    assert np.array_equal(a[3], np.minimum(a[2], 255).astype(np.uint8))


@pytest.mark.parametrize("name", ["box_room", "narrow_passage"])
def test_project_scenes(pair, name):
    sc = getattr(scenes, name)()
    scene, a, info = keys_case(pair, sc.keys, sc.res)
    assert a[0].n_prim > 0 and a[4].min() == 0 and a[4].max() > 0  # the slabs are exercised


@pytest.mark.parametrize("floor", [None, (0.3, -0.4)])
@pytest.mark.parametrize("room", ["room3", "room4", "room5"])
def test_octomap_forms(pair, room, floor):
    A, B = pair
    bt = open(os.path.join(GOLD, room + ".bt"), "rb").read()
    ot = open(os.path.join(GOLD, room + ".ot"), "rb").read()
    res = float(np.load(os.path.join(GOLD, room + "_keys.npz"))["res"])
    body = lambda d: d[d.index(b"\ndata\n") + 6:]
    cases = [(Scene.from_bt(bt, floor_center=floor), lambda: B.set_scene_bt(bt, floor_center=floor)),
             (Scene.from_ot(ot, floor_center=floor), lambda: B.set_scene_ot(ot, floor_center=floor)),
             (Scene.from_octomap_msg("OcTree", res, True, body(bt), floor_center=floor),
              lambda: B.set_scene_octomap_msg("OcTree", res, True, body(bt), floor_center=floor)),
             (Scene.from_octomap_msg("OcTree", res, False, body(ot), floor_center=floor),
              lambda: B.set_scene_octomap_msg("OcTree", res, False, body(ot), floor_center=floor))]
    for scene, build in cases:
        assert scene.info()["n_occupied"] > 1000
        A.set_scene(scene)
        info = build()
        same(A.scene_arrays(), B.scene_arrays())
        same_info(info, scene)


def test_reuse_of_buffers_and_scratch(robot, c2, patch_keys):
    """One planner through scenes of different sizes: stale occupancy bits, stale scratch or a stale byte-field pointer
    after the buffers are reused would show."""
    A, B = GpuPlanner(robot), GpuPlanner(robot)
    for keys, res in [(c2.keys, c2.res), (line(43), 0.05), (c2.keys, c2.res), (patch_keys, 0.02),
                      (np.array([[KEY, KEY, KEY]]), 0.005), (patch_keys, 0.02)]:
        A.set_scene(Scene.from_keys(keys, res))
        B.set_scene_keys(keys, res)
        a, b = A.scene_arrays(), B.scene_arrays()
        assert a[0].has_d2b == (0 if res == 0.005 else 1)
        same(a, b)


def test_checks_and_plan_through_the_built_scene(robot, c2):
    """What the array comparison does not see (the planner's SceneDev / MapCfg fields): validity flags of 10,000
    random configurations and one 120-iteration plan, bit for bit."""
    A, B = GpuPlanner(robot), GpuPlanner(robot)
    A.set_scene(Scene.from_keys(c2.keys, c2.res))
    B.set_scene_keys(c2.keys, c2.res)
    rng = np.random.default_rng(17)
    q = np.column_stack([rng.uniform(-5.5, 5.5, 10000), rng.uniform(-5.5, 5.5, 10000),
                         rng.uniform(-3.14, 3.14, (10000, 6))])
    va, vb = A.check_configs(q), B.check_configs(q)
    assert 0 < va.sum() < len(va) and np.array_equal(va, vb)
    assert np.array_equal(A.check_configs(q, check_self=False), B.check_configs(q, check_self=False))
    query = GpuPlanner.make_query(c2.start, c2.goal, c2.env_x, c2.env_y, iterations=120, seed=3)
    ra, rb = A.plan(query), B.plan(query)
    for f in ("status", "iterations", "configs_checked", "configs_valid", "nodes_start", "nodes_goal", "edges_start",
              "edges_goal", "rewires_start", "rewires_goal"):
        assert ra[f] == rb[f], f
    assert np.array_equal(ra["path"], rb["path"])
    for which in (0, 1):
        (pa, ca, _), (pb, cb, _) = A.tree(which), B.tree(which)
        assert np.array_equal(pa, pb) and np.array_equal(ca, cb)


def test_errors_keep_the_previous_scene(robot, c2):
    B = GpuPlanner(robot)
    B.set_scene_keys(c2.keys, c2.res)
    rng = np.random.default_rng(23)
    q = np.column_stack([rng.uniform(-5.5, 5.5, 2000), rng.uniform(-5.5, 5.5, 2000), rng.uniform(-3.14, 3.14, (2000, 6))])
    before = B.check_configs(q)
    assert 0 < before.sum() < len(before)
    lib = L.lib()
    o = L.SceneOpts()
    lib.smp_scene_opts_default(o)
    assert lib.smp_planner_set_scene_keys(B.h, None, 3, ctypes.byref(o), None) == L.SMP_ERR_ARG
    assert np.array_equal(B.check_configs(q), before)
    with pytest.raises(L.SmpError) as e:
        B.set_scene_keys(c2.keys, 0.0)
    assert e.value.status == L.SMP_ERR_ARG
    assert np.array_equal(B.check_configs(q), before)
    bt = open(os.path.join(GOLD, "room3.bt"), "rb").read()
    with pytest.raises(L.SmpError) as e:
        B.set_scene_bt(bt[:len(bt) // 2])
    assert e.value.status == L.SMP_ERR_PARSE
    assert np.array_equal(B.check_configs(q), before)
