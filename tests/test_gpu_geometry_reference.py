"""The HIP entry points against the independent geometric reference (geometry_reference.py): FK, the boolean checks
through every scene build and the job-tile paths, getCollisions per link and pair, disabled links, clearance of poses and
edges, the margin checks, the carve filter and an attached object.  The inputs are geometry_inputs.py's (four scenes, 400
configurations each, directed rows included); test_geometry_reference_cpu.py pins the reference and the non-vacuity of
these inputs without a GPU.

Every verdict is compared outside the reference's 1e-9 m band only, and every test asserts that at most 1 % of its
cases lie in it.  Rows with an item centre outside the padded grid follow the header's out-of-grid rule: the boolean
verdict must still be right; a distance may only overstate, and must be exact while max_dist + reach <= the pad."""
import ctypes
import json
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import attach_restatement as A
import geometry_inputs as I
import geometry_reference as G
from oracle import octomap_bt
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
_pd = ctypes.POINTER(ctypes.c_double)
FLAGS = [(1, 1), (1, 0), (0, 1)]
MARGINS = [(0.02, 0.0), (0.1, 0.01), (0.0, 0.01)]
DISABLED = ["base_body_link", "shell_base_link_front", "hand_wrist_link"]


@pytest.fixture(scope="module")
def rb():
    return I.robot()


@pytest.fixture(scope="module")
def gp(rb):
    p = GpuPlanner(Robot())
    assert p.robot.link_names == rb.names
    return p


def set_scene(gp, name, how="device"):
    sc = I.scene(name)
    if how == "host":
        gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    elif how == "device":
        gp.set_scene_keys(sc.keys, sc.res)
    else:
        gp.set_scene_bt(octomap_bt.write_bt(sc.keys, sc.res))
    gp.set_disabled_map_links([])
    # every sphere threshold of the model stays below 255 at 5 cm and at 2 cm: the byte field path
    assert gp.scene_device().has_d2b == 1


# ------------------------------------------------------------------------------------------ FK
@pytest.mark.parametrize("name", ["c2", "clutter2"])
def test_probe_fk(gp, rb, model_path, name):
    with open(model_path) as f:
        model = json.load(f)
    bodies = model["bodies"]
    q = np.ascontiguousarray(I.configs(name))
    fr, z = np.zeros((len(q), len(bodies), 12)), np.zeros(len(q))
    L.check(L.lib().smp_probe_fk(gp.h, q.ctypes.data_as(_pd), len(q), fr.ctypes.data_as(_pd), z.ctypes.data_as(_pd)))
    T = rb.frames(q)[:, bodies]
    want = np.concatenate([T[:, :, :3, :3].reshape(len(q), -1, 9), T[:, :, :3, 3]], axis=2)
    err = np.abs(fr - want).max()
    # the chain table: joint pose times frame-to-tip, segment by segment, from the identity
    P = np.tile(np.eye(4), (len(q), 1, 1))
    for seg in model["chain"]:
        J = np.tile(np.eye(4), (len(q), 1, 1))
        ax, org = np.array(seg["axis"], float), np.array(seg["origin"], float)
        if seg["type"] == "RotAxis":
            J[:, :3, :3] = Rotation.from_rotvec(ax[None, :] * q[:, seg["joint"], None]).as_matrix()
            J[:, :3, 3] = org
        elif seg["type"] == "TransAxis":
            J[:, :3, 3] = org[None, :] + ax[None, :] * q[:, seg["joint"], None]
        F = np.eye(4)
        F[:3, :3], F[:3, 3] = np.array(seg["ftip_R"], float).reshape(3, 3), seg["ftip_p"]
        P = P @ J @ F
    assert model["chain"][-1]["name"] == "hand_wrist_link"
    wrist = rb.frames(q)[:, rb.names.index("hand_wrist_link")]
    ez = max(np.abs(z - P[:, 2, 3]).max(), np.abs(z - (wrist[:, 2, 3] - rb.root_z)).max())
    print(name, "largest frame difference", err, "largest eez difference", ez)
    assert err <= 1e-12 and ez <= 1e-12


# ------------------------------------------------------------------------------------------ boolean checks
@pytest.mark.parametrize("how", ["host", "device", "bt"])
@pytest.mark.parametrize("name", I.SCENES)
def test_check_configs(gp, name, how):
    set_scene(gp, name, how)
    q = I.configs(name)
    for flags in FLAGS:
        I.compare_verdicts(gp.check_configs(q, *flags), I.case0(name), flags, what="%s %s %s" % (name, how, flags))


@pytest.mark.parametrize("tile", [-1, -8, 8])
def test_job_tile_shapes(gp, tile):
    set_scene(gp, "c2")
    q = I.configs("c2")
    soa = np.ascontiguousarray(q.T)
    for flags in FLAGS:
        v = np.zeros(len(q), np.uint8)
        L.check(L.lib().smp_probe_check_shape(gp.h, soa.ctypes.data_as(_pd), len(q), flags[0], flags[1], tile, 2048,
                                              v.ctypes.data_as(ctypes.c_void_p)))
        I.compare_verdicts(v, I.case0("c2"), flags, what="tile %d %s" % (tile, flags))


@pytest.mark.parametrize("name", I.SCENES)
def test_get_collisions(gp, rb, name):
    """Per self pair and per map link, each item band-excluded on its own."""
    set_scene(gp, name)
    c = I.case0(name)
    n = 100
    by_link = G.per_group(c.marg[:n], rb.item_link, rb.n_links)
    by_pair = c.self_by_pair()[:n]
    got_l, got_p = np.zeros((n, rb.n_links), bool), np.zeros((n, len(rb.pairs)), bool)
    pair_of = {(rb.names[a], rb.names[b]): k for k, (a, b) in enumerate(rb.pairs)}
    for i in range(n):
        pairs, links = gp.get_collisions(I.configs(name)[i])
        got_l[i, [rb.names.index(l) for l in links]] = True
        got_p[i, [pair_of[p] for p in pairs]] = True
    for got, ref, what in ((got_l, by_link, "links"), (got_p, by_pair, "pairs")):
        band = np.abs(ref) <= G.EPS
        G.band_share(band, "%s %s" % (name, what))
        assert ((got == (ref <= 0)) | band).all(), (name, what)
    assert got_l.any() and got_p.any()


@pytest.mark.parametrize("name", I.SCENES)
def test_disabled_map_links(gp, name):
    """With the shell box off, the cylinders inside its footprint decide rows of their own."""
    set_scene(gp, name)
    q = I.configs(name)
    gp.set_disabled_map_links(DISABLED)
    try:
        got = gp.check_configs(q, False, True)
    finally:
        gp.set_disabled_map_links([])
    c = I.case0(name).with_disabled(DISABLED)
    I.compare_verdicts(got, c, (0, 1), what="%s disabled links" % name)
    changed = int((c.valid(False, True)[0] & ~I.case0(name).valid(False, True)[1]).sum())
    print("configurations the three links alone held invalid:", changed)
    assert changed >= 8


# ------------------------------------------------------------------------------------------ clearance
@pytest.mark.parametrize("name", I.SCENES)
def test_clearance_configs(gp, name):
    set_scene(gp, name)
    for c, D in I.clearance_cases(name):
        I.compare_clearance(name, c, D, gp.clearance(c.q, D), what="%s D=%s rows %d" % (name, D, len(c.q)))


def test_clearance_edges(gp):
    set_scene(gp, I.EDGE_SCENE)
    a, b, M, pts, off = I.edges()
    D = I.D_WIDE[I.EDGE_SCENE]
    ref_map, _ = I.compare_edge_clearance(gp.edge_clearance(a, b, D), D)
    assert (ref_map < D).any() and (ref_map < 0).any()


# ------------------------------------------------------------------------------------------ margins
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("name", I.SCENES)
def test_check_configs_margin(gp, name, margin):
    """Clear = valid and every term beyond its margin; the band lies around the margin.  max margin + reach <= the pad,
    so the rows outside the grid must be exact too."""
    res = I.scene(name).res
    assert max(margin) + I.robot().reach.max() <= I.pad_cells(res) * res
    set_scene(gp, name)
    c = I.case_wide(name)
    got = gp.check_clear(c.q, True, True, margin)
    I.compare_verdicts(got, c, (1, 1), margin, what="%s margin %s" % (name, margin))
    plain = c.valid()[0]
    assert (plain & ~c.valid(True, True, *margin)[1]).sum() >= 1   # the margin takes some valid row away


@pytest.mark.parametrize("margin", MARGINS)
def test_check_edges_margin(gp, margin):
    set_scene(gp, I.EDGE_SCENE)
    a, b, M, pts, off = I.edges()
    first, npts = gp.check_edges(a, b, True, True, margin=margin)
    blocked = I.compare_edge_margin(first, npts, (1, 1), margin, what="edges margin %s" % (margin,))
    assert 0 < blocked < I.N_EDGES


# ------------------------------------------------------------------------------------------ carve
Q_MAP = np.array([0.3, -0.4, 0.7] + scenes.ARM_UNFOLDED)   # the pose the map was taken at
OBJECT = "attached_object"


def _carve_keys(ra):
    """room3 with its floor, plus the robot's own image at Q_MAP: the cells that hold a sphere centre or the centre of a
    primitive, and their neighbours one cell along each axis."""
    sc = I.scene("room3")
    wc, Tp = ra.world(Q_MAP[None])
    pts = np.concatenate([wc[0], Tp[0, :, :3, 3]]) - np.array([0.0, 0.0, ra.z_off])
    k = scenes.coord_to_key(pts, sc.res)
    nb = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    own = (k[:, None, :] + nb[None, :, :]).reshape(-1, 3)
    return np.unique(np.concatenate([sc.keys, own]), axis=0)


@pytest.fixture(scope="module")
def bar(rb):
    centres, radii = A.bar(10)
    return rb.attached(A.HAND, centres, radii), Robot().attach(A.HAND, centres, radii)


@pytest.fixture
def gp_bar(gp, bar):
    """The module's planner with the bar attached for the length of one test."""
    base = gp.robot
    set_scene(gp, "room3")
    gp.set_robot(bar[1])
    yield gp
    gp.set_carve(None)
    gp.set_robot(base)


# The bar hangs on hand_palm_link, which has no collision geometry of its own (and smp_carve_keys rejects a link
# without any), so "hand_palm_link plus the attached bar" is the selection (OBJECT,).
@pytest.mark.parametrize("links", [None, (OBJECT,)])
@pytest.mark.parametrize("pad", [0.0, 0.05])
def test_carve_keys(gp_bar, rb, bar, pad, links):
    """A key is carved iff some item of the selected links is within pad of its box; the band lies around pad."""
    ra, gp = bar[0], gp_bar
    assert A.HAND not in [rb.names[l] for l in rb.collision_links]
    keys = _carve_keys(ra)
    cells = G.Cells(keys, 0.05, ra.z_off)
    assert np.array_equal(cells.keys, keys)
    sel = None if links is None else [ra.names.index(l) for l in links]
    dist, marg = G.cell_terms(ra, cells, Q_MAP, pad + 0.01, sel)
    # contact is the verdict margin's; a positive pad asks for the distance
    lo, hi = (marg <= -G.EPS, marg <= G.EPS) if pad == 0 else (dist <= pad - G.EPS, dist <= pad + G.EPS)
    band = lo != hi
    G.band_share(band, "carve pad %s links %s" % (pad, links))
    got = gp.carve_keys(keys, 0.05, Q_MAP, pad, links).astype(bool)
    print("carved", int(got.sum()), "of", len(keys))
    assert ((got == lo) | band).all()
    assert 0 < lo.sum() < len(keys)


def test_sticky_carve(gp_bar, bar):
    """set_carve, then a device build: the carve pose is map-valid, and the checks equal the reference on the key list
    without the reference's carved keys."""
    ra, gp = bar[0], gp_bar
    keys = _carve_keys(ra)
    cells = G.Cells(keys, 0.05, ra.z_off)
    dist, marg = G.cell_terms(ra, cells, Q_MAP, 0.06)
    pad = 0.05
    lo, hi = dist <= pad - G.EPS, dist <= pad + G.EPS
    assert not (lo != hi).any() and lo.any()
    q = np.concatenate([Q_MAP[None], I.configs("room3")[:150]])
    before = G.Case(ra, cells, q, 0.0)
    assert not before.valid(False, True)[1][0]   # the robot stands in its own image
    gp.set_carve(Q_MAP, pad)
    try:
        gp.set_scene_keys(keys, 0.05)
        got = gp.check_configs(q, False, True)
    finally:
        gp.set_carve(None)
    assert gp.last_carve()["n_carved"] == int(lo.sum())
    after = G.Case(ra, G.Cells(keys[~lo], 0.05, ra.z_off), q, 0.0)
    I.compare_verdicts(got, after, (0, 1), what="sticky carve")
    assert got[0] == 1
    assert (after.valid(False, True)[0] & ~before.valid(False, True)[1]).sum() >= 1


# ------------------------------------------------------------------------------------------ attached objects
def test_attached_bar(gp, rb, bar):
    """The bar as 10 spheres: 66 items, two per lane.  Checks and clearance with it, then without it again."""
    ra, robot = bar
    assert ra.n_sph + ra.n_prim == 66 and robot.link_names == ra.names
    set_scene(gp, "c2")
    base = gp.robot
    q = I.configs("c2")
    D = 0.1
    with_bar0 = G.Case(ra, I.cells("c2"), q, 0.0)
    with_bar = G.Case(ra, I.cells("c2"), q[:I.N_CLEAR["c2"]], D)
    gp.set_robot(robot)
    try:
        for flags in FLAGS:
            I.compare_verdicts(gp.check_configs(q, *flags), with_bar0, flags, what="bar %s" % (flags,))
        I.compare_clearance("c2", with_bar, D, gp.clearance(with_bar.q, D), what="bar D=%s" % D)
    finally:
        gp.set_robot(base)
    c = I.case_wide("c2")
    I.compare_verdicts(gp.check_configs(q), I.case0("c2"), what="bar detached")
    I.compare_clearance("c2", c, D, gp.clearance(c.q, D), what="bar detached D=%s" % D)
    assert (I.case0("c2").valid()[0] & ~with_bar0.valid()[1]).sum() >= 8   # the bar decides some rows


@pytest.mark.parametrize("name", ["c2", "clutter2"])
def test_largest_attached_sphere(gp, rb, name):
    """One sphere of radius 0.45, the largest admitted: the boolean verdict must be right for every row, the bases up
    to 1.5 m outside the occupied box and at x = 100 m included -- the pad's guarantee.  At 2 cm its threshold passes
    255, so the byte field is dropped and the kernels take the wide field."""
    touch = [n for n in rb.names if n.startswith(("arm_link", "hand_"))]
    centre, radius = [(0.0, 0.0, 0.5)], [0.45]
    ra = rb.attached(A.HAND, centre, radius, touch_links=[t for t in touch if rb.names.index(t) in rb.collision_links])
    robot = Robot().attach(A.HAND, centre, radius, touch_links=[t for t in touch
                                                               if rb.names.index(t) in rb.collision_links])
    set_scene(gp, name)
    base = gp.robot
    q = I.configs(name)
    c = G.Case(ra, I.cells(name), q, 0.0)
    gp.set_robot(robot)
    try:
        assert gp.scene_device().has_d2b == (1 if name == "c2" else 0)
        for flags in [(0, 1), (1, 1)]:
            I.compare_verdicts(gp.check_configs(q, *flags), c, flags, what="%s sphere 0.45 %s" % (name, flags))
    finally:
        gp.set_robot(base)
    assert gp.scene_device().has_d2b == 1
    s = ra.n_sph - 1
    alone = (c.marg[:, s] <= 0) & ~(np.delete(c.marg, s, axis=1) <= 0).any(1)
    print(name, "rows the large sphere alone puts into the map:", int(alone.sum()))
    assert alone.sum() >= 8


# ------------------------------------------------------------------------------------------ the out-of-grid rule
@pytest.fixture(scope="module")
def beyond_pad(gp, rb):
    """One voxel at x in [0.5, 0.55] (the grid spans x in [-0.05, 1.10]), the base at x = -0.06 with the arm folded,
    max_dist 0.5: the head is 0.33 m from the voxel (test_geometry_reference_cpu.py pins that), but its centre column
    lies outside the grid.  Returns (the call's record, the reference's map)."""
    keys = np.array([[32768 + 10, 32768, 32768 + 18]])
    q = np.array([[-0.06, 0.0, 0.0] + scenes.ARM_FOLDED])
    ref = G.Case(rb, G.Cells(keys, 0.05, rb.z_off), q, 0.5).clearance()[0][0]
    gp.set_scene_keys(keys, 0.05)
    gp.set_disabled_map_links([])
    got = gp.clearance(q, 0.5)[0]
    print("map", got["map"], "reference", ref)
    return got, ref


def test_clearance_beyond_the_pad_never_understates(beyond_pad):
    got, ref = beyond_pad
    assert got["map"] >= ref - I.TOL


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="out-of-grid rule: an item whose centre cell lies outside the padded grid gives max_dist, "
                          "so a clearance with max_dist + reach > pad may overstate (0.3913, kinect, against 0.33)")
def test_clearance_beyond_the_pad_is_exact(beyond_pad):
    got, ref = beyond_pad
    assert abs(got["map"] - ref) <= I.TOL
