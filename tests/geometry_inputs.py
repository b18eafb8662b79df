"""The input sets of test_geometry_reference_cpu.py and test_gpu_geometry_reference.py: four scenes as octomap keys and
at most 400 configurations each -- random rows over the bounds and the joint ranges +- 0.3 rad, and directed rows where
the geometry degenerates or the grid ends.  Nothing here computes an expected answer."""
import functools
import math
import os

import numpy as np

import geometry_reference as G
from squirrel_motion_planner_amd import scenes

SCENES = ("c2", "c4", "room3", "clutter2")
N_CONFIGS = 400
PAD_M = 0.45   # the largest admitted item reach: the grid is padded by ceil(PAD_M / res) + 2 cells


def pad_cells(res):
    return int(math.ceil(PAD_M / res)) + 2


@functools.lru_cache(maxsize=None)
def robot():
    return G.Robot()


def _clutter2(seed=21, res=0.02):
    """A 2 x 2 x 1 m room at 2 cm: walls, about 3000 random clutter points in a few clusters, a floor."""
    rng = np.random.default_rng(seed)
    n_cl = 7
    ctr = np.column_stack([rng.uniform(-0.9, 0.9, n_cl), rng.uniform(-0.9, 0.9, n_cl), rng.uniform(0.45, 0.95, n_cl)])
    size = rng.uniform(0.05, 0.25, (n_cl, 3))
    idx = rng.integers(0, n_cl, 3000)
    pts = ctr[idx] + rng.uniform(-0.5, 0.5, (3000, 3)) * size[idx]
    pts = pts[(np.abs(pts[:, :2]) < 1.0).all(1) & (pts[:, 2] > 0.0) & (pts[:, 2] < 1.0)]
    keys = np.concatenate([scenes.coord_to_key(pts, res), scenes._walls(1.0, 1.0, 1.0, res),
                           scenes.floor_keys([0.0, 0.0], res, 1.5)])
    sc = scenes.Scene("clutter-2cm", keys, res, [0.0, 0.0, 0.0] + scenes.ARM_FOLDED,
                      [0.3, 0.3, 1.0] + scenes.ARM_UNFOLDED, (0, 0), (0, 0))
    sc.env_x, sc.env_y = sc.bounds()
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene description (keys with the floor the tests insert, res, env bounds, start, goal)."""
    if name == "c2":
        return scenes.box_room()
    if name == "c4":
        return scenes.narrow_passage()
    if name == "room3":
        f = np.load(os.path.join(G.ROOT, "tests", "golden", "room3_keys.npz"))
        keys = np.concatenate([f["keys"].astype(np.int64), scenes.floor_keys([0.0, 0.0], 0.05, 3.0)])
        sc = scenes.Scene(name, keys, 0.05, [0, 0, 0] + scenes.ARM_FOLDED, [1, 1, 0] + scenes.ARM_UNFOLDED, (0, 0), (0, 0))
        sc.env_x, sc.env_y = sc.bounds()
        return sc
    if name == "clutter2":
        return _clutter2()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cells(name):
    sc = scene(name)
    return G.Cells(sc.keys, sc.res, robot().z_off)


def grid_bounds(name, keys=None):
    """(lo, hi) in metres of the padded grid: the key bounding box plus pad_cells(res) cells, z offset included."""
    sc = scene(name)
    k = sc.keys if keys is None else np.asarray(keys, np.int64).reshape(-1, 3)
    pad = pad_cells(sc.res)
    off = np.array([0.0, 0.0, robot().z_off])
    return (k.min(0) - pad - G.KEY0) * sc.res + off, (k.max(0) + pad + 1 - G.KEY0) * sc.res + off


SEED = {"c2": 31, "c4": 32, "room3": 33, "clutter2": 34}

# Poses with one primitive nearest to an obstacle (x, y, yaw; folded arm), found by a scan of the reference over a
# coarse base grid (step 0.25 m, or 0.2 m in the 2 cm room; 8 yaw values): per scene the shell box, the neck and head
# cylinders, the kinect box, the scanner cylinder and the 1 mm marker box (the committed model holds one).
NEAREST = {
    "c2": [(-1.45, -0.7, 2.4562), (1.8, 2.3, 0.1), (-2.7, 1.3, 2.4562), (-2.7, 2.05, 0.1), (0.8, 2.3, 1.6708), (-3.45, 0.8, 5.5978)],
    "c4": [(-0.05, -4.8, 0.8854), (-4.55, 4.7, 0.1), (-0.05, -4.8, 0.1), (-4.55, 4.7, 0.1), (-0.05, -4.8, 0.1), (-0.3, -4.55, 1.6708)],
    "room3": [(-2.2, 4.05, 2.4562), (-2.45, 4.05, 2.4562), (-2.2, 4.05, 2.4562), (-2.45, 4.05, 2.4562), (1.8, 3.3, 4.8124), (-2.7, 1.05, 5.5978)],
    "clutter2": [(-0.2, -0.6, 0.8854), (-0.4, -0.6, 0.1), (0.6, 1.0, 5.5978), (0.4, -0.0, 0.1), (-1.2, 1.0, 0.8854), (-0.6, -0.6, 5.5978)],
}


def random_rows(sc, n, rng):
    q0, q1 = joint_ranges()
    (x0, x1), (y0, y1) = sc.env_x, sc.env_y
    return np.column_stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)] +
                           [rng.uniform(q0[j] - 0.3, q1[j] + 0.3, n) for j in range(2, 8)])


@functools.lru_cache(maxsize=None)
def joint_ranges():
    import json
    with open(G.MODEL_JSON) as f:
        m = json.load(f)
    return np.array(m["q_min"], float), np.array(m["q_max"], float)


@functools.lru_cache(maxsize=None)
def directed(name):
    """The directed rows of a scene."""
    sc = scene(name)
    rng = np.random.default_rng(SEED[name] + 1000)
    (x0, x1), (y0, y1) = sc.env_x, sc.env_y
    rows = []
    # base yaw where the box's axis terms degenerate, and far outside one turn
    yaws = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, math.pi / 4, 3 * math.pi / 4, 1e3, -1e3]
    r = random_rows(sc, 2 * len(yaws), rng)
    r[:, 2] = yaws + yaws
    r[len(yaws):, 3:] = scenes.ARM_FOLDED
    # keep the degenerate yaws off the walls, so that the box decides near an obstacle rather than inside one
    r[:, 0] = np.clip(r[:, 0], x0 + 0.6, x1 - 0.6)
    r[:, 1] = np.clip(r[:, 1], y0 + 0.6, y1 - 0.6)
    rows.append(r)
    # bases within one cell of a wall's inner face, on both sides of it
    res = sc.res
    t = 0.1   # wall thickness of scenes._walls
    for xw, yw in [(x0 + t, None), (x1 - t, None), (None, y0 + t), (None, y1 - t)]:
        for sgn in (-1.0, 1.0):
            q = random_rows(sc, 1, rng)[0]
            q[3:] = scenes.ARM_FOLDED
            d = sgn * rng.uniform(0.0, res)
            if xw is not None:
                q[0] = xw + d
            else:
                q[1] = yw + d
            rows.append(q[None, :])
    rows.append(np.array([sc.start, sc.goal], float))
    # outside the occupied bounding box by up to 1.5 m, on every side and at the corners; one base at x = 100 m
    for dx, dy in [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1), (-1, 1), (1, -1)]:
        for k in range(2):
            q = random_rows(sc, 1, rng)[0]
            if k:
                q[3:] = scenes.ARM_FOLDED
            u = rng.uniform(0.0, 1.5)
            if dx:
                q[0] = (x0 - u) if dx < 0 else (x1 + u)
            if dy:
                q[1] = (y0 - u) if dy < 0 else (y1 + u)
            rows.append(q[None, :])
    far = random_rows(sc, 1, rng)[0]
    far[0], far[3:] = 100.0, scenes.ARM_FOLDED
    rows.append(far[None, :])
    near = np.array([list(p) + scenes.ARM_FOLDED for p in NEAREST.get(name, [])], float).reshape(-1, 8)
    rows.append(near)
    # the head (radius 0.23) reaching 5 and 15 mm into the low-x wall, the folded arm turned along the wall: with the
    # shell box's link disabled the cylinder is the only item in contact
    for k, yaw in enumerate([1.2, 1.6, 2.0, 2.4] * 2):
        rows.append(np.array([[x0 + t + (0.225 if k < 4 else 0.215), 0.5 * (y0 + y1) + 0.37 + 0.11 * k, yaw]
                              + scenes.ARM_FOLDED]))
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def configs(name):
    """The 400 configurations of a scene: the directed rows first, random rows after them."""
    d = directed(name)
    rng = np.random.default_rng(SEED[name])
    q = np.concatenate([d, random_rows(scene(name), N_CONFIGS - len(d), rng)])
    assert q.shape == (N_CONFIGS, 8)
    q.setflags(write=False)
    return q


def inside_grid(name, q, rb=None, keys=None):
    """Per configuration: does every item's centre cell lie inside the padded grid (spheres: the cell; primitives:
    the column)?"""
    rb = rb or robot()
    lo, hi = grid_bounds(name, keys)
    wc, Tp = rb.world(q)
    s_in = ((wc >= lo) & (wc < hi)).all(axis=(1, 2))
    pc = Tp[:, :, :2, 3]
    p_in = ((pc >= lo[:2]) & (pc < hi[:2])).all(axis=(1, 2))
    return s_in & p_in


# ------------------------------------------------------------------------------------------ the reference's answers
# One evaluation per scene and process, shared by every test that needs it.
D_WIDE = {"c2": 0.3, "c4": 0.3, "room3": 0.3, "clutter2": 0.3}   # the reference is exact below this distance
# configurations of the distance comparisons: every directed row (59) and the random rows after them; at 2 cm a
# configuration costs the reference about ten times what it costs at 5 cm
N_CLEAR = {"c2": 200, "c4": 200, "room3": 200, "clutter2": 80}
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def case0(name):
    """All 400 configurations, exact around contact (the boolean verdicts)."""
    return G.Case(robot(), cells(name), configs(name), 0.0)


@functools.lru_cache(maxsize=None)
def case_wide(name):
    """The first N_CLEAR configurations (every directed row and some random ones), exact below D_WIDE."""
    return G.Case(robot(), cells(name), configs(name)[:N_CLEAR[name]], D_WIDE[name])


def clearance_cases(name):
    """(reference case, max_dist) of the clearance comparisons: 0.1 and 0.3 on every scene."""
    return [(case_wide(name), d) for d in (0.1, 0.3)]


def compare_verdicts(got, case, flags=(1, 1), margin=(0.0, 0.0), what=""):
    """got: 1 valid / clear per configuration; equal to the reference outside the band."""
    lo, hi, band = case.valid(bool(flags[0]), bool(flags[1]), *margin)
    got = np.asarray(got).astype(bool)
    G.band_share(band, what)
    bad = np.flatnonzero((got != lo) & ~band)
    assert len(bad) == 0, "%s: verdicts differ at rows %s" % (what, bad[:10])
    return band


def compare_clearance(name, case, D, got, rb=None, inside=None, with_map=True, with_self=True, what=""):
    """got: a structured array with map, self, map_link, self_a, self_b.  Values within 1e-9 wherever the reference is
    below D, witnesses attain the reference's minimum within 1e-9; rows with an item centre outside the padded grid
    follow the out-of-grid rule (never below the reference; equal while D + reach <= pad).  Returns the largest
    differences (map, self)."""
    rb = rb or case.rb
    res = scene(name).res
    assert D <= case.D + 1e-12
    ref_map = np.minimum(case.map_dist().min(1), D)
    ref_self = case.self.min(1)
    if inside is None:
        inside = inside_grid(name, case.q, rb)
    exact = inside | (D + rb.reach.max() <= pad_cells(res) * res)
    dm = ds = 0.0
    if with_map:
        diff = got["map"] - ref_map
        assert (diff >= -TOL).all(), "%s: map below the reference at rows %s" % (what, np.flatnonzero(diff < -TOL)[:10])
        bad = np.flatnonzero(exact & (np.abs(diff) > TOL))
        assert len(bad) == 0, "%s: map differs at rows %s: %s vs %s" % (what, bad[:10], got["map"][bad[:10]],
                                                                        ref_map[bad[:10]])
        dm = float(np.abs(diff[exact]).max()) if exact.any() else 0.0
        by_link = case.map_by_link()
        rows = np.flatnonzero(exact & (ref_map < D - TOL))
        assert (got["map_link"][rows] >= 0).all(), what
        w = by_link[rows, got["map_link"][rows]]
        assert (w <= ref_map[rows] + TOL).all(), "%s: a map witness link does not attain the minimum" % what
        capped = np.flatnonzero(exact & (ref_map >= D + TOL))
        assert (got["map_link"][capped] == -1).all() and (got["map"][capped] == D).all(), what
    if with_self:
        diff = got["self"] - ref_self
        assert (np.abs(diff) <= TOL).all(), "%s: self differs at rows %s" % (what, np.flatnonzero(np.abs(diff) > TOL)[:10])
        ds = float(np.abs(diff).max())
        pair_of = {p: k for k, p in enumerate(rb.pairs)}
        k = np.array([pair_of[(int(a), int(b))] for a, b in zip(got["self_a"], got["self_b"])])
        w = case.self_by_pair()[np.arange(len(k)), k]
        assert (w <= ref_self + TOL).all(), "%s: a self witness pair does not attain the minimum" % what
    print("%s: largest difference map %.3g self %.3g; rows outside the grid %d" % (what, dm, ds, int((~inside).sum())))
    return dm, ds


# ------------------------------------------------------------------------------------------ edges
EDGE_SCENE = "room3"
N_EDGES = 40


@functools.lru_cache(maxsize=None)
def edges():
    """40 short edges of the room3 scene: random rows and a nearby second end, so that each has one or two hops of the
    density rule.  Returns (a, b, M, points, offsets) with the points of shortcut_restatement's density rule."""
    import shortcut_restatement as R
    q = configs(EDGE_SCENE)
    a = q[N_CONFIGS - N_EDGES:].copy()
    rng = np.random.default_rng(77)
    b = a + np.concatenate([rng.normal(0.0, 0.25, (N_EDGES, 2)), rng.normal(0.0, 0.3, (N_EDGES, 6))], axis=1)
    rev = np.array([0, 0, 1, 1, 1, 1, 1, 1])
    _, M = R.density(a, b, rev, R.N_SEG, R.STEP)
    pts, off = R.all_points(a, b, M)
    return a, b, M, pts, off


@functools.lru_cache(maxsize=None)
def edge_case():
    return G.Case(robot(), cells(EDGE_SCENE), edges()[3], D_WIDE[EDGE_SCENE])


def compare_edge_clearance(got, D, what="edges"):
    """got: smp_clearance_edges' records.  map / self are the reference's minima over the edge's points, the point
    fields name points that attain them within 1e-9."""
    a, b, M, pts, off = edges()
    c = edge_case()
    ref_map = np.minimum(c.map_dist().min(1), D)
    ref_self = c.self.min(1)
    inside = inside_grid(EDGE_SCENE, pts)
    dm = ds = 0.0
    for e in range(N_EDGES):
        s = slice(off[e], off[e + 1])
        assert got["n_points"][e] == M[e] + 1
        m, sf = ref_map[s].min(), ref_self[s].min()
        assert got["map"][e] >= m - TOL and abs(got["self"][e] - sf) <= TOL, (what, e)
        ds = max(ds, abs(got["self"][e] - sf))
        assert abs(ref_self[s][got["self_point"][e]] - sf) <= TOL, (what, e)
        if inside[s].all():
            assert abs(got["map"][e] - m) <= TOL, (what, e, got["map"][e], m)
            dm = max(dm, abs(got["map"][e] - m))
            if m < D - TOL:
                assert got["map_point"][e] >= 0 and abs(ref_map[s][got["map_point"][e]] - m) <= TOL, (what, e)
            elif m >= D + TOL:
                assert got["map_point"][e] == -1, (what, e)
    print("%s: largest difference map %.3g self %.3g" % (what, dm, ds))
    return ref_map, ref_self


def compare_edge_margin(first, n_points, flags, margin, what="edges"):
    """first: smp_check_edges_margin's first point that is not clear (-1: none)."""
    a, b, M, pts, off = edges()
    lo, hi, _ = edge_case().valid(bool(flags[0]), bool(flags[1]), *margin)
    band = np.zeros(N_EDGES, bool)
    blocked = 0
    for e in range(N_EDGES):
        s = slice(off[e], off[e + 1])
        assert n_points[e] == M[e] + 1
        f = [int(np.flatnonzero(~v[s])[0]) if (~v[s]).any() else -1 for v in (lo, hi)]
        band[e] = f[0] != f[1]
        blocked += f[0] >= 0
        assert band[e] or first[e] == f[0], (what, e, first[e], f)
    G.band_share(band, what)
    return blocked
