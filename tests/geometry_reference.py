"""An independent geometric reference for the collision, clearance, margin and carve answers of this library.

Everything here is written from geometry in plain numpy / scipy and builds on data only: the `links`, `spheres`, `prims`,
`root_z`, `octree_z_offset` and `self_pairs` tables of the committed model JSON, the SRDF (to cross-check the pair
list), and octomap keys with a resolution.  It imports neither the CPU oracle nor any restatement, reads none of the
product's derived tables (`bodies`, `body_chain`, `cb`, `ab`, `rxy`, `link_bounds`) and knows no grid: a map cell is the
box its key names, nothing else.

  frames     one 4x4 homogeneous matrix per link by tree recursion (scipy rotations)
  items      sphere centres; primitives as full 3-D oriented boxes / cylinders on their link frames (their axis is
             asserted vertical at every pose evaluated, so "upright" is checked, not assumed)
  map        candidate cells by a KD-tree ball query of radius reach + distance + res * sqrt(3) (for a primitive, less
             the cells that the axis-aligned box around it already puts too far); then every candidate:
             sphere: point-to-box distance - r (negative inside); box: z gap combined with the distance of two convex
             polygons (0 when they overlap, else the least vertex-edge distance), and the signed 15-axis separating-axis
             margin for the verdict; cylinder: disk-rectangle distance combined with the z gap
  self       sphere-sphere, sphere-box (centre brought into the box frame by R^T), sphere-cylinder
  verdicts   every decision twice, at distance <= -EPS and at <= +EPS (EPS = 1e-9 m); a case on which the two differ is
             "in the band" and is left out of a comparison -- the only exclusion, capped at 1 % by the tests
"""
import json
import os
import re

import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_JSON = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")
SRDF = os.path.join(ROOT, "tests", "golden", "robotino_plan.srdf")
EPS = 1e-9
BAND_CAP = 0.01
KEY0 = 32768
INF = float("inf")
UPRIGHT_TOL = 1e-12


# ------------------------------------------------------------------------------------------ robot
class Robot:
    """The data tables of the model, and optionally one attached object (a new link fixed to `link`, identity frame,
    covered by spheres)."""

    def __init__(self, path=MODEL_JSON):
        with open(path) as f:
            m = json.load(f)
        L = m["links"]
        self.names = [e["name"] for e in L]
        self.parent = [int(e["parent"]) for e in L]
        self.type = [e["type"] for e in L]
        self.joint = [int(e["joint"]) for e in L]
        self.axis = np.array([e["axis"] for e in L], float)
        self.origin = np.array([e["origin"] for e in L], float)
        self.R = np.array([e["R"] for e in L], float).reshape(-1, 3, 3)
        self.p = np.array([e["p"] for e in L], float)
        self.root_z = float(m["root_z"])
        self.z_off = float(m["octree_z_offset"])
        self.sph_link = np.array([s["link"] for s in m["spheres"]], int)
        self.sph_c = np.array([s["c"] for s in m["spheres"]], float).reshape(-1, 3)
        self.sph_r = np.array([s["r"] for s in m["spheres"]], float)
        self.prim_link = np.array([p["link"] for p in m["prims"]], int)
        self.prim_box = np.array([p["type"] == "box" for p in m["prims"]], bool)
        # box: three half extents; cylinder: [radius, half length]
        self.prim_half = np.array([p["half"] for p in m["prims"]], float).reshape(-1, 3)
        self.pairs = [(int(a), int(b)) for a, b in m["self_pairs"]]
        assert all(p < i for i, p in enumerate(self.parent)), "parents precede their children"
        self._index()

    def _index(self):
        self.n_links, self.n_sph, self.n_prim = len(self.names), len(self.sph_r), len(self.prim_link)
        self.item_link = np.concatenate([self.sph_link, self.prim_link])
        self.reach = np.concatenate([self.sph_r, np.where(self.prim_box, np.linalg.norm(self.prim_half, axis=1),
                                                          np.hypot(self.prim_half[:, 0], self.prim_half[:, 1]))])
        self.collision_links = sorted(set(self.item_link.tolist()))
        link_prim = {int(l): k for k, l in enumerate(self.prim_link)}
        ss, sp = [], []   # (sphere a, sphere b, pair index), (primitive, sphere, pair index)
        for k, (a, b) in enumerate(self.pairs):
            assert not (a in link_prim and b in link_prim), "two primitives in one pair: none of the model's"
            if a in link_prim or b in link_prim:
                p, sl = (link_prim[a], b) if a in link_prim else (link_prim[b], a)
                sp += [(p, s, k) for s in np.flatnonzero(self.sph_link == sl)]
            else:
                ss += [(sa, sb, k) for sa in np.flatnonzero(self.sph_link == a)
                       for sb in np.flatnonzero(self.sph_link == b)]
        self.ss = np.array(ss, int).reshape(-1, 3)
        self.sp = np.array(sp, int).reshape(-1, 3)
        self.self_pair = np.concatenate([self.ss[:, 2], self.sp[:, 2]])   # pair index of every self term

    def attached(self, link, centres, radii, name="attached_object", touch_links=()):
        """A copy with the object attached: a link `name` on `link` (identity frame), its spheres, and one self pair
        with every collision link that moves against it and is no touch link."""
        import copy
        r = copy.copy(self)
        par = self.names.index(link)
        new = self.n_links
        r.names = self.names + [name]
        r.parent, r.type, r.joint = self.parent + [par], self.type + ["None"], self.joint + [-1]
        r.axis, r.origin = np.vstack([self.axis, np.zeros(3)]), np.vstack([self.origin, np.zeros(3)])
        r.R, r.p = np.concatenate([self.R, np.eye(3)[None]]), np.vstack([self.p, np.zeros(3)])
        c = np.asarray(centres, float).reshape(-1, 3)
        r.sph_link = np.concatenate([self.sph_link, np.full(len(c), new)])
        r.sph_c, r.sph_r = np.vstack([self.sph_c, c]), np.concatenate([self.sph_r, np.asarray(radii, float)])
        r.n_links = new + 1
        touch = {self.names.index(t) for t in touch_links}
        rigid = r.rigid_with(new)
        r.pairs = sorted(self.pairs + [(l, new) for l in self.collision_links if l not in rigid and l not in touch])
        r._index()
        return r

    # -------------------------------------------------------------------------------------- frames
    def frames(self, q):
        """(n, n_links, 4, 4) link frames of the configurations q (n, 8)."""
        q = np.asarray(q, float).reshape(-1, 8)
        n = len(q)
        T = np.zeros((n, self.n_links, 4, 4))
        for i in range(self.n_links):
            J = np.tile(np.eye(4), (n, 1, 1))
            if self.parent[i] < 0:
                J[:, 2, 3] = self.root_z
                T[:, i] = J
                continue
            if self.type[i] == "RotAxis":
                J[:, :3, :3] = Rotation.from_rotvec(self.axis[i][None, :] * q[:, self.joint[i], None]).as_matrix()
                J[:, :3, 3] = self.origin[i]
            elif self.type[i] == "TransAxis":
                J[:, :3, 3] = self.origin[i][None, :] + self.axis[i][None, :] * q[:, self.joint[i], None]
            else:
                J[:, :3, :3], J[:, :3, 3] = self.R[i], self.p[i]
            T[:, i] = T[:, self.parent[i]] @ J
        return T

    def rigid_with(self, link, seed=0):
        """Links whose transform relative to `link` is the same at three random configurations."""
        q = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, 8))
        T = self.frames(q)
        rel = np.linalg.inv(T[:, link])[:, None] @ T
        return {l for l in range(self.n_links) if np.abs(rel[:, l] - rel[0, l]).max() < 1e-9}

    def world(self, q):
        """Sphere centres (n, S, 3) and primitive frames (n, P, 4, 4); asserts every primitive's axis vertical."""
        T = self.frames(q)
        Ts = T[:, self.sph_link]
        wc = np.einsum("nsij,sj->nsi", Ts[:, :, :3, :3], self.sph_c) + Ts[:, :, :3, 3]
        Tp = T[:, self.prim_link]
        if self.n_prim and len(Tp):
            ez = np.array([0.0, 0.0, 1.0])
            tilt = max(np.abs(Tp[:, :, :3, 2] - ez).max(), np.abs(Tp[:, :, 2, :3] - ez).max())
            assert tilt <= UPRIGHT_TOL, "a primitive's axis leaves the vertical by %g" % tilt
        return wc, Tp

    def derived_pairs(self, srdf=SRDF, seed=1):
        """The self pair list re-derived: all pairs of collision links, minus the SRDF's disable_collisions pairs,
        minus the rigid pairs.  Returns (pairs, number of SRDF-enabled pairs, number of rigid ones among them)."""
        text = open(srdf).read()
        off = set()
        for tag in re.findall(r"<disable_collisions\b[^>]*>", text):
            a, b = re.search(r'link1="([^"]+)"', tag).group(1), re.search(r'link2="([^"]+)"', tag).group(1)
            off.add(frozenset((a, b)))
        cl = self.collision_links
        enabled = [(a, b) for i, a in enumerate(cl) for b in cl[i + 1:]
                   if frozenset((self.names[a], self.names[b])) not in off]
        rigid = {a: self.rigid_with(a, seed) for a in cl}
        kept = [(a, b) for a, b in enabled if b not in rigid[a]]
        return kept, len(enabled), len(enabled) - len(kept)


# ------------------------------------------------------------------------------------------ distances
def point_box(c, lo, hi):
    """Distance of points c to the boxes [lo, hi] (0 inside); all (N, 3)."""
    return np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0), axis=1)


def _cross2(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def point_segment(p, a, b):
    """Distance of points p to the segments a-b; broadcastable (..., 2)."""
    ab, ap = b - a, p - a
    t = np.clip((ap * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(ap - t[..., None] * ab, axis=-1)


def polygon_distance(A, B):
    """Distance of two convex polygons given counter-clockwise, A (N, na, 2) and B (N, nb, 2): 0 when they are not
    separated (a vertex of one inside the other, or two edges crossing), else the least vertex-to-edge distance."""
    A2, B2 = np.roll(A, -1, axis=1), np.roll(B, -1, axis=1)

    def inside(P, Q, Q2):  # any vertex of P inside the closed polygon Q
        c = _cross2((Q2 - Q)[:, None, :, :], P[:, :, None, :] - Q[:, None, :, :])
        return (c >= 0).all(axis=2).any(axis=1)

    a, b, c, d = A[:, :, None, :], A2[:, :, None, :], B[:, None, :, :], B2[:, None, :, :]
    o1, o2 = _cross2(b - a, c - a), _cross2(b - a, d - a)
    o3, o4 = _cross2(d - c, a - c), _cross2(d - c, b - c)
    crossing = ((o1 * o2 < 0) & (o3 * o4 < 0)).any(axis=(1, 2))
    overlap = inside(A, B, B2) | inside(B, A, A2) | crossing
    dmin = np.minimum(point_segment(A[:, :, None, :], B[:, None, :, :], B2[:, None, :, :]).min(axis=(1, 2)),
                      point_segment(B[:, :, None, :], A[:, None, :, :], A2[:, None, :, :]).min(axis=(1, 2)))
    return np.where(overlap, 0.0, dmin)


def sat_margin(ca, Ra, ha, cb, hb, Rb=None):
    """Signed 15-axis separating-axis margin of oriented boxes (centres (N, 3), axes as the columns of (N, 3, 3), half
    extents (N, 3)): the largest gap along a unit axis; > 0 separated, < 0 overlapping by that depth."""
    N = len(ca)
    if Rb is None:
        Rb = np.tile(np.eye(3), (N, 1, 1))
    t = cb - ca
    axes = [Ra[:, :, i] for i in range(3)] + [Rb[:, :, j] for j in range(3)]
    axes += [np.cross(Ra[:, :, i], Rb[:, :, j]) for i in range(3) for j in range(3)]
    best = np.full(N, -INF)
    for L in axes:
        ln = np.linalg.norm(L, axis=1)
        ok = ln > 1e-9   # parallel edges: the face axes already cover that direction
        Lu = L / np.where(ok, ln, 1.0)[:, None]
        ra = (np.abs(np.einsum("nij,ni->nj", Ra, Lu)) * ha).sum(1)
        rb = (np.abs(np.einsum("nij,ni->nj", Rb, Lu)) * hb).sum(1)
        gap = np.abs((t * Lu).sum(1)) - ra - rb
        best = np.where(ok, np.maximum(best, gap), best)
    return best


def _combine(mxy, mz):
    """Signed margin of two products (a planar shape times a z interval) from the signed planar and z margins."""
    return np.where((mxy < 0) & (mz < 0), np.maximum(mxy, mz), np.hypot(np.maximum(mxy, 0.0), np.maximum(mz, 0.0)))


def box_cell(T, half, lo, hi):
    """(distance >= 0, signed margin) of upright oriented boxes (frames T (N, 4, 4), half (N, 3)) to the cells."""
    c, R = T[:, :3, 3], T[:, :3, :3]
    zg = np.maximum(np.maximum(lo[:, 2] - (c[:, 2] + half[:, 2]), (c[:, 2] - half[:, 2]) - hi[:, 2]), 0.0)
    ux, uy = R[:, :2, 0] * half[:, 0:1], R[:, :2, 1] * half[:, 1:2]
    flip = np.where(_cross2(ux, uy) < 0, -1.0, 1.0)[:, None]   # keep the rectangle counter-clockwise
    uy = uy * flip
    A = np.stack([c[:, :2] - ux - uy, c[:, :2] + ux - uy, c[:, :2] + ux + uy, c[:, :2] - ux + uy], axis=1)
    B = np.stack([lo[:, :2], np.stack([hi[:, 0], lo[:, 1]], 1), hi[:, :2], np.stack([lo[:, 0], hi[:, 1]], 1)], axis=1)
    d = np.hypot(polygon_distance(A, B), zg)
    # the vertical is one of the 15 axes: a clear z gap is a separation already, the other 14 axes are tried without one
    m = zg.copy()
    k = zg <= 1e-6
    m[k] = sat_margin(c[k], R[k], half[k], 0.5 * (lo[k] + hi[k]), 0.5 * (hi[k] - lo[k]))
    return d, m


def cylinder_cell(T, rad, hl, lo, hi):
    """(distance >= 0, signed margin) of upright cylinders (axis: the frame's z) to the cells."""
    c = T[:, :3, 3]
    g = np.maximum(lo[:, :2] - c[:, :2], c[:, :2] - hi[:, :2])   # signed per axis: < 0 inside the slab
    out = np.linalg.norm(np.maximum(g, 0.0), axis=1)
    mxy = np.where((g < 0).all(1), g.max(1), out) - rad
    mz = np.maximum(lo[:, 2] - (c[:, 2] + hl), (c[:, 2] - hl) - hi[:, 2])
    d = np.hypot(np.maximum(out - rad, 0.0), np.maximum(mz, 0.0))
    return d, _combine(mxy, mz)


def sphere_box(c, T, half):
    """Distance of sphere centres c (..., 3) to solid oriented boxes (frames T (..., 4, 4))."""
    loc = np.einsum("...ji,...j->...i", T[..., :3, :3], c - T[..., :3, 3])
    return np.linalg.norm(np.maximum(np.abs(loc) - half, 0.0), axis=-1)


def sphere_cylinder(c, T, rad, hl):
    loc = np.einsum("...ji,...j->...i", T[..., :3, :3], c - T[..., :3, 3])
    return np.hypot(np.maximum(np.hypot(loc[..., 0], loc[..., 1]) - rad, 0.0), np.maximum(np.abs(loc[..., 2]) - hl, 0.0))


# ------------------------------------------------------------------------------------------ map
class Cells:
    """The occupied cells of a key list: lo = (key - 32768) * res with the octree's z offset, hi = lo + res."""

    def __init__(self, keys, res, z_off):
        self.keys = np.unique(np.asarray(keys, np.int64).reshape(-1, 3), axis=0)
        self.res = float(res)
        self.lo = (self.keys - KEY0).astype(float) * self.res
        self.lo[:, 2] += z_off
        self.hi = self.lo + self.res
        self.tree = cKDTree(0.5 * (self.lo + self.hi)) if len(self.keys) else None

    def candidates(self, centres, radius):
        """(query index, cell index) of every cell whose centre is within radius + res * sqrt(3) of the query."""
        if self.tree is None or len(centres) == 0:
            return np.zeros(0, int), np.zeros(0, int)
        got = self.tree.query_ball_point(centres, radius + self.res * np.sqrt(3.0), return_sorted=False)
        cnt = np.fromiter((len(g) for g in got), int, len(got))
        if cnt.sum() == 0:
            return np.zeros(0, int), np.zeros(0, int)
        return np.repeat(np.arange(len(got)), cnt), np.concatenate([np.asarray(g, int) for g in got if len(g)])


def _map_pairs(rb, cells, q, D, budget=1500000, links=None, item_min=False):
    """Yields (flat index conf * (S + P) + item, cell index, distance, verdict margin) of every culled (item, cell)
    pair, in chunks of whole configurations that keep the candidate count bounded.  links: item filter by link.
    item_min: the caller wants each item's minimum only, so a primitive's cells that cannot attain it are dropped: the
    distance to a cell is at least the gap of the axis-aligned box around the primitive, and the item's minimum is at
    most the distance of the primitive to any one cell's centre."""
    n, S, P = len(q), rb.n_sph, rb.n_prim
    wc, Tp = rb.world(q)
    # half extents of a box around each primitive in its own frame (cylinder: radius, radius, half length)
    hull = np.where(rb.prim_box[:, None], rb.prim_half, rb.prim_half[:, [0, 0, 1]])
    ctr = np.concatenate([wc, Tp[:, :, :3, 3]], axis=1).reshape(-1, 3)
    rad = np.tile(rb.reach + D, n)
    cnt = cells.tree.query_ball_point(ctr, rad + cells.res * np.sqrt(3.0), return_length=True)
    if links is not None:
        cnt = cnt * np.tile(np.isin(rb.item_link, links), n)
    per = cnt.reshape(n, S + P).sum(1)
    start = 0
    while start < n:
        stop, tot = start + 1, per[start]
        while stop < n and tot + per[stop] <= budget:
            tot += per[stop]
            stop += 1
        sl = slice(start * (S + P), stop * (S + P))
        start = stop
        live = np.flatnonzero(cnt[sl] > 0) + sl.start
        qi, ci = cells.candidates(ctr[live], rad[live])
        flat = live[qi]
        item = flat % (S + P)
        conf = flat // (S + P)
        # primitives: drop the cells that the axis-aligned box around the primitive already puts beyond D
        k = np.flatnonzero(item >= S)
        Tk = Tp[conf[k], item[k] - S]
        e = np.einsum("nij,nj->ni", np.abs(Tk[:, :3, :3]), hull[item[k] - S])
        gap = np.maximum(np.maximum(cells.lo[ci[k]] - (Tk[:, :3, 3] + e), (Tk[:, :3, 3] - e) - cells.hi[ci[k]]), 0.0)
        low = np.linalg.norm(gap, axis=1)
        keep = np.ones(len(flat), bool)
        keep[k] = low <= D + 1e-6
        if item_min and len(k):
            mid = 0.5 * (cells.lo[ci[k]] + cells.hi[ci[k]])
            hk = rb.prim_half[item[k] - S]
            up = np.where(rb.prim_box[item[k] - S], sphere_box(mid, Tk, hk), sphere_cylinder(mid, Tk, hk[:, 0], hk[:, 1]))
            best = np.full(n * (S + P), INF)
            _min_into(best, flat[k], up)
            keep[k] &= low <= best[flat[k]] + 1e-6
        flat, item, conf, ci = flat[keep], item[keep], conf[keep], ci[keep]
        lo, hi = cells.lo[ci], cells.hi[ci]
        d, m = np.empty(len(flat)), np.empty(len(flat))
        s = item < S
        d[s] = point_box(wc[conf[s], item[s]], lo[s], hi[s]) - rb.sph_r[item[s]]
        m[s] = d[s]
        for p in range(P):
            k = item == S + p
            if not k.any():
                continue
            if rb.prim_box[p]:
                d[k], m[k] = box_cell(Tp[conf[k], p], np.tile(rb.prim_half[p], (k.sum(), 1)), lo[k], hi[k])
            else:
                d[k], m[k] = cylinder_cell(Tp[conf[k], p], rb.prim_half[p, 0], rb.prim_half[p, 1], lo[k], hi[k])
        yield flat, ci, d, m


def _min_into(out, idx, val):
    """out[i] = min(out[i], val[idx == i]) for every i."""
    if len(idx):
        order = np.argsort(idx, kind="stable")
        i, v = idx[order], val[order]
        first = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])
        out[i[first]] = np.minimum(out[i[first]], np.minimum.reduceat(v, first))


def map_terms(rb, cells, q, D=0.0):
    """Per configuration and item (spheres, then primitives): (dist, margin), each (n, S + P).  dist is the distance to
    the nearest culled cell (spheres: signed, negative = penetration; primitives: >= 0), margin the signed separation
    the verdicts use (spheres: dist; boxes: the 15-axis margin; cylinders: the signed disk / z margin).  Both are exact
    below D and +inf or larger than D beyond."""
    q = np.asarray(q, float).reshape(-1, 8)
    n, S, P = len(q), rb.n_sph, rb.n_prim
    dist, marg = np.full((n, S + P), INF), np.full((n, S + P), INF)
    if n == 0 or cells.tree is None:
        return dist, marg
    for flat, ci, d, m in _map_pairs(rb, cells, q, D, item_min=True):
        _min_into(dist.reshape(-1), flat, d)
        _min_into(marg.reshape(-1), flat, m)
    return dist, marg


def cell_terms(rb, cells, q, D, links=None):
    """Per cell of `cells`: (dist, margin) to the nearest item of the robot at the one configuration q (items of
    `links` only, link indices; None: all); exact below D."""
    dist, marg = np.full(len(cells.keys), INF), np.full(len(cells.keys), INF)
    if cells.tree is None:
        return dist, marg
    for flat, ci, d, m in _map_pairs(rb, cells, np.asarray(q, float).reshape(1, 8), D, links=links):
        _min_into(dist, ci, d)
        _min_into(marg, ci, m)
    return dist, marg


def self_terms(rb, q):
    """(n, K) signed distance of every self term (sphere pairs, then primitive-sphere pairs); rb.self_pair maps the
    columns to the indices of rb.pairs."""
    q = np.asarray(q, float).reshape(-1, 8)
    wc, Tp = rb.world(q)
    a, b = rb.ss[:, 0], rb.ss[:, 1]
    ds = np.linalg.norm(wc[:, a] - wc[:, b], axis=2) - (rb.sph_r[a] + rb.sph_r[b])[None, :]
    p, s = rb.sp[:, 0], rb.sp[:, 1]
    h = rb.prim_half[p]
    dp = np.where(rb.prim_box[p][None, :], sphere_box(wc[:, s], Tp[:, p], h[None, :, :]),
                  sphere_cylinder(wc[:, s], Tp[:, p], h[None, :, 0], h[None, :, 1])) - rb.sph_r[s][None, :]
    return np.concatenate([ds, dp], axis=1)


# ------------------------------------------------------------------------------------------ verdicts with a band
def hit(margin, thr=0.0):
    """(hit at thr - EPS, hit at thr + EPS): `hit` is margin <= threshold, taken over the last axis."""
    m = np.min(margin, axis=-1) if np.ndim(margin) else margin
    return m <= thr - EPS, m <= thr + EPS


def per_group(values, group, n_groups):
    """Minimum of values (n, K) over the columns of each group: (n, n_groups), +inf for an empty group."""
    out = np.full((len(values), n_groups), INF)
    for g in range(n_groups):
        k = group == g
        if k.any():
            out[:, g] = values[:, k].min(1)
    return out


class Case:
    """Everything the reference knows about a batch of configurations in one scene, computed once."""

    def __init__(self, rb, cells, q, D=0.0, disabled=()):
        self.rb, self.cells, self.q, self.D = rb, cells, np.asarray(q, float).reshape(-1, 8), float(D)
        self.dist, self.marg = map_terms(rb, cells, self.q, D)
        self.off = np.isin(rb.item_link, [rb.names.index(l) for l in disabled])
        self.self = self_terms(rb, self.q)
        # the two methods agree on contact: the distance is positive exactly where the verdict margin is
        near = np.isfinite(self.marg) & (np.abs(self.marg) > EPS)
        assert ((self.dist > 0) == (self.marg > 0))[near].all(), "distance and separating-axis margin disagree in sign"

    def with_disabled(self, disabled):
        """The same evaluation with the map items of the links `disabled` left out."""
        import copy
        c = copy.copy(self)
        c.off = np.isin(self.rb.item_link, [self.rb.names.index(l) for l in disabled])
        return c

    def map_margin(self):
        return np.where(self.off[None, :], INF, self.marg)

    def map_dist(self):
        return np.where(self.off[None, :], INF, self.dist)

    def valid(self, with_self=True, with_map=True, mm=0.0, ms=0.0):
        """(valid at the strict end, valid at the lenient end, in band) per configuration; with margins: "clear"."""
        n = len(self.q)
        h_lo, h_hi = np.zeros(n, bool), np.zeros(n, bool)
        if with_map:
            # the verdict margin decides contact; a positive margin asks for the distance
            a, b = hit(self.map_margin())
            if mm > 0:
                c, d = hit(self.map_dist(), mm)
                a, b = a | c, b | d
            h_lo, h_hi = h_lo | a, h_hi | b
        if with_self:
            a, b = hit(self.self, ms)
            h_lo, h_hi = h_lo | a, h_hi | b
        return ~h_hi, ~h_lo, h_lo != h_hi

    def clearance(self):
        """map (capped at D) and self minima per configuration."""
        mp = np.minimum(self.map_dist().min(1), self.D)
        return mp, self.self.min(1)

    def map_by_link(self):
        return per_group(self.map_dist(), self.rb.item_link, self.rb.n_links)

    def self_by_pair(self):
        return per_group(self.self, self.rb.self_pair, len(self.rb.pairs))


def band_share(band, what=""):
    share = float(np.mean(band)) if np.size(band) else 0.0
    print("band share %s: %d of %d (%.4f)" % (what, int(np.sum(band)), np.size(band), share))
    assert share <= BAND_CAP, "more than 1 %% of the cases of %s lie within 1e-9 m of a boundary" % what
    return share
