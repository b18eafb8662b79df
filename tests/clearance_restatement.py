"""Numpy restatement of the clearance queries (include/smp_gpu.h: smp_clearance_configs, smp_clearance_edges), shared by
test_clearance_cpu.py, test_gpu_clearance.py and test_shim_clearance.py.

It follows the wording of the header term by term, over the local cell window of each item.  It builds only on
oracle.Oracle.body_fk (the body frames), OracleRobot (the model) and OracleScene (the occupancy grid); the density rule
and the points of an edge are shortcut_restatement.py's.  numpy evaluates every operation on its own, so no product and
sum are ever contracted, and np.sqrt is correctly rounded.

An item is skipped without a sweep when scipy's Euclidean distance transform of the grid proves its term above D
(`gap`: the box-to-box gap, in cells, from a cell to the nearest occupied cell bounds the distance from any point of the
cell to any occupied box from below); `prefilter=False` sweeps every item, and test_clearance_cpu.py checks both
agree."""
import functools

import numpy as np

import shortcut_restatement as R

INF = float("inf")
CLEARANCE_DTYPE = np.dtype([("map", np.float64), ("self", np.float64), ("map_link", np.int32), ("self_a", np.int32),
                            ("self_b", np.int32), ("kind", np.int8), ("self_kind", np.int8)])
EDGE_FIELDS = ("map", "self", "map_point", "self_point", "map_link", "self_a", "self_b", "n_points")
# kind of the map witness (the restatement's own bookkeeping, for the tests' non-vacuity conditions)
NONE, SPHERE, PRIM = 0, 1, 2


def _gapv(c, lo, hi):
    return np.where(c < lo, lo - c, np.where(c > hi, c - hi, 0.0))


class Model:
    """The flat self pair lists of the oracle's robot model, by link pair."""

    def __init__(self, rb):
        self.rb = rb
        link_prim = np.full(rb.n_links, -1)
        for p in range(rb.n_prim):
            link_prim[rb.prim_link[p]] = p
        link_sph = [[] for _ in range(rb.n_links)]
        for s in range(rb.n_sph):
            link_sph[rb.sph_link[s]].append(s)
        sp, pp = [], []
        for a, b in zip(rb.pair_a, rb.pair_b):
            a, b = int(a), int(b)
            lo, hi = min(a, b), max(a, b)
            if link_prim[a] >= 0 or link_prim[b] >= 0:
                p, sl = (link_prim[a], b) if link_prim[a] >= 0 else (link_prim[b], a)
                pp += [(p, s, lo, hi) for s in link_sph[sl]]
            else:
                sp += [(sa, sb, lo, hi) for sa in link_sph[a] for sb in link_sph[b]]
        self.sp = np.array(sp, np.int64).reshape(-1, 4)
        self.pp = np.array(pp, np.int64).reshape(-1, 4)
        self.sph_cb = rb.sph_cb.reshape(-1, 3)
        self.prim_cb = rb.prim_cb.reshape(-1, 3)
        self.prim_ab = rb.prim_ab.reshape(-1, 3)
        self.prim_h = rb.prim_h.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def model():
    return Model(R.orobot())


_CUSTOM = {}


def register_scene(name, keys, res):
    """A scene of the tests' own under `name`, beside those of shortcut_restatement.scene."""
    from oracle import oracle as O
    _CUSTOM[name] = O.OracleScene(keys, res)


@functools.lru_cache(maxsize=None)
def fk_oracle():
    from oracle import oracle as O
    return O.Oracle(R.orobot())


@functools.lru_cache(maxsize=None)
def grid(name):
    """(OracleScene, box-to-box gap in cells per cell) of a registered scene or one of shortcut_restatement.scene."""
    from scipy.ndimage import binary_dilation, distance_transform_edt
    osc = _CUSTOM[name] if name in _CUSTOM else R.scene(name)[1]
    if osc.occ.any():
        gap = distance_transform_edt(~binary_dilation(osc.occ, structure=np.ones((3, 3, 3), bool)))
    else:
        gap = np.full(osc.occ.shape, 1e30)
    return osc, gap


def world(orc, q):
    """Sphere centres (n, S, 3) and primitive centres / x axes (n, P, 5) from the oracle's body frames, as the checker
    forms them (KDL Frame * Vector: the three-term sum, then the translation)."""
    m = model()
    rb = m.rb
    q = np.asarray(q, np.float64).reshape(-1, 8)
    B = orc.body_fk(q)  # (n, n_body, 12): R row-major, then p
    Bs = B[:, rb.sph_body, :]
    cb = m.sph_cb[None, :, :]
    wc = np.stack([(Bs[:, :, 3 * r] * cb[:, :, 0] + Bs[:, :, 3 * r + 1] * cb[:, :, 1] + Bs[:, :, 3 * r + 2] * cb[:, :, 2])
                   + Bs[:, :, 9 + r] for r in range(3)], axis=2)
    P = rb.n_prim
    pw = np.zeros((len(q), P, 5))
    if P:
        Bp = B[:, rb.prim_body[:P], :]
        pc, ab = m.prim_cb[None, :P, :], m.prim_ab[None, :P, :]
        for r in range(3):
            pw[:, :, r] = (Bp[:, :, 3 * r] * pc[:, :, 0] + Bp[:, :, 3 * r + 1] * pc[:, :, 1]
                           + Bp[:, :, 3 * r + 2] * pc[:, :, 2]) + Bp[:, :, 9 + r]
        pw[:, :, 3] = Bp[:, :, 0] * ab[:, :, 0] + Bp[:, :, 1] * ab[:, :, 1] + Bp[:, :, 2] * ab[:, :, 2]
        pw[:, :, 4] = Bp[:, :, 3] * ab[:, :, 0] + Bp[:, :, 4] * ab[:, :, 1] + Bp[:, :, 5] * ab[:, :, 2]
    return wc, pw


def _window(osc, lo, hi):
    """Occupied cells (i, j, k as float64 arrays) of the window lo..hi (world coordinates), a cell of margin, clipped."""
    o = (osc.ox, osc.oy, osc.oz)
    n = (osc.nx, osc.ny, osc.nz)
    a = [max(int(np.floor((lo[d] - o[d]) / osc.res)) - 1, 0) for d in range(3)]
    b = [min(int(np.floor((hi[d] - o[d]) / osc.res)) + 1, n[d] - 1) for d in range(3)]
    if a[0] > b[0] or a[1] > b[1] or a[2] > b[2]:
        z = np.zeros(0)
        return z, z, z
    kk, jj, ii = np.nonzero(osc.occ[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1])
    return (ii + a[0]).astype(np.float64), (jj + a[1]).astype(np.float64), (kk + a[2]).astype(np.float64)


def sphere_term(osc, c, r, D):
    """min(D, min over the occupied cells within reach of dist(c, cell) - r)."""
    i, j, k = _window(osc, c - (r + D), c + (r + D))
    if len(i) == 0:
        return D
    res = osc.res
    gx = _gapv(c[0], osc.ox + i * res, osc.ox + (i + 1.0) * res)
    gy = _gapv(c[1], osc.oy + j * res, osc.oy + (j + 1.0) * res)
    gz = _gapv(c[2], osc.oz + k * res, osc.oz + (k + 1.0) * res)
    d = np.sqrt(gx * gx + gy * gy + gz * gz) - r
    return min(D, float(d.min()))


def prim_term(osc, ty, h, pw, D):
    """min(D, min over the occupied cells within reach of the primitive's distance to the cell's box)."""
    px, py, pz, c, s = (float(v) for v in pw)
    h0, h1, h2 = (float(v) for v in h)
    ac, as_ = abs(c), abs(s)
    ex = ac * h0 + as_ * h1 if ty == 1 else h0
    ey = as_ * h0 + ac * h1 if ty == 1 else h0
    hz = h2 if ty == 1 else h1
    e = np.array([ex, ey, hz])
    ctr = np.array([px, py, pz])
    i, j, k = _window(osc, ctr - e - D, ctr + e + D)
    if len(i) == 0:
        return D
    res = osc.res
    xlo, xhi = osc.ox + i * res, osc.ox + (i + 1.0) * res
    ylo, yhi = osc.oy + j * res, osc.oy + (j + 1.0) * res
    zlo, zhi = osc.oz + k * res, osc.oz + (k + 1.0) * res
    dz = np.maximum(np.maximum(zlo - (pz + hz), (pz - hz) - zhi), 0.0)
    if ty == 2:
        qx, qy = _gapv(px, xlo, xhi), _gapv(py, ylo, yhi)
        dxy = np.maximum(np.sqrt(qx * qx + qy * qy) - h0, 0.0)
        d = np.sqrt(dxy * dxy + dz * dz)
        return min(D, float(d.min()))
    hw = 0.5 * res
    dx, dy = 0.5 * (xlo + xhi) - px, 0.5 * (ylo + yhi) - py
    apart = ((np.abs(dx) > hw + (ac * h0 + as_ * h1)) | (np.abs(dy) > hw + (as_ * h0 + ac * h1))
             | (np.abs(c * dx + s * dy) > h0 + hw * (ac + as_)) | (np.abs(c * dy - s * dx) > h1 + hw * (ac + as_)))
    cands = []
    for X in (xlo, xhi):
        for Y in (ylo, yhi):
            qex, qey = X - px, Y - py
            lx, ly = np.abs(c * qex + s * qey), np.abs(c * qey - s * qex)
            qx, qy = np.maximum(lx - h0, 0.0), np.maximum(ly - h1, 0.0)
            cands.append(qx * qx + qy * qy)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            cx = (px + sx * (c * h0)) - sy * (s * h1)
            cy = (py + sx * (s * h0)) + sy * (c * h1)
            gx, gy = _gapv(cx, xlo, xhi), _gapv(cy, ylo, yhi)
            cands.append(gx * gx + gy * gy)
    dxy2 = np.where(apart, np.minimum.reduce(cands), 0.0)
    d = np.sqrt(dxy2 + dz * dz)
    return min(D, float(d.min()))


def map_terms(name, wc, pw, D, map_enabled=None, prefilter=True):
    """Map term of every item of every pose: (n, S + P) float64; items of disabled links hold D."""
    m = model()
    rb = m.rb
    osc, gap = grid(name)
    n, S, P = len(wc), rb.n_sph, rb.n_prim
    en = np.ones(rb.n_links, bool) if map_enabled is None else np.asarray(map_enabled).astype(bool)
    out = np.full((n, S + P), float(D))
    org = np.array([osc.ox, osc.oy, osc.oz])
    dims = np.array([osc.nx, osc.ny, osc.nz])
    # spheres
    f = np.floor((wc - org) / osc.res)
    inside = ((f >= 0) & (f < dims)).all(axis=2) & en[rb.sph_link][None, :]
    fi = np.where(inside[:, :, None], f, 0).astype(np.int64)
    if prefilter:
        g = gap[fi[:, :, 2], fi[:, :, 1], fi[:, :, 0]] * osc.res
        inside &= ~(g > rb.sph_r[None, :] + D + 1e-6)
    for i, s in zip(*np.nonzero(inside)):
        out[i, s] = sphere_term(osc, wc[i, s], float(rb.sph_r[s]), D)
    # primitives: the ball around the centre that holds the primitive bounds it
    for p in range(P):
        if not en[rb.prim_link[p]]:
            continue
        ty, h = int(rb.prim_type[p]), m.prim_h[p]
        hz = h[2] if ty == 1 else h[1]
        rad = float(np.sqrt(rb.prim_rxy[p] * rb.prim_rxy[p] + hz * hz))
        fp = np.floor((pw[:, p, :3] - org) / osc.res)
        col = (fp[:, 0] >= 0) & (fp[:, 0] < osc.nx) & (fp[:, 1] >= 0) & (fp[:, 1] < osc.ny)
        zin = (fp[:, 2] >= 0) & (fp[:, 2] < osc.nz)
        for i in np.flatnonzero(col):
            if prefilter and zin[i] and gap[int(fp[i, 2]), int(fp[i, 1]), int(fp[i, 0])] * osc.res > rad + D + 1e-6:
                continue
            out[i, S + p] = prim_term(osc, ty, h, pw[i, p], D)
    return out


def self_terms(wc, pw):
    """(values (n, NS + NP), a, b (NS + NP): link indices a < b) of every self pair."""
    m = model()
    rb = m.rb
    ia, ib = m.sp[:, 0], m.sp[:, 1]
    e = wc[:, ia, :] - wc[:, ib, :]
    ex, ey, ez = e[:, :, 0], e[:, :, 1], e[:, :, 2]
    ds = np.sqrt(ex * ex + ey * ey + ez * ez) - (rb.sph_r[ia] + rb.sph_r[ib])[None, :]
    ip, isp = m.pp[:, 0], m.pp[:, 1]
    P = pw[:, ip, :]
    W = wc[:, isp, :]
    h = m.prim_h[ip][None, :, :]
    dx, dy, dz = W[:, :, 0] - P[:, :, 0], W[:, :, 1] - P[:, :, 1], W[:, :, 2] - P[:, :, 2]
    az = np.abs(dz)
    c, s = P[:, :, 3], P[:, :, 4]
    lx, ly = np.abs(c * dx + s * dy), np.abs(c * dy - s * dx)
    qx = np.where(lx > h[:, :, 0], lx - h[:, :, 0], 0.0)
    qy = np.where(ly > h[:, :, 1], ly - h[:, :, 1], 0.0)
    qz = np.where(az > h[:, :, 2], az - h[:, :, 2], 0.0)
    q2_box = qx * qx + qy * qy + qz * qz
    rho = np.sqrt(dx * dx + dy * dy)
    qr = np.where(rho > h[:, :, 0], rho - h[:, :, 0], 0.0)
    qzc = np.where(az > h[:, :, 1], az - h[:, :, 1], 0.0)
    q2_cyl = qr * qr + qzc * qzc
    is_box = (rb.prim_type[ip] == 1)[None, :]
    dp = np.sqrt(np.where(is_box, q2_box, q2_cyl)) - rb.sph_r[isp][None, :]
    return (np.concatenate([ds, dp], axis=1), np.concatenate([m.sp[:, 2], m.pp[:, 2]]),
            np.concatenate([m.sp[:, 3], m.pp[:, 3]]))


def clearance(name, q, D, with_self=True, with_map=True, map_enabled=None, prefilter=True):
    """smp_clearance_configs restated: a structured array (CLEARANCE_DTYPE; kind / self_kind: SPHERE or PRIM witness)."""
    m = model()
    rb = m.rb
    q = np.asarray(q, np.float64).reshape(-1, 8)
    n = len(q)
    out = np.zeros(n, CLEARANCE_DTYPE)
    out["map"], out["map_link"] = D, -1
    out["self"], out["self_a"], out["self_b"] = INF, -1, -1
    if n == 0:
        return out
    wc, pw = world(fk_oracle(), q)
    if with_map:
        t = map_terms(name, wc, pw, D, map_enabled, prefilter)
        links = np.concatenate([rb.sph_link, rb.prim_link[:rb.n_prim]])
        kinds = np.concatenate([np.full(rb.n_sph, SPHERE), np.full(rb.n_prim, PRIM)])
        mn = np.minimum(t.min(axis=1), D)
        for i in range(n):
            if mn[i] < D:
                at = np.flatnonzero(t[i] == mn[i])
                w = at[np.argmin(links[at])]
                out["map"][i], out["map_link"][i] = mn[i], links[w]
                # a link is either spheres or one primitive, so the witness link fixes the kind
                out["kind"][i] = kinds[w]
    if with_self:
        v, a, b = self_terms(wc, pw)
        mn = v.min(axis=1)
        nsp = len(m.sp)
        for i in range(n):
            at = np.flatnonzero(v[i] == mn[i])
            w = at[np.lexsort((b[at], a[at]))[0]]
            out["self"][i], out["self_a"][i], out["self_b"][i] = mn[i], a[w], b[w]
            out["self_kind"][i] = SPHERE if w < nsp else PRIM
    return out


def edge_clearance(name, a, b, D, with_self=True, with_map=True, map_enabled=None, n=R.N_SEG, f=R.STEP):
    """smp_clearance_edges restated: dict of EDGE_FIELDS arrays, and `points` (the total point count)."""
    a = np.asarray(a, np.float64).reshape(-1, 8)
    b = np.asarray(b, np.float64).reshape(-1, 8)
    _, M = R.density(a, b, R.orobot().rev, n, f)
    pts, off = R.all_points(a, b, M)
    c = clearance(name, pts, D, with_self, with_map, map_enabled)
    E = len(a)
    out = {k: np.zeros(E, np.float64 if k in ("map", "self") else np.int32) for k in EDGE_FIELDS}
    for e in range(E):
        ce = c[off[e]:off[e + 1]]
        im, is_ = int(np.argmin(ce["map"])), int(np.argmin(ce["self"]))  # (argmin: the lowest index of the minimum)
        out["map"][e], out["self"][e] = ce["map"][im], ce["self"][is_]
        capped = not ce["map"][im] < D
        out["map_point"][e] = -1 if capped else im
        out["map_link"][e] = -1 if capped else ce["map_link"][im]
        out["self_point"][e] = is_ if with_self else -1
        out["self_a"][e], out["self_b"][e] = ce["self_a"][is_], ce["self_b"][is_]
        out["n_points"][e] = M[e] + 1
    out["points"] = int(off[-1])
    out["M"] = M
    return out


# ------------------------------------------------------------------------------------------ shared inputs
# The inputs of the GPU tests, built once per process; the seeds are chosen on the CPU so that the restatement and the
# oracle alone meet the conditions test_clearance_cpu.py pins.
SCENES = ("c2", "room3")
POSE_SEED = {"c2": 5, "room3": 6}
POOL = 800
# Rows of random_configs(scene, POOL, seed): the first rows as they come, then the next rows whose map witness at
# D = 0.3 is a sphere link in range (the base's primitives are the usual witness: they ride 2 cm above the floor).
POSE_ROWS = {"c2": list(range(91)) + [101, 102, 108, 115, 137, 157],
             "room3": list(range(86)) + [87, 91, 92, 100, 111, 113, 146, 180, 213, 218, 219]}
DISABLED_LINK = "arm_link2"  # the disabled-link cases: an arm link that is the map witness of some C2 poses
N_POSES = 97


@functools.lru_cache(maxsize=None)
def poses(name):
    """The GPU tests' 97 configurations of a scene."""
    q = R.random_configs(R.scene(name)[0], POOL, POSE_SEED[name])[POSE_ROWS[name]]
    assert len(q) == N_POSES
    return q


@functools.lru_cache(maxsize=None)
def expected(name, n, D, with_self=True, with_map=True, disabled=False):
    return clearance(name, poses(name)[:n], D, with_self, with_map, map_enabled_for(disabled))


def map_enabled_for(disabled):
    if not disabled:
        return None
    rb = R.orobot()
    en = np.ones(rb.n_links, np.uint8)
    en[rb.link_names.index(DISABLED_LINK)] = 0
    return en


EDGE_MAX_POINTS_TOTAL = 4000


@functools.lru_cache(maxsize=None)
def edges(name):
    """16 of shortcut_restatement.long_edges: the shortest ones after the longest, so that one edge spans several tiles
    and the total stays within a few thousand points.  Returns (a, b)."""
    a, b = R.long_edges(name)
    _, M = R.density(a, b, R.orobot().rev, R.N_SEG, R.STEP)
    order = np.argsort(M, kind="stable")
    idx = np.sort(np.concatenate([order[:15], order[-1:]]))
    assert int((M[idx] + 1).sum()) <= EDGE_MAX_POINTS_TOTAL
    return a[idx], b[idx]


@functools.lru_cache(maxsize=None)
def edges_expected(name, D=0.3):
    a, b = edges(name)
    return edge_clearance(name, a, b, D)


@functools.lru_cache(maxsize=None)
def path12():
    """The shortcut tests' 12-waypoint C2 path."""
    return R.shortcut_input("c2")
