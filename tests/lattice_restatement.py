"""The far-goal stage restated (include/smp_gpu.h "Far goals": smp_base_lattice_fit, smp_base_free_map, smp_base_route,
smp_plan_far), shared by test_lattice_cpu.py, test_gpu_lattice.py and test_shim_far.py.

Node configurations with the header's operations (integer to double, product, sum; numpy and Python floats round every
operation on its own), expected bits from the CPU oracle's check_configs(q, self_=False, map_=True) -- with a margin
from margin_restatement.py's predicate --, a heapq Dijkstra with the header's priority and neighbour order, the merge of
straight runs, the handover loop and the stitch of smp_plan_far.  Nothing here runs code of the library."""
import collections
import functools
import heapq
import math

import numpy as np

import margin_restatement as G
import shortcut_restatement as R
from squirrel_motion_planner_amd import scenes

OK, ERR_ARG, ERR_START_INVALID, ERR_GOAL_INVALID, ERR_NO_SOLUTION = 0, -1, -2, -3, -4
ARM = tuple(scenes.ARM_FOLDED)

Lattice = collections.namedtuple("Lattice", "x0 y0 pitch nx ny theta0 dtheta n_theta wrap_theta arm")


def fit(env_x, env_y, pitch, n_theta, theta0=0.0, arm=ARM):
    nx = int(math.floor((env_x[1] - env_x[0]) / pitch)) + 1
    ny = int(math.floor((env_y[1] - env_y[0]) / pitch)) + 1
    return Lattice(float(env_x[0]), float(env_y[0]), float(pitch), nx, ny, float(theta0), (2.0 * math.pi) / n_theta,
                   int(n_theta), 1, tuple(arm))


def n_nodes(lat):
    return lat.nx * lat.ny * lat.n_theta


def node_config(lat, ix, iy, t):
    return [lat.x0 + float(ix) * lat.pitch, lat.y0 + float(iy) * lat.pitch, lat.theta0 + float(t) * lat.dtheta] + \
        [float(a) for a in lat.arm]


def node_configs(lat):
    """(N, 8): node n = (t * ny + iy) * nx + ix."""
    n = np.arange(n_nodes(lat), dtype=np.int64)
    ix, iy, t = n % lat.nx, (n // lat.nx) % lat.ny, n // (lat.nx * lat.ny)
    q = np.empty((len(n), 8))
    q[:, 0] = lat.x0 + ix.astype(np.float64) * lat.pitch
    q[:, 1] = lat.y0 + iy.astype(np.float64) * lat.pitch
    q[:, 2] = lat.theta0 + t.astype(np.float64) * lat.dtheta
    q[:, 3:] = np.asarray(lat.arm, np.float64)[None, :]
    return q


def pack(free):
    """The words of smp_base_free_map: bit n % 32 of word n / 32, the unused bits of the last word 0."""
    f = np.asarray(free, bool).reshape(-1)
    f = np.concatenate([f, np.zeros(-len(f) % 32, bool)])
    return np.packbits(f, bitorder="little").view(np.uint32)


@functools.lru_cache(maxsize=None)
def expected_free(name, lat, mm=0.0, disabled=None):
    """free (n_theta, ny, nx) bool of the lattice in scene `name`: the oracle's map check of every node (disabled: a
    link name left out of it), or the margin predicate at (mm, 0) with the self part off."""
    q = node_configs(lat)
    if mm > 0:
        assert disabled is None
        ok = G.oracle(name, mm, 0.0).check_configs(q, False, True)
    else:
        en = None
        if disabled is not None:
            rb = R.orobot()
            en = np.ones(rb.n_links, np.uint8)
            en[rb.link_names.index(disabled)] = 0
        ok = R.oracle_for(name, en).check_configs(q, False, True)
    return ok.astype(bool).reshape(lat.n_theta, lat.ny, lat.nx)


# The disabled-link case: with the arm folded inside the base's footprint clearance_restatement.DISABLED_LINK (arm_link2)
# decides no node of C2's lattice; the hand's base link, the arm's far end, decides five.
DISABLED_LINK = "hand_base_link"


# ------------------------------------------------------------------------------------------ the route
def _round_index(v):
    f = math.floor(v + 0.5) if math.isfinite(v) else float("nan")
    if not math.isfinite(f) or f < -2147483648.0 or f > 2147483647.0:
        return None
    return int(f)


def snap(lat, free, p, snap_cells, blocked):
    """(status, (ix, iy, t) or None)."""
    if not all(math.isfinite(float(v)) for v in p[:3]):
        return ERR_ARG, None
    ix = _round_index((float(p[0]) - lat.x0) / lat.pitch)
    iy = _round_index((float(p[1]) - lat.y0) / lat.pitch)
    d = float(p[2]) - lat.theta0
    t = _round_index(d / lat.dtheta if lat.dtheta != 0 else (float("nan") if d == 0 else math.copysign(float("inf"), d)))
    if ix is None or iy is None or t is None:
        return ERR_ARG, None
    if lat.wrap_theta:
        t %= lat.n_theta
    if not (0 <= ix < lat.nx and 0 <= iy < lat.ny and 0 <= t < lat.n_theta):
        return ERR_ARG, None
    if free[t, iy, ix]:
        return OK, (ix, iy, t)
    for r in range(1, min(snap_cells, max(lat.nx, lat.ny)) + 1):
        best = None
        for y in range(max(iy - r, 0), min(iy + r, lat.ny - 1) + 1):
            for x in range(max(ix - r, 0), min(ix + r, lat.nx - 1) + 1):
                if max(abs(x - ix), abs(y - iy)) != r or not free[t, y, x]:
                    continue
                key = ((x - ix) ** 2 + (y - iy) ** 2, (t * lat.ny + y) * lat.nx + x)
                if best is None or key < best[0]:
                    best = (key, (x, y, t))
        if best is not None:
            return OK, best[1]
    return blocked, None


def route(lat, free, frm, to, snap_cells=2, full=False):
    """smp_base_route restated: dict of status, from_node, to_node, chain (n_chain, 3), rows (n_out, 8), cost, n_settled.
    full=True settles every reachable node instead of stopping at to_node (`reached`: their number)."""
    free = np.asarray(free, bool).reshape(lat.n_theta, lat.ny, lat.nx)
    out = dict(status=OK, from_node=None, to_node=None, chain=None, rows=None, cost=0.0, n_settled=0, reached=0)
    st, a = snap(lat, free, frm, snap_cells, ERR_START_INVALID)
    if st != OK:
        out["status"] = st
        return out
    out["from_node"] = a
    st, b = snap(lat, free, to, snap_cells, ERR_GOAL_INVALID)
    if st != OK:
        out["status"] = st
        return out
    out["to_node"] = b
    nx, ny, nt = lat.nx, lat.ny, lat.n_theta
    node = lambda x, y, t: (t * ny + y) * nx + x
    ok = lambda x, y, t: 0 <= x < nx and 0 <= y < ny and bool(free[t, y, x])
    w_axis = lat.pitch
    w_diag = math.sqrt(lat.pitch * lat.pitch + lat.pitch * lat.pitch)
    w_turn = math.fabs(lat.dtheta)
    src, dst = node(*a), node(*b)
    dp = {src: 0.0}
    parent, settled = {}, set()
    heap = [(0.0, src)]
    found = False
    while heap:
        _, u = heapq.heappop(heap)
        if u in settled:
            continue
        settled.add(u)
        if u == dst:
            found = True
            if not full:
                break
        t, rem = divmod(u, nx * ny)
        y, x = divmod(rem, nx)
        du = dp[u]
        nbrs = [(x + dx, y + dy, t, w_axis) for dx, dy in ((0, -1), (-1, 0), (1, 0), (0, 1)) if ok(x + dx, y + dy, t)]
        nbrs += [(x + dx, y + dy, t, w_diag) for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1))
                 if ok(x + dx, y + dy, t) and ok(x + dx, y, t) and ok(x, y + dy, t)]
        for s in (-1, 1):
            tt = (t + s) % nt if lat.wrap_theta else t + s
            if 0 <= tt < nt and ok(x, y, tt):
                nbrs.append((x, y, tt, w_turn))
        for vx, vy, vt, w in nbrs:
            v = node(vx, vy, vt)
            c = du + w
            if c < dp.get(v, float("inf")):
                dp[v], parent[v] = c, u
                heapq.heappush(heap, (c, v))
    out["n_settled"] = len(settled)
    out["reached"] = len(settled)
    if not found:
        out["status"] = ERR_NO_SOLUTION
        return out
    chain = []
    v = dst
    while True:
        t, rem = divmod(v, nx * ny)
        y, x = divmod(rem, nx)
        chain.append((x, y, t))
        if v == src:
            break
        v = parent[v]
    chain.reverse()
    out.update(chain=np.array(chain, np.int32).reshape(-1, 3), rows=merged_rows(lat, chain), cost=dp[dst])
    return out


def merged_rows(lat, chain):
    """The chain with runs of equal step merged: a node is kept where the step changes, plus both ends."""
    chain = [tuple(int(v) for v in c) for c in chain]
    step = lambda a, b: (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    rows = []
    for i, c in enumerate(chain):
        if 0 < i < len(chain) - 1 and step(chain[i - 1], c) == step(c, chain[i + 1]):
            continue
        rows.append(node_config(lat, *c))
    return np.array(rows, np.float64).reshape(-1, 8)


def handover(lat, chain, distance):
    """The pop-back loop: the index j of the chain node the 8-DoF planner takes over at."""
    diag = math.sqrt(lat.pitch * lat.pitch + lat.pitch * lat.pitch)
    acc, j = 0.0, len(chain) - 1
    while j > 0 and acc < distance:
        a, b = chain[j], chain[j - 1]
        moved = int(a[0] != b[0]) + int(a[1] != b[1])
        acc += diag if moved == 2 else (lat.pitch if moved == 1 else 0.0)
        j -= 1
    return j


def route_rows(lat, start, chain, j):
    """The rows smp_plan_far hands to the dense check: the query's start, then the merged rows of c_0 .. c_j."""
    return np.concatenate([np.asarray(start, np.float64).reshape(1, 8), merged_rows(lat, chain[:j + 1])])


def stitch(route, tail):
    """out->waypoints: the checked route rows, then the tail plan's rows without its first (the joint row)."""
    return np.concatenate([np.asarray(route, np.float64).reshape(-1, 8), np.asarray(tail, np.float64).reshape(-1, 8)[1:]])


# ------------------------------------------------------------------------------------------ shared inputs
PITCH = 0.2
MARGIN = 0.1   # margin_restatement.POSE_MARGINS[0]'s map part
FAR_START = tuple([-3.0, -3.0, 0.0] + list(ARM))


FAR_OPTS = dict(pitch=0.1, n_theta=8)      # the plan_far cases: smp_far_opts_default's lattice
COARSE_OPTS = dict(pitch=PITCH, n_theta=8)  # ... and one whose route turns in place through a blocked heading
FAR_BUDGET = dict(iterations=300, seed=7)  # shortcut_restatement.SHORTCUT_PLANS' C2 budget
STAGE3_NODE = (86, 64, 0)                  # free with the arm folded; ARM_UNFOLDED there reaches into a box


@functools.lru_cache(maxsize=None)
def far_case(start=FAR_START, pitch=FAR_OPTS["pitch"]):
    """C2's far query from `start` restated up to the dense check: (lattice, free map, route, handover index j, the rows
    handed to the dense check)."""
    sc, _ = R.scene("c2")
    lat = fit(sc.env_x, sc.env_y, pitch, FAR_OPTS["n_theta"])
    free = expected_free("c2", lat)
    r = route(lat, free, start[:3], sc.goal[:3], 2)
    assert r["status"] == OK
    j = handover(lat, r["chain"], 2.0)
    return lat, free, r, j, route_rows(lat, start, r["chain"], j)


def stage3_start():
    """An unfolded start on a node that is free with the arm folded: its first edge (folding the arm) collides."""
    lat = fit(*R.scene("c2")[0].bounds(), FAR_OPTS["pitch"], FAR_OPTS["n_theta"])
    return tuple(node_config(lat, *STAGE3_NODE)[:3] + list(scenes.ARM_UNFOLDED))


@functools.lru_cache(maxsize=None)
def scene_lattice(name, n_theta=4, pitch=PITCH):
    """The lattice over the scene's own bounds."""
    sc, _ = R.scene(name)
    return fit(sc.env_x, sc.env_y, pitch, n_theta)


def sub_lattice(lat, ix0, iy0, nx, ny, t0=0, n_theta=1):
    """A window of a lattice as a lattice of its own: the origin moved by whole steps (formed as the nodes are)."""
    return lat._replace(x0=lat.x0 + float(ix0) * lat.pitch, y0=lat.y0 + float(iy0) * lat.pitch, nx=nx, ny=ny,
                        theta0=lat.theta0 + float(t0) * lat.dtheta, n_theta=n_theta, wrap_theta=0)


# Small lattices of the GPU test: windows of C2's lattice that straddle an obstacle's rim, so both answers occur.
# (name, lattice) by node count; the 3-heading one has nx = 11: tiles straddle rows and layers.
@functools.lru_cache(maxsize=None)
def small_lattices():
    base = scene_lattice("c2", 4)
    out = {}
    for n, (nx, ny, nt) in {1: (1, 1, 1), 31: (31, 1, 1), 32: (8, 4, 1), 33: (11, 3, 1), 97: (97, 1, 1)}.items():
        # (the single node is a free one, so its word is 1 and the 31 unused bits show; the row of 97 is at half pitch)
        out[n] = sub_lattice(base, 7 if n == 1 else 3, 14, nx, ny, 0, nt)._replace(pitch=base.pitch if n != 97 else 0.1)
    out["3x"] = sub_lattice(base, 3, 10, 11, 7, 0, 3)._replace(dtheta=base.dtheta)
    return out
