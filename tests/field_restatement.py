"""The cost field of a base lattice restated (include/smp_gpu.h "Far goals": smp_base_cost_field, smp_base_route_gpu),
shared by test_field_cpu.py and test_gpu_field.py.

A heapq Dijkstra run until its heap is empty with lattice_restatement.route's rules (priority (cost, node number), strict
relaxation, the neighbour order of the header), the schedule-free definitions of the parent and of the settled count that
the device uses, the tile geometry by brute force, and the hand-made maps.  Nothing here runs code of the library; the
tile shape is the Python mirror's constant."""
import functools
import heapq
import math

import numpy as np

import lattice_restatement as T
from squirrel_motion_planner_amd import _lib as L

BX, BY, BT = L.FIELD_TILE
B = BX
INF = float("inf")


def weights(lat):
    return lat.pitch, math.sqrt(lat.pitch * lat.pitch + lat.pitch * lat.pitch), math.fabs(lat.dtheta)


def neighbours(lat, free, x, y, t):
    """(node, weight) of every edge of node (x, y, t), in the header's order."""
    nx, ny, nt = lat.nx, lat.ny, lat.n_theta
    w_axis, w_diag, w_turn = weights(lat)
    ok = lambda a, b, c: 0 <= a < nx and 0 <= b < ny and bool(free[c, b, a])
    node = lambda a, b, c: (c * ny + b) * nx + a
    out = [(node(x + dx, y + dy, t), w_axis) for dx, dy in ((0, -1), (-1, 0), (1, 0), (0, 1)) if ok(x + dx, y + dy, t)]
    out += [(node(x + dx, y + dy, t), w_diag) for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1))
            if ok(x + dx, y + dy, t) and ok(x + dx, y, t) and ok(x, y + dy, t)]
    for s in (-1, 1):
        tt = (t + s) % nt if lat.wrap_theta else t + s
        if 0 <= tt < nt and ok(x, y, tt):
            out.append((node(x, y, tt), w_turn))
    return out


def split(lat, n):
    t, rem = divmod(int(n), lat.nx * lat.ny)
    y, x = divmod(rem, lat.nx)
    return x, y, t


def dijkstra(lat, free, src):
    """The host search from node src = (ix, iy, t) until its heap is empty: cost (N,) float64 with +inf where not
    reached, parent (N,) int32 as the search left it (-1 for the source and unreached nodes), order: the nodes as they
    were settled."""
    free = np.asarray(free, bool).reshape(lat.n_theta, lat.ny, lat.nx)
    n = T.n_nodes(lat)
    cost = np.full(n, INF)
    parent = np.full(n, -1, np.int32)
    s = (src[2] * lat.ny + src[1]) * lat.nx + src[0]
    cost[s] = 0.0
    heap, settled, order = [(0.0, s)], np.zeros(n, bool), []
    while heap:
        _, u = heapq.heappop(heap)
        if settled[u]:
            continue
        settled[u] = True
        order.append(u)
        du = float(cost[u])
        for v, w in neighbours(lat, free, *split(lat, u)):
            c = du + w
            if c < cost[v]:
                cost[v], parent[v] = c, u
                heapq.heappush(heap, (c, v))
    return cost, parent, order


def parent_candidates(lat, free, cost, n):
    """The neighbours u of node n with fl(cost[u] + w) == cost[n], as (cost[u], u)."""
    if not (0.0 < cost[n] < INF):
        return []
    return sorted({(float(cost[u]), u) for u, w in neighbours(lat, free, *split(lat, n)) if float(cost[u]) + w == cost[n]})


def parent_rule(lat, free, cost):
    """parent[n] from the field alone: -1 for the source and +inf nodes, else the candidate with the least (cost, u)."""
    free = np.asarray(free, bool).reshape(lat.n_theta, lat.ny, lat.nx)
    out = np.full(len(cost), -1, np.int32)
    for n in np.flatnonzero((cost > 0.0) & (cost < INF)):
        out[n] = parent_candidates(lat, free, cost, int(n))[0][1]
    return out


def settled_count(cost, to):
    """The host's n_settled from the field alone."""
    reached = np.isfinite(cost)
    if not reached[to]:
        return int(reached.sum())
    n = np.arange(len(cost))
    return int((reached & ((cost < cost[to]) | ((cost == cost[to]) & (n <= to)))).sum())


def chain_of(lat, parent, src, to):
    """The chain src -> to through parent[], (n_chain, 3) of (ix, iy, t)."""
    out, v = [], to
    while True:
        out.append(split(lat, v))
        if v == src:
            break
        v = int(parent[v])
        assert v >= 0
    return np.array(out[::-1], np.int32).reshape(-1, 3)


def unique(cost_max, lat):
    """The fallback predicate: the least weight still moves the largest finite cost."""
    w_axis, _, w_turn = weights(lat)
    w = min(w_axis, w_turn) if lat.n_theta > 1 else w_axis
    return cost_max + w != cost_max


# ------------------------------------------------------------------------------------------ tiles
def tile_of(lat, x, y, t):
    tx, ty = -(-lat.nx // BX), -(-lat.ny // BY)
    return ((t // BT) * ty + y // BY) * tx + x // BX


def n_tiles(lat):
    return -(-lat.nx // BX) * -(-lat.ny // BY) * -(-lat.n_theta // BT)


def activates(lat, x, y, t):
    """The tiles whose halo holds node (x, y, t): those of its neighbour positions (free or not) that are not its own."""
    own, out = tile_of(lat, x, y, t), set()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if (dx or dy) and 0 <= x + dx < lat.nx and 0 <= y + dy < lat.ny:
                out.add(tile_of(lat, x + dx, y + dy, t))
    for s in (-1, 1):
        tt = (t + s) % lat.n_theta if lat.wrap_theta and lat.n_theta > 1 else t + s
        if 0 <= tt < lat.n_theta:
            out.add(tile_of(lat, x, y, tt))
    out.discard(own)
    return sorted(out)


# ------------------------------------------------------------------------------------------ the maps
def grid_lattice(nx, ny, nt=1, wrap=0, pitch=0.25, dtheta=math.pi / 4):
    return T.Lattice(-1.0, 0.5, pitch, nx, ny, 0.1, dtheta, nt, wrap, T.ARM)


def at(lat, ix, iy, t=0):
    return tuple(T.node_config(lat, ix, iy, t)[:3])


OPEN_NX_NY = {1: 15, B - 1: B, B: B + 1, B + 1: B - 1, 2 * B + 1: B}
OPEN_NT = (1, 2, 3, BT + 1)
MAZE_N = (3 * B + 1, 3 * B)   # 4 x 3 tiles
RANDOM_SEED, RANDOM_FREE = 2, 0.35   # (free fraction; see test_field_cpu.py on the choice)


def maze():
    """A comb: every odd row is a wall with one gap, at the right end and the left end in turn, so the only route runs
    every even row from end to end and crosses every column of tiles once per row."""
    nx, ny = MAZE_N
    free = np.ones((1, ny, nx), bool)
    for y in range(1, ny, 2):
        free[0, y, :] = False
        free[0, y, nx - 1 if y % 4 == 1 else 0] = True
    return free


@functools.lru_cache(maxsize=None)
def maps():
    """name -> (lattice, free (n_theta, ny, nx), from, to, snap_cells); the field's source is the snapped from."""
    m = {}
    for nx, ny in OPEN_NX_NY.items():
        for nt in OPEN_NT:
            for wrap in (0, 1):
                lat = grid_lattice(nx, ny, nt, wrap)
                m["open_%dx%dx%d_w%d" % (nx, ny, nt, wrap)] = (lat, np.ones((nt, ny, nx), bool), at(lat, nx // 3, 1, 0),
                                                               at(lat, nx - 1, ny - 1, nt - 1), 0)
    lat = grid_lattice(*MAZE_N)
    m["maze"] = (lat, maze(), at(lat, 0, 0), at(lat, 0, MAZE_N[1] - 2), 0)
    lat = grid_lattice(2 * B, 2 * B, 2 * BT, 1, 0.1, 2.0 * math.pi / (2 * BT))
    rng = np.random.RandomState(RANDOM_SEED)
    free = rng.random_sample((2 * BT, 2 * B, 2 * B)) < RANDOM_FREE
    free[0, B, B] = free[BT, 3, 3] = True
    m["random"] = (lat, free, at(lat, B, B, 0), at(lat, 3, 3, BT), 0)
    # a wall in one layer with a door in another (test_lattice_cpu.py's case)
    door = np.ones((3, 3, 5), bool)
    door[0, :, 2] = door[1, :, 2] = False
    lat = grid_lattice(5, 3, 3, 0)
    m["door_in_another_layer"] = (lat, door, at(lat, 0, 1, 0), at(lat, 4, 1, 0), 0)
    # the diagonal (B - 1, B - 1) -> (B, B) crosses the corner of four tiles; one of its axis cells is blocked
    lat = grid_lattice(2 * B, 2 * B)
    free = np.ones((1, 2 * B, 2 * B), bool)
    free[0, B - 1, B] = False
    m["forbidden_diagonal_on_a_tile_corner"] = (lat, free, at(lat, B - 1, B - 1), at(lat, B, B), 0)
    lat = grid_lattice(2 * B + 3, B + 2, BT + 1, 1)
    m["source_in_the_last_partial_tile"] = (lat, np.ones((BT + 1, B + 2, 2 * B + 3), bool), at(lat, 2 * B + 2, B + 1, BT),
                                            at(lat, 0, 0, 0), 0)
    lat = grid_lattice(B + 1, B + 1, 2, 0)
    free = np.ones((2, B + 1, B + 1), bool)
    free[:, B - 1:, B - 1] = free[:, B - 1, B - 1:] = False   # walls off the corner (B, B)
    free[1, B, B] = False
    m["isolated_source"] = (lat, free, at(lat, B, B, 0), at(lat, 0, 0, 0), 0)
    lat = grid_lattice(2 * B, 5, 2, 1)
    free = np.ones((2, 5, 2 * B), bool)
    free[:, :, B] = False   # a wall along the tiles' seam, in both layers
    m["unreachable_to"] = (lat, free, at(lat, 1, 1, 0), at(lat, 2 * B - 1, 3, 1), 0)
    # Sources on a tile's rim whose way on lies in the next tile alone: the source is never lowered, so only the start of
    # round 0 can run that tile.  A one-row corridor over two tiles from its seam; one column of headings over two
    # tiles from the lower tile's top layer; the same through the wrap, the layer above the source blocked; a source on
    # the corner of four tiles with its own tile's cells around it blocked.
    lat = grid_lattice(2 * B, 1)
    m["corridor_from_the_seam"] = (lat, np.ones((1, 1, 2 * B), bool), at(lat, B - 1, 0), at(lat, 2 * B - 1, 0), 0)
    lat = grid_lattice(1, 1, 2 * BT, 0)
    m["headings_from_the_seam"] = (lat, np.ones((2 * BT, 1, 1), bool), at(lat, 0, 0, BT - 1), at(lat, 0, 0, 2 * BT - 1), 0)
    lat = grid_lattice(1, 1, 2 * BT, 1)
    free = np.ones((2 * BT, 1, 1), bool)
    free[1] = False
    m["headings_through_the_wrap"] = (lat, free, at(lat, 0, 0, 0), at(lat, 0, 0, BT), 0)
    lat = grid_lattice(2 * B, 2 * B)
    free = np.ones((1, 2 * B, 2 * B), bool)
    free[0, B - 2, B - 2:B] = free[0, B - 1, B - 2] = False
    m["source_on_a_tile_corner"] = (lat, free, at(lat, B - 1, B - 1), at(lat, 0, 0), 0)
    lat = grid_lattice(B + 2, 3, 2, 1)
    m["from_is_to"] = (lat, np.ones((2, 3, B + 2), bool), at(lat, B, 1, 1), at(lat, B, 1, 1), 0)
    return m


ONE_TILE = [k for k, v in maps().items() if n_tiles(v[0]) == 1]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restated answers of map `name`: dict of route (lattice_restatement.route's dict), src and to node numbers
    (to None where the ends do not snap), cost, parent (the search's), order."""
    lat, free, frm, to, snap = maps()[name]
    r = T.route(lat, free, frm, to, snap)
    assert r["from_node"] is not None
    cost, parent, order = dijkstra(lat, free, r["from_node"])
    node = lambda c: (c[2] * lat.ny + c[1]) * lat.nx + c[0]
    return dict(route=r, src=node(r["from_node"]), to=None if r["to_node"] is None else node(r["to_node"]), cost=cost,
                parent=parent, order=order)
