"""Numpy restatement of the dense edge checks and of path shortcutting (include/smp_gpu.h: smp_check_edges,
smp_shortcut_path), shared by test_gpu_edges.py, test_gpu_shortcut.py, test_shim_shortcut.py and test_edges_cpu.py.

It follows the wording of the header: the density rule (revolute and prismatic lengths summed for joints ascending, m
hops of at most one planner step, M = n * m, point k = a + k * (d / M) with the quotient formed first) and the dynamic
program (j ascending, i ascending, first strict minimum).  Validity of the points comes from the CPU oracle
(oracle.Oracle.check_configs), all points of a call in one batch.  numpy evaluates every operation on its own, so no
product and sum are ever contracted."""
import functools
import os

import numpy as np


def density(a, b, rev, n, f):
    """(m, M) of the edges a[i] -> b[i]; a, b: (E, 8)."""
    a = np.asarray(a, np.float64).reshape(-1, 8)
    b = np.asarray(b, np.float64).reshape(-1, 8)
    d = b - a
    sr, sp = np.zeros(len(a)), np.zeros(len(a))
    for j in range(8):
        if rev[j]:
            sr = sr + d[:, j] * d[:, j]
        else:
            sp = sp + d[:, j] * d[:, j]
    m = np.maximum(1, np.ceil(np.maximum(np.sqrt(sr), np.sqrt(sp)) / f)).astype(np.int64)
    return m, n * m


def edge_points(a, b, M):
    """The M + 1 points of one edge, (M + 1, 8)."""
    a = np.asarray(a, np.float64)
    step = (np.asarray(b, np.float64) - a) / float(M)
    return a[None, :] + np.arange(M + 1, dtype=np.float64)[:, None] * step[None, :]


def all_points(a, b, M):
    """The points of every edge stacked, and each edge's offset into the stack (len E + 1)."""
    pts = [edge_points(a[i], b[i], int(M[i])) for i in range(len(a))]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    return (np.concatenate(pts) if pts else np.zeros((0, 8))), off


def first_invalid(orc, a, b, M, self_=True, map_=True):
    """Index of each edge's first colliding point by the oracle, -1 if free."""
    pts, off = all_points(a, b, M)
    valid = orc.check_configs(pts, self_, map_) if len(pts) else np.zeros(0, np.uint8)
    out = np.full(len(a), -1, np.int64)
    for i in range(len(a)):
        bad = np.flatnonzero(valid[off[i]:off[i + 1]] == 0)
        if len(bad):
            out[i] = bad[0]
    return out


def dist(a, b):
    s = 0.0
    for j in range(8):
        d = float(b[j]) - float(a[j])
        s += d * d
    return float(np.sqrt(s))


def candidates(k, window=0):
    """Candidate pairs in the order of the dynamic program: j ascending, then i ascending."""
    w = k - 1 if window <= 0 or window > k - 1 else window
    return [(i, j) for j in range(1, k) for i in range(max(0, j - w), j)]


def shortcut(orc, w, rev, n, f, self_=True, map_=True, window=0):
    """smp_shortcut_path restated: dict of path (None when blocked), n_edges, n_valid, configs_checked, cost_in,
    cost_out, first_blocked and, for the tests' own conditions, pairs / first (per candidate)."""
    w = np.asarray(w, np.float64).reshape(-1, 8)
    k = len(w)
    pairs = candidates(k, window)
    a = np.array([w[i] for i, _ in pairs])
    b = np.array([w[j] for _, j in pairs])
    m, M = density(a, b, rev, n, f)
    first = first_invalid(orc, a, b, M, self_, map_)
    return shortcut_route(w, pairs, a, b, m, M, first, n)


def shortcut_route(w, pairs, a, b, m, M, first, n):
    """The part of shortcut that needs no oracle: the dynamic program over the candidates' first invalid points and
    the rows of the route it finds."""
    k = len(w)
    dp = [float("inf")] * k
    pred = [-1] * k
    pe = [-1] * k
    dp[0] = 0.0
    first_blocked = -1
    for e, (i, j) in enumerate(pairs):
        if first[e] >= 0:
            if i == j - 1 and first_blocked < 0:
                first_blocked = i
            continue
        c = dp[i] + dist(w[i], w[j])
        if c < dp[j]:
            dp[j], pred[j], pe[j] = c, i, e
    cost_in = 0.0
    for j in range(1, k):
        cost_in += dist(w[j - 1], w[j])
    out = dict(n_edges=len(pairs), n_valid=int((first < 0).sum()),
               configs_checked=int(np.where(first < 0, M + 1, first + 1).sum()), cost_in=cost_in, pairs=pairs,
               first=first, m=m)
    if pred[k - 1] < 0:
        out.update(path=None, cost_out=0.0, first_blocked=first_blocked)
        return out
    route = []
    j = k - 1
    while j > 0:
        route.append(pe[j])
        j = pred[j]
    rows = []
    for e in reversed(route):
        pts = edge_points(a[e], b[e], int(M[e]))
        rows.append(a[e])
        rows.extend(pts[n:int(M[e]):n])
    rows.append(w[k - 1])
    out.update(path=np.array(rows), cost_out=dp[k - 1], first_blocked=-1)
    return out


def subsample(path, k=12):
    """At most k waypoints of a path, ends kept."""
    path = np.asarray(path, np.float64)
    idx = np.unique(np.round(np.linspace(0, len(path) - 1, min(k, len(path)))).astype(int))
    return path[idx]


# ------------------------------------------------------------------------------------------ shared inputs
# The inputs of the edge and shortcut tests, built once per process from the CPU oracle alone (the GPU tests and the CPU
# test of their non-vacuity conditions share them).
N_SEG, STEP = 20, 0.5  # smp_params_default: num_traj_segments, step_factor
CT = 32                # configurations per collision tile of the edge kernel


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def orobot():
    from oracle import oracle as O
    return O.OracleRobot(os.path.join(_root(), "squirrel_motion_planner_amd", "data", "robotino_model.json"))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene description, OracleScene) of c1 / c2 / c4 / room3, as tests/test_gpu_parity.py builds them."""
    from oracle import oracle as O
    from squirrel_motion_planner_amd import scenes
    if name.startswith("room"):
        f = np.load(os.path.join(_root(), "tests", "golden", name + "_keys.npz"))
        keys = np.concatenate([f["keys"].astype(np.int64), scenes.floor_keys([0.0, 0.0], 0.05, 3.0)])
        sc = scenes.Scene(name, keys, 0.05, [0, 0, 0] + scenes.ARM_FOLDED, [1, 1, 0] + scenes.ARM_UNFOLDED, (0, 0),
                          (0, 0))
        sc.env_x, sc.env_y = sc.bounds()
    else:
        sc = {"c1": scenes.empty_room, "c2": scenes.box_room, "c4": scenes.narrow_passage}[name]()
    return sc, O.OracleScene(sc.keys, sc.res)


def oracle_for(name, map_enabled=None):
    from oracle import oracle as O
    return O.Oracle(orobot(), scene(name)[1], map_enabled=map_enabled)


@functools.lru_cache(maxsize=None)
def oracle_path(name, seed, iters, n_pts=N_SEG):
    sc, _ = scene(name)
    o = oracle_for(name).plan(sc.start, sc.goal, env_x=sc.env_x, env_y=sc.env_y, max_iter=iters, seed=seed,
                              n_pts=n_pts)
    assert o["status"] == 0
    return o["path"]


def random_configs(sc, n, seed):
    """tests/test_gpu_parity.py random_configs."""
    rb = orobot()
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sc.env_x, sc.env_y
    return np.column_stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)] +
                           [rng.uniform(rb.q_min[j] - 0.3, rb.q_max[j] + 0.3, n) for j in range(2, 8)])


# Seeds of long_edges, chosen on the CPU so that the oracle alone meets the conditions test_gpu_edges.py asserts.
LONG_SEED = {"c2": 23, "room3": 1}


@functools.lru_cache(maxsize=None)
def long_edges(name):
    """64 long edges: 2048 random pairs drawn as random_configs draws them, the first 63 whose endpoints are both valid
    by the oracle, and the first pair whose start is invalid and whose end is valid (an edge that collides at index 0
    cannot have a valid start).  Returns (a, b)."""
    sc, _ = scene(name)
    q = random_configs(sc, 4096, LONG_SEED[name])
    a, b = q[:2048], q[2048:]
    orc = oracle_for(name)
    va, vb = orc.check_configs(a).astype(bool), orc.check_configs(b).astype(bool)
    idx = np.concatenate([np.flatnonzero(va & vb)[:63], np.flatnonzero(~va & vb)[:1]])
    assert len(idx) == 64
    return a[idx], b[idx]


# The shortcut tests' paths: an oracle plan subsampled to 12 waypoints, ends kept.  C2's seed is chosen on the CPU: the
# subsampled path is free at the dense check (the paths of seeds 3 and 8 hold waypoints that collide themselves, which
# the reference's planner never re-checks after it truncates an edge), and the oracle alone meets the conditions
# test_gpu_shortcut.py asserts.
SHORTCUT_PLANS = {"c2": (7, 300), "c4": (2, 400)}


@functools.lru_cache(maxsize=None)
def shortcut_input(name):
    seed, iters = SHORTCUT_PLANS[name]
    return subsample(oracle_path(name, seed, iters), 12)


@functools.lru_cache(maxsize=None)
def shortcut_expected(name, window=0):
    return shortcut(oracle_for(name), shortcut_input(name), orobot().rev, N_SEG, STEP, window=window)


# Blocked path: C1's plan (empty room, seed 1, 50 iterations) subsampled to 8 waypoints, then one 0.3 m x 0.3 m x 1.2 m
# box centred on the path's middle waypoint.  By the oracle both end waypoints stay valid and no route remains.
BLOCK_HALF, BLOCK_HEIGHT = 0.15, 1.2


@functools.lru_cache(maxsize=None)
def blocked_case():
    """(waypoints, keys of the blocked scene, resolution, restatement's result)."""
    from oracle import oracle as O
    from squirrel_motion_planner_amd import scenes
    sc, _ = scene("c1")
    path = oracle_path("c1", 1, 50)
    w = subsample(path, 8)
    mid = path[len(path) // 2]
    box = scenes._box_keys([mid[0] - BLOCK_HALF, mid[1] - BLOCK_HALF, 0.0],
                           [mid[0] + BLOCK_HALF, mid[1] + BLOCK_HALF, BLOCK_HEIGHT], sc.res)
    keys = np.concatenate([sc.keys, box])
    orc = O.Oracle(orobot(), O.OracleScene(keys, sc.res))
    return w, keys, sc.res, shortcut(orc, w, orobot().rev, N_SEG, STEP), orc.check_configs(w)
