"""The tree audit: a finished BiRRT* run checked by plain tree arithmetic (DESIGN.md "The tree audit").

Data in, report out.  This module imports neither the oracle nor the library: it takes a state dict in the form of
`GpuPlanner.export_state()` / `Oracle.export_state()`, the run's result (path, cost rows, counters, in the names of
the C ABI's smp_stats; `from_oracle` renames an oracle result), the query's start and goal, `n_pts`
(num_traj_segments_interp), `near_r` and the revolute mask of the model JSON, and recomputes from the configurations
alone what the planner stored: the structure (A1), the in-edges (A2), the three costs of every node (A3), their bounds
(A4), the connection record with c_best (A5), the path (A6) and the cost rows and counters (A7).

Sums and norms are taken in np.longdouble; every check is vectorised over the nodes (depth and cycles by pointer
doubling), only the two solution branches are walked node by node.

Tolerances, with eps = 2^-52, R the tree's rewire counter, n the segment count:
  tol_c = 2 (R + n + 8) eps max(1, max cost)   a stored cost takes one rounding per segment norm when its edge is made
                                               and one more per rewire above it (the cost update's old + red)
  tol_q = 4 (R + 1) eps max(1, max |q|)        each rewire re-rounds the node's configuration to the end of the new
                                               interpolation; R = 0 leaves the 3.5 ulp of s + k ((g - s) / n)
A quantity summed over both trees takes the sum of the two trees' tolerances.
"""
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
NO_SOLUTION_COST = 10000.0
TREES = ("start", "goal")

# result keys compared with the state (A7), and their names in an oracle result
_ORACLE_KEYS = {"iterations": "iterations", "first_solution_iter": "first_iter", "configs_checked": "checked",
                "configs_valid": "valid", "nodes_start": "n_start", "nodes_goal": "n_goal",
                "edges_start": "edges_start", "edges_goal": "edges_goal", "rewires_start": "rewires_start",
                "rewires_goal": "rewires_goal", "conn_node_b": "conn_b", "conn_node_a": "conn_a",
                "connected_tree_is_start": "conn_start", "cost_best": "cost", "path": "path", "cost_rows": "cost_rows"}


def from_oracle(o):
    """An oracle result under the keys of the C ABI's result (the ones the audit reads)."""
    return {k: o[v] for k, v in _ORACLE_KEYS.items()}


class Report:
    """findings: (name, detail) pairs, name = check or check[tree]; residuals: the largest residual of every check that
    ran; info: tolerances, depths, rewires, the tree sum and c_best; skipped: checks that had nothing sound to run on."""

    def __init__(self):
        self.findings, self.residuals, self.info, self.skipped = [], {}, {}, []

    @property
    def ok(self):
        return not self.findings

    def names(self):
        return sorted({n for n, _ in self.findings})

    def check(self, name, residual, bound, detail=""):
        """Records the residual; a finding unless residual <= bound."""
        r = float(residual)
        self.residuals[name] = max(self.residuals.get(name, -np.inf), r)
        if not r <= bound:
            self.findings.append((name, "%s residual %.3e > %.3e" % (detail, r, bound)))

    def require(self, name, cond, detail=""):
        self.residuals.setdefault(name, 0.0)
        if not cond:
            self.residuals[name] = 1.0
            self.findings.append((name, detail))

    def __str__(self):
        out = ["tree audit: %s" % ("clean" if self.ok else "%d finding(s)" % len(self.findings))]
        out += ["  FINDING %s: %s" % f for f in self.findings]
        out += ["  skipped %s" % s for s in self.skipped]
        out += ["  %-28s %.3e" % (k, v) for k, v in sorted(self.residuals.items())]
        out += ["  %-28s %s" % (k, v) for k, v in sorted(self.info.items())]
        return "\n".join(out)


def _norms(d, rev):
    """(total, revolute, prismatic) Euclidean norms of the rows of d (m, 8), longdouble."""
    sq = np.asarray(d, LD) ** 2
    return np.sqrt(np.stack([sq.sum(1), sq[:, rev].sum(1), sq[:, ~rev].sum(1)], 1))


def _maxabs(a):
    a = np.asarray(a)
    return float(np.abs(a).max()) if a.size else 0.0


def _depths(parent):
    """(depth of every node, mask of the nodes that do not reach node 0) by pointer doubling; parent[0] taken as 0."""
    n = len(parent)
    anc = parent.copy()
    anc[0] = 0
    depth = (np.arange(n) != 0).astype(np.int64)
    for _ in range(max(1, int(n).bit_length()) + 1):
        depth = depth + depth[anc]
        anc = anc[anc]
    return depth, anc != 0


def _tolerances(t, n_pts):
    R = int(t["rewires"])
    tol_c = 2.0 * (R + n_pts + 8) * EPS * max(1.0, _maxabs(t["cost"]))
    tol_q = 4.0 * (R + 1) * EPS * max(1.0, _maxabs(t["conf"]))
    return tol_c, tol_q


def _audit_tree(rep, name, t, n_pts, near_r, rev):
    """A1 - A4 of one tree; True if every node reaches the root (the branches can be walked)."""
    tag = "[%s]" % name
    parent = np.asarray(t["parent"], np.int64)
    conf, cost = np.asarray(t["conf"], LD), np.asarray(t["cost"], LD)
    n = len(parent)
    tol_c, tol_q = _tolerances(t, n_pts)
    rep.info["tol_c" + tag], rep.info["tol_q" + tag] = tol_c, tol_q
    rep.info["nodes" + tag], rep.info["rewires" + tag] = n, int(t["rewires"])

    # ---- A1 structure
    rep.require("A1.root" + tag, n >= 1 and parent[0] == 0, "parent[0] = %s" % (parent[0] if n else None))
    in_range = (parent >= 0) & (parent < n)
    par = np.where(in_range, parent, 0)
    depth, lost = _depths(par)
    lost |= ~in_range
    rep.require("A1.reach" + tag, not lost.any(), "nodes off the root (cycle or bad parent): %s" % np.flatnonzero(lost)[:8])
    off, ids = np.asarray(t["child_off"], np.int64), np.asarray(t["child_ids"], np.int64)
    lists_ok = len(off) == n + 1 and off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0) and \
        (len(ids) == 0 or (ids.min() >= 0 and ids.max() < n))
    if lists_ok:
        count = np.bincount(ids, minlength=n)
        want = np.ones(n, np.int64)
        want[0] = 0
        bad = np.flatnonzero(count != want)
        rep.require("A1.children_once" + tag, len(ids) == n - 1 and len(bad) == 0,
                    "%d listed for %d nodes; listed != once: %s" % (len(ids), n, bad[:8]))
        owner = np.repeat(np.arange(n), np.diff(off))
        bad = ids[owner != parent[ids]]
        rep.require("A1.children_parent" + tag, len(bad) == 0, "listed under another node than the parent: %s" % bad[:8])
    else:
        rep.require("A1.children_once" + tag, False, "malformed child lists")
    rep.require("A1.edge_count" + tag, int(t["edges"]) == n - 1, "edges %d, nodes %d" % (int(t["edges"]), n))
    if lost.any():
        rep.skipped.append("A2-A4%s: parent chains do not end at the root" % tag)
        return False
    rep.info["depth" + tag] = int(depth.max())

    # ---- A2 in-edges
    k = np.arange(1, n)
    rep.check("A2.e_start" + tag, _maxabs(np.asarray(t["e_start"], LD)[k] - conf[par[k]]), tol_q)
    rep.check("A2.e_target" + tag, _maxabs(np.asarray(t["e_target"], LD)[k] - conf[k]), tol_q)

    # ---- A3 costs: every node's three costs from its parent's and the configurations
    rep.check("A3.root_cost" + tag, _maxabs(cost[0]), 0.0)
    edge = _norms(conf[k] - conf[par[k]], rev)
    res = np.abs((cost[k] - cost[par[k]]) - edge)
    worst = k[np.argsort(res.max(1))[::-1][:4]] if n > 1 else []
    rep.check("A3.edge_cost" + tag, res.max() if n > 1 else 0.0, tol_c, "nodes %s" % list(worst))
    rep.info["A3.offenders" + tag] = [int(i) for i in k[(res > tol_c).any(1)]][:16] if n > 1 else []

    # ---- A4 bounds
    rep.check("A4.cost_bound" + tag, (_norms(conf - conf[0], rev) - cost).max(), tol_c)
    rep.check("A4.edge_length" + tag, (edge[:, 0].max() - LD(near_r)) if n > 1 else -np.inf, tol_q)
    return True


def _branch(parent, node):
    """The nodes from `node` up to the child of the root."""
    out = []
    while node != 0:
        out.append(node)
        node = int(parent[node])
    return out


def _edge_points(t, c, n_pts):
    """Points 0 .. n_pts of node c's in-edge: s + k ((g - s) / n_pts)."""
    s, g = np.asarray(t["e_start"][c], LD), np.asarray(t["e_target"][c], LD)
    return s[None, :] + np.arange(n_pts + 1, dtype=LD)[:, None] * ((g - s) / LD(n_pts))[None, :]


def audit(state, result, start, goal, n_pts, near_r, rev_mask, first_row=1):
    """The report of one finished single-query run.  first_row: the iteration of the first cost row (1, or the resumed
    run's first iteration)."""
    rep = Report()
    rev = np.asarray(rev_mask, bool)
    iv, dv = np.asarray(state["iv"], np.int64), np.asarray(state["dv"], np.float64)
    have_sol = bool(iv[5])
    sound = {name: _audit_tree(rep, name, state[name], n_pts, near_r, rev) for name in TREES}
    tol = {name: _tolerances(state[name], n_pts) for name in TREES}
    tol_c, tol_q = tol["start"][0] + tol["goal"][0], max(tol["start"][1], tol["goal"][1])
    start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
    h0 = _norms((goal - start)[None, :], rev)[0]
    rep.info["have_sol"] = have_sol

    if have_sol and all(sound.values()):
        nameB, nameA = ("start", "goal") if iv[6] else ("goal", "start")
        rec = {"B": (state[nameB], nameB, int(iv[8]), int(iv[9]), dv[3:11], dv[11:14]),
               "A": (state[nameA], nameA, int(iv[10]), int(iv[11]), dv[14:22], dv[22:25])}
        in_tree = all(0 <= r[2] < len(r[0]["parent"]) for r in rec.values())
        rep.require("A5.copy_id", in_tree, "nB %d, nA %d" % (rec["B"][2], rec["A"][2]))
        if in_tree:
            # ---- A5 connection record
            for k, (t, name, i, p, q, c) in rec.items():
                rep.require("A5.copy_parent[n%s]" % k, p == int(t["parent"][i]),
                            "copy %d, %s tree %d" % (p, name, int(t["parent"][i])))
                rep.check("A5.copy_cost[n%s]" % k, _maxabs(np.asarray(c, LD) - np.asarray(t["cost"][i], LD)),
                          tol[name][0])
                rep.check("A5.copy_q[n%s]" % k, _maxabs(np.asarray(q, LD) - np.asarray(t["conf"][i], LD)), tol[name][1])
            (tB, _, iB, _, _, _), (tA, _, iA, _, _, _) = rec["B"], rec["A"]
            rep.check("A5.meet", _maxabs(np.asarray(tB["conf"][iB], LD) - np.asarray(tA["conf"][iA], LD)), tol_q)
            tree_sum = np.asarray(tB["cost"][iB], LD) + np.asarray(tA["cost"][iA], LD)
            rep.info["tree_sum"], rep.info["c_best"] = [float(v) for v in tree_sum], [float(v) for v in dv[:3]]
            rep.info["c_best_below_tree_sum"] = float(tree_sum[0] - LD(dv[0]))
            rep.check("A5.cbest_parts", _maxabs(np.asarray(dv[1:3], LD) - tree_sum[1:]), tol_c)
            rep.check("A5.cbest_total", LD(dv[0]) - tree_sum[0], tol_c)
            rep.check("A5.cbest_h0", (h0 - np.asarray(dv[:3], LD)).max(), tol_c)

            # ---- A6 path: the start-tree branch root to connection node, then the goal-tree branch down to its root
            path = np.asarray(result["path"], np.float64).reshape(-1, 8)
            ts, tg = state["start"], state["goal"]
            i_s, i_g = (iB, iA) if iv[6] else (iA, iB)
            es, eg = _branch(ts["parent"], i_s)[::-1], _branch(tg["parent"], i_g)
            rep.info["path_edges"] = (len(es), len(eg))
            want = [_edge_points(ts, c, n_pts)[:-1] for c in es]
            want += [_edge_points(tg, c, n_pts)[:0:-1] for c in eg]
            if eg:
                want.append(_edge_points(tg, eg[-1], n_pts)[:1])
            want = np.concatenate(want) if want else np.zeros((0, 8), LD)
            rows = (len(es) + len(eg)) * n_pts + (1 if eg else 0)
            rep.require("A6.row_count", len(path) == rows == len(want), "%d rows, %d edges of %d points%s" % (
                len(path), len(es) + len(eg), n_pts, " + 1" if eg else ""))
            if len(path):
                rep.require("A6.first_is_start", np.array_equal(path[0], start), "first row %s" % path[0])
                if eg:
                    rep.require("A6.last_is_goal", np.array_equal(path[-1], goal), "last row %s" % path[-1])
            if len(path) == len(want):
                rep.check("A6.waypoints", _maxabs(np.asarray(path, LD) - want), tol_q)
                if rep.residuals["A6.waypoints"] <= tol_q:
                    length = _norms(np.diff(np.asarray(path, LD), axis=0), rev)[:, 0].sum()
                    if not eg and es:  # the last point of the last start-tree edge is not part of such a path
                        length += _norms((_edge_points(ts, es[-1], n_pts)[-1] - np.asarray(path[-1], LD))[None, :], rev)[0, 0]
                    rep.check("A6.length", abs(length - tree_sum[0]), max(len(path), 1) * tol_c)
                else:
                    rep.skipped.append("A6.length: the waypoints are not the branches' in-edges")
            else:
                rep.skipped.append("A6.waypoints, A6.length: row count")
    elif have_sol:
        rep.skipped.append("A5, A6: a tree's parent chains do not end at the root")

    # ---- A7 cost rows and counters
    rows = np.asarray(result["cost_rows"], np.float64).reshape(-1, 5)
    first = int(iv[3])
    if len(rows):
        it = rows[:, 0]
        rep.require("A7.row_iters", np.array_equal(it, first_row + np.arange(len(rows))) and it[-1] == iv[0],
                    "iterations %s .. %s for %d rows, state at %d" % (it[0], it[-1], len(rows), iv[0]))
        rise = np.diff(rows[:, 2])
        rep.check("A7.rows_monotone", rise.max() if len(rise) else 0.0, 0.0, "row %d" % (np.argmax(rise) + 1 if len(rise) else 0))
        solved = (it > first) if have_sol else np.zeros(len(rows), bool)
        rep.require("A7.rows_first", np.all(rows[~solved, 2] == NO_SOLUTION_COST) and np.all(rows[solved, 2] < NO_SOLUTION_COST),
                    "first solution in iteration %d" % first)
        rep.require("A7.rows_last", np.array_equal(rows[-1, 2:5], dv[:3]), "last row %s, c_best %s" % (rows[-1, 2:5], dv[:3]))
    want = {"iterations": iv[0], "configs_checked": iv[1], "configs_valid": iv[2], "first_solution_iter": iv[3]}
    for name in TREES:
        want["nodes_" + name] = len(state[name]["parent"])
        want["edges_" + name] = state[name]["edges"]
        want["rewires_" + name] = state[name]["rewires"]
    if have_sol:
        want.update(conn_node_b=iv[8], conn_node_a=iv[10], connected_tree_is_start=iv[6])
    bad = ["%s: result %s, state %s" % (k, result[k], v) for k, v in want.items() if int(result[k]) != int(v)]
    if not np.array_equal(np.asarray(result["cost_best"], np.float64), dv[:3]):
        bad.append("cost_best: result %s, state %s" % (list(result["cost_best"]), list(dv[:3])))
    rep.require("A7.counters", not bad, "; ".join(bad))
    rep.require("A7.valid_le_checked", int(result["configs_valid"]) <= int(result["configs_checked"]),
                "%s valid of %s checked" % (result["configs_valid"], result["configs_checked"]))
    return rep
