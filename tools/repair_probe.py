"""Path repair, then shortcutting, on a full planner path: smp_repair_path and smp_shortcut_path on C2
(scenes.box_room).

The path is the planner's own output for a budget of 1e6 collision-checked configurations (seed 1), not subsampled: it
fails the dense check (smp_shortcut_path alone answers SMP_ERR_NO_SOLUTION).  smp_repair_path bridges its blocked
stretches with one-via detours (default options: 256 samples per gap and round, 4 rounds, seed 1) and
smp_shortcut_path then shortens the repaired path.  kernel_ms is the library's HIP-event time around its kernels (the
waypoint check, the adjacent-edge check and the detour launches for the repair), total_ms its host clock from call entry
to return.  One process, one warm-up call each, then REPS calls; medians.

For comparison the detour items of the call are replayed round by round with smp_sample_detours (the same gaps, seed,
rounds and half widths), and the points the kernel's order makes it check -- per item the 32-point tiles of the leg
v -> b from v on, then those of the leg a -> v from v back, up to and including the first tile that holds a colliding
point -- are built with numpy and checked by the CPU oracle's check_configs on one host core, timing only those calls.
The oracle's free / blocked answer per item must equal the kernel's.  Prints one JSON line.

    python tools/repair_probe.py [--reps 10] [--samples 1000000] > profiles/repair.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from squirrel_motion_planner_amd import _lib as L  # noqa: E402
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene  # noqa: E402

CT = 32  # configurations per collision tile of detours_kernel


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def call(fn, *args, **kw):
    """(status, output or None, info)"""
    try:
        out, info = fn(*args, **kw)
        return L.SMP_OK, out, info
    except L.SmpError as e:
        if e.status != L.SMP_ERR_NO_SOLUTION:
            raise
        return e.status, None, e.info


def find_gaps(valid, first):
    """Step 2 of smp_repair_path: [l, r] per gap."""
    gaps = []
    for i in range(len(first)):
        if first[i] < 0:
            continue
        l, r = i, i + 1
        while not valid[l]:
            l -= 1
        while not valid[r]:
            r += 1
        if gaps and l < gaps[-1][1]:
            gaps[-1][1] = max(gaps[-1][1], r)
        else:
            gaps.append([l, r])
    return gaps


def dist(a, b):
    s = 0.0
    for j in range(8):
        d = float(b[j]) - float(a[j])
        s += d * d
    return float(np.sqrt(s))


def leg(a, b, M):
    return a[None, :] + np.arange(M + 1, dtype=np.float64)[:, None] * ((b - a) / float(M))[None, :]


def item_tiles(a, v, b, M1, M2):
    """The item's points tile by tile in the kernel's order."""
    l1, l2 = leg(a, v, M1), leg(v, b, M2)
    tiles = [l2[c:c + CT] for c in range(0, M2 + 1, CT)]
    tiles += [l1[c:c + CT] for c in reversed(range(0, M1 + 1, CT))]
    return tiles


def replay(gp, orc, path, samples, rounds, seed, step):
    """The call's items round by round: (items, free items, rounds used, points the kernel's order checks, all points of
    the items' legs, oracle seconds over the former)."""
    valid = gp.check_configs(path)
    first, _ = gp.check_edges(path[:-1], path[1:])
    gaps = find_gaps(valid, first)
    a = np.array([path[l] for l, _ in gaps])
    b = np.array([path[r] for _, r in gaps])
    open_ = list(range(len(gaps)))
    n_items = n_free = used = points = all_points = 0
    secs = 0.0
    for rho in range(rounds):
        if not open_:
            break
        d = gp.sample_detours(a, b, samples, step * 2.0 ** rho, seed=seed, round=rho)  # g = the gap's index
        used += 1
        still = []
        for g in open_:
            best, chosen = float("inf"), -1
            for s in range(samples):
                tiles = item_tiles(a[g], d["v"][g, s], b[g], int(d["M1"][g, s]), int(d["M2"][g, s]))
                ok = [bool(orc.check_configs(t).all()) for t in tiles]  # (not timed: finds where the kernel stops)
                run = tiles[:ok.index(False) + 1] if False in ok else tiles
                pts = np.ascontiguousarray(np.concatenate(run))
                t0 = time.perf_counter()
                v = orc.check_configs(pts)
                secs += time.perf_counter() - t0
                points += len(pts)
                all_points += sum(len(t) for t in tiles)
                assert bool(v.all()) == bool(d["free"][g, s]), (rho, g, s)
                n_items += 1
                if d["free"][g, s]:
                    n_free += 1
                    c = dist(a[g], d["v"][g, s]) + dist(d["v"][g, s], b[g])
                    if c < best:
                        best, chosen = c, s
            if chosen < 0:
                still.append(g)
        open_ = still
    return n_items, n_free, used, points, all_points, secs, gaps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sc = scenes.box_room()
    gp = GpuPlanner(Robot())
    gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=a.samples, seed=a.seed))
    if r["status"] != L.SMP_OK:
        raise SystemExit("no path within the budget (status %d)" % r["status"])
    path = r["path"]
    s0, _, i0 = call(gp.shortcut_path, path)  # the shortcut alone
    o = L.RepairOpts()
    L.lib().smp_repair_opts_default(o)
    status, repaired, info = call(gp.repair_path, path)  # warm-up
    kern, total = [], []
    for _ in range(a.reps):
        s, out, i = call(gp.repair_path, path)
        assert s == status and i["n_items"] == info["n_items"] and i["n_free"] == info["n_free"]
        assert (out is None) == (repaired is None) and (out is None or np.array_equal(out, repaired))
        kern.append(i["kernel_ms"])
        total.append(i["total_ms"])
    res = {"scene": sc.name, "plan": {"samples": a.samples, "seed": a.seed, "iterations": r["iterations"],
                                      "cost": r["cost_best"][0]},
           "clocks": {"kernel_ms": "smp_repair_info.kernel_ms / smp_shortcut_info.kernel_ms (HIP events around the kernels)",
                      "total_ms": "smp_repair_info.total_ms / smp_shortcut_info.total_ms (host clock, call entry to return)",
                      "oracle_s": "time.perf_counter around Oracle.check_configs, one host core, the points the "
                                  "kernel's tile order checks"},
           "reps": a.reps, "warmup": 1, "k": int(len(path)),
           "shortcut_alone": {"status": s0, "first_blocked": i0["first_blocked"]},
           "repair": {"opts": {"samples": o.samples, "rounds": o.rounds, "seed": o.seed}, "status": status,
                      "rows_out": 0 if repaired is None else int(len(repaired)),
                      **{f: info[f] for f in ("n_blocked_edges", "n_gaps", "n_repaired", "n_items", "n_free",
                                              "rounds_used", "cost_in", "cost_out", "first_blocked")},
                      "kernel_ms": stats(kern), "total_ms": stats(total)}}
    orc = O.Oracle(O.OracleRobot(L.MODEL_JSON), O.OracleScene(sc.keys, sc.res))
    n_items, n_free, used, points, all_points, cpu_s, gaps = replay(gp, orc, path, o.samples, o.rounds, o.seed,
                                                                    gp.params.step_factor)
    assert (n_items, n_free, used) == (info["n_items"], info["n_free"], info["rounds_used"])
    res["repair"]["gaps"] = gaps
    res["detour_items"] = {"items": n_items, "free": n_free, "points_checked_in_tile_order": points,
                           "points_of_all_legs": all_points, "oracle_s": cpu_s,
                           "oracle_configs_per_second": points / cpu_s if cpu_s > 0 else None,
                           "ratio_oracle_over_repair_total": cpu_s / (np.median(total) * 1e-3),
                           "ratio_oracle_over_repair_kernel": cpu_s / (np.median(kern) * 1e-3)}
    if repaired is not None:
        ss, short, si = call(gp.shortcut_path, repaired)  # warm-up
        sk, st = [], []
        for _ in range(a.reps):
            s, out, i = call(gp.shortcut_path, repaired)
            assert s == ss and i["configs_checked"] == si["configs_checked"]
            sk.append(i["kernel_ms"])
            st.append(i["total_ms"])
        res["shortcut_after_repair"] = {"status": ss, "k": int(len(repaired)),
                                        "rows_out": 0 if short is None else int(len(short)),
                                        **{f: si[f] for f in ("n_edges", "n_valid", "configs_checked", "cost_in",
                                                              "cost_out", "first_blocked")},
                                        "kernel_ms": stats(sk), "total_ms": stats(st)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
