"""The host logic of the path tools (csrc/smp_paths.cpp: density rule, shortcut dynamic program, gap gathering, detour
choice, repaired route, output rows) on the CPU, built with ASAN / UBSAN and driven by tests/cpp/paths_table.cpp:
every result bit for bit against the Python restatements (shortcut_restatement.py, repair_restatement.py).  Floats
cross the pipe as hex, so nothing is rounded on the way."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import repair_restatement as P
import shortcut_restatement as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")
REV = [0, 0, 1, 1, 1, 1, 1, 1]  # the robotino model's joint_is_revolute: x and y prismatic, then the rotation and the arm
N, F, MAXP = R.N_SEG, R.STEP, P.MAX_POINTS


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("paths") / "paths_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "paths_table.cpp"), os.path.join(CSRC, "smp_paths.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(exe, mode, stdin):
    """The driver's stdout lines; the environment is passed through as it is."""
    p = subprocess.run([exe, mode], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout.splitlines()


def hx(values):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.asarray(values, np.float64).ravel())


def rule(rev=REV, f=F, n=N, maxp=MAXP):
    return "%s %s %d %d" % (" ".join(map(str, rev)), float(f).hex(), n, maxp)


def unhex(tokens):
    return np.array([float.fromhex(t) for t in tokens], np.float64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_robotino_rev(orobot):
    assert [int(bool(r)) for r in orobot.rev] == REV


# ------------------------------------------------------------------------------------------ density
def density_many(exe, a, b, **kw):
    a, b = np.asarray(a, np.float64).reshape(-1, 8), np.asarray(b, np.float64).reshape(-1, 8)
    text = rule(**kw) + "\n" + "".join(hx(a[i]) + " " + hx(b[i]) + "\n" for i in range(len(a)))
    out = [int(line) for line in run(exe, "density", text)]
    assert len(out) == len(a)
    return np.array(out, np.int64)


def restated_segments(a, b, rev=REV, n=N, f=F):
    """repair_restatement.leg_segments with a non-finite coordinate refused, as make_edge refuses it."""
    a, b = np.asarray(a, np.float64).reshape(-1, 8), np.asarray(b, np.float64).reshape(-1, 8)
    M = P.leg_segments(a, b, rev, n, f)
    return np.where(np.isfinite(a).all(1) & np.isfinite(b).all(1), M, 0)


def test_density_named_edges(table):
    z = np.zeros(8)

    def move(j, d):
        q = z.copy()
        q[j] = d
        return q
    last = (MAXP - 1) // N  # the most hops the table admits: N * last <= MAXP - 1 < N * (last + 1)
    cases = [
        (z, z, N),                                   # zero length: one hop
        (z, move(0, 3 * F), 3 * N),                  # exact multiples of the step
        (z, move(4, 3 * F), 3 * N),
        (z, move(0, 1 * F), N),
        (z, move(3, 0.7), 2 * N),                    # revolute only
        (z, move(1, 0.7), 2 * N),                    # prismatic only
        (z, move(0, last * F), last * N),            # the longest edge admitted
        (z, move(0, np.nextafter(last * F, np.inf)), 0),   # one hop more: refused
        (z, move(0, (last + 1) * F), 0),
        (z, move(5, 1.0e300), 0),
        (z, move(2, np.nan), 0),                     # a non-finite coordinate: refused
        (move(7, np.inf), z, 0),
        (move(0, -np.inf), move(0, np.inf), 0),
    ]
    a, b, want = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    got = density_many(table, a, b)
    assert got.tolist() == want
    assert got.tolist() == restated_segments(a, b).tolist()


def test_density_random_edges(table):
    rng = np.random.default_rng(1)
    n = 4000
    a = rng.uniform(-3.0, 3.0, (n, 8))
    b = a + rng.uniform(-1.0, 1.0, (n, 8)) * rng.choice([1e-3, 0.1, 1.0, 10.0, 300.0], (n, 1))
    b[::7, 2:] = a[::7, 2:]   # prismatic only
    b[3::7, :2] = a[3::7, :2]  # revolute only
    for rev, nseg, f in ((REV, N, F), ([1, 0, 1, 0, 0, 1, 1, 0], 31, 0.125), ([0] * 8, 1, 0.3)):
        got = density_many(table, a, b, rev=rev, n=nseg, f=f)
        want = restated_segments(a, b, rev, nseg, f)
        assert (want > 0).all() and len(set(want.tolist())) > 20
        assert np.array_equal(got, want), (rev, nseg, f)


# ------------------------------------------------------------------------------------------ shortcut
def shortcut_case(k, window, share, seed):
    """(waypoints, first[]) of one case: seeded random waypoints; every candidate blocked with probability `share`, at a
    point drawn within its M + 1."""
    rng = np.random.default_rng([k, window, int(share * 10), seed])
    w = np.cumsum(rng.uniform(-0.4, 0.4, (k, 8)), 0)
    pairs = R.candidates(k, window)
    a = np.array([w[i] for i, _ in pairs])
    b = np.array([w[j] for _, j in pairs])
    m, M = R.density(a, b, REV, N, F)
    first = np.where(rng.random(len(pairs)) < share, (rng.random(len(pairs)) * (M + 1)).astype(np.int64), -1)
    return w, pairs, a, b, m, M, first


def test_shortcut(table):
    cases = [shortcut_case(k, window, share, seed)
             for k in (2, 3, 5, 12, 40) for window in (0, 1, 2, k) for share in (0.0, 0.3, 0.7, 1.0) for seed in (0, 1)]
    windows = [window for k in (2, 3, 5, 12, 40) for window in (0, 1, 2, k) for _ in range(8)]
    text = "".join("%s %d %d %s %s\n" % (rule(), len(c[0]), win, hx(c[0]), " ".join(map(str, c[6])))
                   for c, win in zip(cases, windows))
    lines = run(table, "shortcut", text)
    assert len(lines) == len(cases)
    found = blocked = 0
    for (w, pairs, a, b, m, M, first), line in zip(cases, lines):
        exp = R.shortcut_route(w, pairs, a, b, m, M, first, N)
        t = line.split()
        got_int = [int(v) for v in t[:4]]
        assert got_int == [exp["n_edges"], exp["n_valid"], exp["configs_checked"], exp["first_blocked"]], line[:200]
        assert same_bits(unhex(t[4:6]), [exp["cost_in"], exp["cost_out"]])
        rows = int(t[6])
        if exp["path"] is None:
            blocked += 1
            assert rows == 0 and len(t) == 7
            assert exp["first_blocked"] >= 0
        else:
            found += 1
            assert rows == len(exp["path"])
            assert same_bits(unhex(t[7:]).reshape(rows, 8), exp["path"])
    assert found >= 20 and blocked >= 20, (found, blocked)


def test_shortcut_refuses_what_make_edge_refuses(table):
    w = np.zeros((3, 8))
    w[1, 0] = np.nan
    assert run(table, "shortcut", "%s 3 0 %s -1 -1 -1\n" % (rule(), hx(w))) == ["refused"]


# ------------------------------------------------------------------------------------------ gaps
def gap_patterns(k):
    """Every valid[] with both ends valid, and with each every first[] consistent with it: an edge with an invalid
    endpoint is blocked (at its first or last point), any other edge is free or blocked in between."""
    for inner in itertools.product((1, 0), repeat=k - 2):
        valid = (1,) + inner + (1,)
        free_choice = [i for i in range(k - 1) if valid[i] and valid[i + 1]]
        for bits in itertools.product((-1, 3), repeat=len(free_choice)):
            first = [0 if not valid[i] else N for i in range(k - 1)]
            for i, f in zip(free_choice, bits):
                first[i] = f
            yield valid, first


def test_gaps_exhaustive(table):
    cases = [c for k in range(2, 9) for c in gap_patterns(k)]
    text = "".join("%d %s %s\n" % (len(v), " ".join(map(str, v)), " ".join(map(str, f))) for v, f in cases)
    lines = run(table, "gaps", text)
    assert len(lines) == len(cases)
    merged = runs = touch_first = touch_last = 0
    for (valid, first), line in zip(cases, lines):
        parts = [[int(x) for x in part.split()] for part in line.split(";")]
        exp = P.find_gaps(valid, first)
        n_blocked = sum(f >= 0 for f in first)
        assert parts[0] == [n_blocked, len(exp)], (valid, first, line)
        assert parts[1:] == exp, (valid, first, line)
        for l, r, e in exp:
            assert valid[l] and valid[r] and l <= e < r and not any(valid[l + 1:r])
            runs += r - l > 2  # two invalid waypoints or more between the anchors
            touch_first += l == 0
            touch_last += r == len(valid) - 1
        merged += n_blocked > len(exp)
    assert merged > 0 and runs > 0 and touch_first > 0 and touch_last > 0


# ------------------------------------------------------------------------------------------ detour choice, repaired rows
def repair_case(k, samples, share, seed, ties):
    """(waypoints, gaps, free flags, vias) of one case: seeded waypoints, validity and blocked edges; per gap `samples`
    vias around its centre, each free with probability `share`.  With ties the vias of a gap repeat, so that several
    free items cost the same to the bit."""
    rng = np.random.default_rng([k, samples, int(share * 10), seed, int(ties)])
    w = np.cumsum(rng.uniform(-0.4, 0.4, (k, 8)), 0)
    valid = np.concatenate([[1], (rng.random(k - 2) < 0.7).astype(int), [1]])
    first = [-1 if valid[i] and valid[i + 1] and rng.random() < 0.6 else 1 for i in range(k - 1)]
    gaps = P.find_gaps(valid, first)
    free, vias = [], []
    for l, r, _ in gaps:
        c = 0.5 * (w[l] + w[r])
        v = c[None, :] + rng.uniform(-0.5, 0.5, (samples, 8))
        if ties:
            v = v[np.arange(samples) % max(1, samples // 3)]
        vias.append(v)
        free.append((rng.random(samples) < share).astype(int))
    return w, gaps, free, vias


def test_detour_choice_and_repaired_rows(table):
    cases = [repair_case(k, samples, share, seed, ties)
             for k in (2, 3, 6, 17) for samples in (1, 4, 9) for share in (0.0, 0.3, 1.0) for seed in (0, 1, 2)
             for ties in (False, True)]
    text = ""
    for w, gaps, free, vias in cases:
        text += "%s %d %d %d %s" % (rule(), len(w), len(free[0]) if free else 1, len(gaps), hx(w))
        for g, (l, r, e) in enumerate(gaps):
            text += " %d %d %d" % (l, r, e)
            for s in range(len(free[g])):
                text += " %d %s" % (free[g][s], hx(vias[g][s]))
        text += "\n"
    lines = run(table, "repair", text)
    assert len(lines) == len(cases)
    repaired = left_open = tie_broken = 0
    for (w, gaps, free, vias), line in zip(cases, lines):
        head, tail = line.split(";")
        chosen_idx = [int(v) for v in head.split()]
        exp_idx = [P.choose_detour(w[l], w[r], free[g], vias[g]) for g, (l, r, _) in enumerate(gaps)]
        assert chosen_idx == exp_idx
        for g, s in enumerate(exp_idx):  # a tie in cost goes to the first
            if s >= 0:
                l, r, _ = gaps[g]
                costs = [P.dist(w[l], v) + P.dist(v, w[r]) for v in vias[g]]
                same = [t for t in range(len(costs)) if free[g][t] and costs[t] == costs[s]]
                assert s == same[0]
                tie_broken += len(same) > 1
        chosen = [vias[g][s] if s >= 0 else None for g, s in enumerate(exp_idx)]
        t = tail.split()
        n_free, first_blocked, rows = int(t[0]), int(t[1]), int(t[3])
        assert n_free == sum(int(f.sum()) for f in free)
        assert first_blocked == P.first_open_gap(gaps, chosen)
        if first_blocked >= 0:
            left_open += 1
            assert rows == 0 and float.fromhex(t[2]) == 0.0
            assert first_blocked == [gaps[g][2] for g in range(len(gaps)) if chosen[g] is None][0]
            continue
        repaired += len(gaps) > 0
        route, exp_rows, cost_out = P.repaired_route(w, gaps, chosen, REV, N, F)
        assert same_bits(float.fromhex(t[2]), cost_out)
        assert rows == len(exp_rows)
        assert same_bits(unhex(t[4:]).reshape(rows, 8), exp_rows)
    assert repaired >= 10 and left_open >= 10 and tie_broken >= 10, (repaired, left_open, tie_broken)
