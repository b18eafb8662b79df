"""The provisioning unit (csrc/smp_provision.cpp: PlanKnobs and provision) on the CPU, built with ASAN / UBSAN and
driven by tests/cpp/provision_table.cpp: a sweep against the Python restatement (tests/provision_restatement.py), the
rule's invariants on every case, hand-derived cases and the SMP_* knobs' defaults and clamps."""
import itertools
import os
import subprocess

import pytest

import provision_restatement as PR
from conftest import ROOT

CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")

SLOTS = [1, 4, 6, 18, 64, 104, 256, 512]
QUERIES = [1, 2, 3, 7, 8, 9, 16, 64]
HELPERS = [-1, 0, 1, 3, 4, 15, 16, 63, 250]
SCOUT = [0, 1, 2, 3, 4, 9]
SHARE = [1, 2]
PATTERNS = ["clear", "set", "alternating"]


def have_sol(pattern, n):
    return [{"clear": 0, "set": 1, "alternating": i & 1}[pattern] for i in range(n)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("provision") / "provision_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "cpp", "provision_table.cpp"),
           os.path.join(CSRC, "smp_provision.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, args=(), stdin="", env=None):
    """The driver's stdout; its environment holds no SMP_* variable but those of `env`."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("SMP_")}
    e.pop("LD_PRELOAD", None) if "asan" in e.get("LD_PRELOAD", "") else None  # as test_host_sanitize_cpu.py
    e.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    e.update(env or {})
    p = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout


def provision_many(exe, cases, env=None):
    """cases: (slots, num_cus, num_xcd, slot_share, helpers, scout, have_sol) -> what PR.provision returns, per case."""
    text = "".join("%d %d %d %d %d %d %d %s\n" % (c[0], c[1], c[2], c[3], c[4], c[5], len(c[6]),
                                                   " ".join(map(str, c[6]))) for c in cases)
    lines = run(exe, stdin=text, env=env).splitlines()
    assert len(lines) == len(cases)
    out = []
    for line in lines:
        parts = [[int(v) for v in part.split()] for part in line.split(";")]
        nh, ns, ns_base = parts[0]
        out.append((nh, ns, ns_base, [(q[0], q[1], q[2], q[3:]) for q in parts[1:]]))
    return out


def sweep_cases():
    cases = []
    for slots, nq, h, sc, share, pat in itertools.product(SLOTS, QUERIES, HELPERS, SCOUT, SHARE, PATTERNS):
        cases.append((slots, 256, 8, share, h, sc, have_sol(pat, nq)))
    n_mi355x = len(cases)
    for slots, nq, h, sc, pat in itertools.product(SLOTS, QUERIES, HELPERS, SCOUT, PATTERNS):  # a device of one XCD
        cases.append((slots, 64, 1, 1, h, sc, have_sol(pat, nq)))
    return cases, n_mi355x


def test_sweep_matches_restatement_and_keeps_invariants(table):
    cases, n_mi355x = sweep_cases()
    assert n_mi355x == 20736
    got = provision_many(table, cases)
    for c, g in zip(cases, got):
        slots, num_cus, num_xcd, share, h, sc, sol = c
        assert g == PR.provision(slots, num_cus, num_xcd, share, h, sc, sol), c
        nh, ns, ns_base, queries = g
        assert len(queries) == len(sol)
        assert 1 + ns + nh <= max(1, slots // len(sol)), (c, g)
        if nh < 4:
            assert ns == 0, (c, g)
        for nscouts, nworkers, sampler, sw in queries:
            assert len(sw) == ns
            if nscouts > 0:
                assert (nworkers - 1) + sum(w - 1 for w in sw) + 1 == nh, (c, g)


MI355X = (256, 256, 8, 1, 0, 1)  # 256 slots, 256 CUs, 8 XCDs, share 1, automatic helpers, scout 1


def test_one_unsolved_query(table):
    (got,) = provision_many(table, [MI355X + ([0],)])
    assert got == (200, 4, 4, [(4, 67, 1, [56, 55, 13, 13])])


def test_eight_queries_second_solved(table):
    sol = [0, 1, 0, 0, 0, 0, 0, 0]
    (got,) = provision_many(table, [MI355X + (sol,)])
    nh, ns, ns_base, queries = got
    assert (nh, ns, ns_base) == (26, 4, 2)
    for i, q in enumerate(queries):
        if sol[i]:
            assert q == (2, 9, 1, [10, 9, 1, 1])
        else:
            assert q == (4, 6, 1, [6, 6, 6, 6])


def test_no_active_query_provisions_as_for_one(table):
    """n_act == 0 (the driver never sends it: with no query to launch it provisions all of them): the launch-wide counts
    of one query, no per-query record, and no unsolved query to raise two scouts to four."""
    cases = [(slots, 256, 8, share, h, sc, []) for slots, h, sc, share in itertools.product(SLOTS, HELPERS, SCOUT, SHARE)]
    got = provision_many(table, cases)
    for c, g in zip(cases, got):
        assert g == PR.provision(*c), c
    assert got[cases.index(MI355X + ([],))] == (200, 4, 4, [])
    assert got[cases.index((18, 256, 8, 1, 0, 1, []))] == (15, 2, 2, [])  # (one unsolved query there: 13 4 2)
    assert provision_many(table, [(18, 256, 8, 1, 0, 1, [0])])[0][:3] == (13, 4, 2)


@pytest.mark.parametrize("margin, want", [(26, (8, 4)), (29, (0, 0, 0)), (64, (0, 0, 0))])
def test_xcd_margin(table, margin, want):
    (got,) = provision_many(table, [MI355X + ([0],)], env={"SMP_XCD_MARGIN": str(margin)})
    assert got[:len(want)] == want
    assert got == PR.provision(*MI355X, [0], knobs={"xcd_margin": margin})


def knobs(exe, helpers=0, nq=1, env=None):
    out = {}
    for line in run(exe, ["knobs", str(helpers), str(nq)], env=env).splitlines():
        name, value = line.split()
        out[name] = float(value) if name in ("slice_ms", "wait_slack_s") else int(value)
    return out


DEFAULTS = dict(tile_ct=0, scan_min=12288, scan_pnn=64, scan_pnear=32, scan_nshift=12, scan_ps0=0, helper_cap=200,
                lead_div=3, pre_lead_div=5, pre_helpers=12, pre_delay=3, early_ask=0, pre_refresh=1, conn_check=0,
                pre_commit=1, pre_scouts=1, rebalance=1, rebalance_div=4, slice_ms=50.0, xcd_margin=1,
                wait_slack_s=60.0, chunk0=1 << 30, host_prof=0, debug=0, debug_scouts=0, bounds=0)


def test_knob_defaults(table):
    assert knobs(table) == DEFAULTS
    assert knobs(table, helpers=12) == dict(DEFAULTS, rebalance=0)
    assert knobs(table, nq=8) == DEFAULTS                                      # time slices: one launch's chunk is open
    assert knobs(table, nq=8, env={"SMP_SLICE_MS": "0"}) == dict(DEFAULTS, slice_ms=0.0, chunk0=256)
    assert knobs(table, nq=1, env={"SMP_SLICE_MS": "0"}) == dict(DEFAULTS, slice_ms=0.0)


@pytest.mark.parametrize("var, value, name, want", [
    ("SMP_TILE_CT", "3", "tile_ct", 0), ("SMP_TILE_CT", "8", "tile_ct", 8),
    ("SMP_SCAN_MIN", "-5", "scan_min", 0),
    ("SMP_SCAN_PNN", "1000", "scan_pnn", 64), ("SMP_SCAN_PNN", "0", "scan_pnn", 2),
    ("SMP_SCAN_PNEAR", "1000", "scan_pnear", 32), ("SMP_SCAN_PNEAR", "-3", "scan_pnear", 2),
    ("SMP_SCAN_NSHIFT", "2", "scan_nshift", 6), ("SMP_SCAN_NSHIFT", "40", "scan_nshift", 20),
    ("SMP_SCAN_PS0", "-1", "scan_ps0", 0), ("SMP_SCAN_PS0", "9", "scan_ps0", 4),
    ("SMP_HELPER_CAP", "0", "helper_cap", 1),
    ("SMP_LEAD_DIV", "0", "lead_div", 1),
    ("SMP_PRE_LEAD_DIV", "-2", "pre_lead_div", 1),
    ("SMP_PRE_HELPERS", "-4", "pre_helpers", 0),
    ("SMP_REBALANCE_DIV", "0", "rebalance_div", 1),
    ("SMP_SLICE_MS", "-1.5", "slice_ms", 0.0),
    ("SMP_XCD_MARGIN", "-7", "xcd_margin", 0),
    ("SMP_CHUNK0", "0", "chunk0", 1),
    ("SMP_PRE_DELAY", "-2", "pre_delay", -2),  # as given
    ("SMP_WAIT_SLACK_S", "0.25", "wait_slack_s", 0.25),
    ("SMP_REBALANCE", "0", "rebalance", 0),
    ("SMP_DEBUG", "", "debug", 1), ("SMP_HOST_PROF", "0", "host_prof", 1),
    ("SMP_DEBUG_SCOUTS", "1", "debug_scouts", 1), ("SMP_BOUNDS", "1", "bounds", 1),
])
def test_knob_clamps(table, var, value, name, want):
    assert knobs(table, env={var: value})[name] == want


def test_rebalance_cannot_be_turned_on(table):
    assert knobs(table, helpers=12, env={"SMP_REBALANCE": "1"})["rebalance"] == 0
    assert knobs(table, helpers=0, env={"SMP_REBALANCE": "1"})["rebalance"] == 1
