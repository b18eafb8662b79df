"""The cost field on the CPU: the HIP-free unit (csrc/smp_field.h, smp_field_host.cpp: the tile geometry, the round cap,
the fallback test and the host forms of the parents, the chain and the settled count) through a stand-alone ASAN / UBSAN
driver against field_restatement.py; the claims the device method rests on (the parent rule and the settled count follow
from the field alone), and the conditions test_gpu_field.py rests on, asserted on the restatement alone."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import field_restatement as F
import lattice_restatement as T
from conftest import ROOT
from squirrel_motion_planner_amd import _lib as L

CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")
hx = lambda v: float(v).hex()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("field") / "field_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "field_table.cpp"), os.path.join(CSRC, "smp_field_host.cpp"),
           os.path.join(CSRC, "smp_route.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(table, text):
    p = subprocess.run([table], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout.split()


# ------------------------------------------------------------------------------------------ the host unit
def case_text(lat, free, frm, to, snap, cost):
    words = T.pack(free)
    head = [hx(lat.x0), hx(lat.y0), hx(lat.pitch), lat.nx, lat.ny, hx(lat.theta0), hx(lat.dtheta), lat.n_theta,
            lat.wrap_theta] + [hx(a) for a in lat.arm] + [hx(v) for v in frm] + [hx(v) for v in to] + [snap, len(words)]
    return "C " + " ".join(str(v) for v in head) + "\n" + " ".join(str(int(w)) for w in words) + "\n" + \
        " ".join(hx(v) for v in cost) + "\n"


def test_host_forms_on_every_map(table):
    """field_parent / field_chain / field_settled on the restatement's cost array: smp_base_route's chain, cost and
    n_settled, and the restatement's parents."""
    names = list(F.maps())
    tok = run(table, "".join(case_text(*F.maps()[k], F.expected(k)["cost"]) for k in names))
    for k in names:
        lat, free = F.maps()[k][:2]
        e = F.expected(k)
        r = e["route"]
        st, same, s_route, s_field, reached = [int(tok.pop(0)) for _ in range(5)]
        cost_to = float.fromhex(tok.pop(0))
        n_chain = int(tok.pop(0))
        chain = np.array([int(tok.pop(0)) for _ in range(3 * n_chain)], np.int32).reshape(-1, 3)
        parent = np.array([int(tok.pop(0)) for _ in range(T.n_nodes(lat))], np.int32)
        assert st == r["status"], k
        assert s_route == s_field == r["n_settled"] == F.settled_count(e["cost"], e["to"]), k
        assert reached == len(e["order"]), k
        assert np.array_equal(parent, e["parent"]), k
        if st == T.OK:
            assert same == 1 and np.array_equal(chain, r["chain"]) and hx(cost_to) == hx(r["cost"]), k
        else:
            assert st == T.ERR_NO_SOLUTION and n_chain == 0 and cost_to == F.INF, k
    assert not tok


GEOMETRY = [(1, 1, 1, 0), (F.B - 1, F.B + 1, 3, 1), (2 * F.B + 1, F.B, F.BT + 1, 1), (2 * F.B + 1, F.B, F.BT + 1, 0),
            (F.B + 1, 2 * F.B + 3, 2 * F.BT, 1), (3, 3, 2 * F.BT + 1, 1), (F.B, F.B, F.BT, 1), (5, 4, 2, 1), (5, 4, 1, 1)]


def test_tile_geometry(table):
    """The tiles cover each node once, and a change activates exactly the tiles whose halo holds the node."""
    tok = [int(v) for v in run(table, "".join("G %d %d %d %d\n" % g for g in GEOMETRY))]
    for nx, ny, nt, wrap in GEOMETRY:
        lat = F.grid_lattice(nx, ny, nt, wrap)
        n = tok.pop(0)
        assert n == F.n_tiles(lat)
        owner = np.full((nt, ny, nx), -1)
        for tile in range(n):
            x0, y0, t0, ex, ey, et = [tok.pop(0) for _ in range(6)]
            assert 1 <= ex <= F.BX and 1 <= ey <= F.BY and 1 <= et <= F.BT
            assert (owner[t0:t0 + et, y0:y0 + ey, x0:x0 + ex] == -1).all()
            owner[t0:t0 + et, y0:y0 + ey, x0:x0 + ex] = tile
        assert (owner >= 0).all()
        for t in range(nt):
            for y in range(ny):
                for x in range(nx):
                    tile, k = tok.pop(0), tok.pop(0)
                    act = [tok.pop(0) for _ in range(k)]
                    assert tile == owner[t, y, x] == F.tile_of(lat, x, y, t)
                    assert act == F.activates(lat, x, y, t), (nx, ny, nt, wrap, x, y, t)
    assert not tok


def test_round_zero_runs_the_source_tile_and_every_tile_whose_halo_holds_the_source(table):
    """The source is never lowered, so nothing but the start flags its neighbours: on every map and on rim, corner and
    wrap positions of the geometry cases the start set is the source's tile and field_restatement.activates' tiles."""
    cases = [(v[0], F.expected(k)["route"]["from_node"]) for k, v in F.maps().items()]
    for nx, ny, nt, wrap in GEOMETRY:
        lat = F.grid_lattice(nx, ny, nt, wrap)
        cases += [(lat, (x, y, t)) for x in {0, min(F.B - 1, nx - 1), nx - 1} for y in {0, min(F.B, ny - 1), ny - 1}
                  for t in {0, min(F.BT - 1, nt - 1), nt - 1}]
    tok = [int(v) for v in run(table, "".join("S %d %d %d %d %d %d %d\n" % (l.nx, l.ny, l.n_theta, l.wrap_theta, *s)
                                              for l, s in cases))]
    for lat, s in cases:
        k = tok.pop(0)
        assert [tok.pop(0) for _ in range(k)] == sorted([F.tile_of(lat, *s)] + F.activates(lat, *s)), (lat, s)
    assert not tok


def test_geometry_cases_hold_every_kind():
    """A tile that wraps inside itself, two tiles that are each other's both heading neighbours, a one-layer last tile."""
    act = lambda g, x, y, t: F.activates(F.grid_lattice(*g), x, y, t)
    assert act((F.B, F.B, F.BT, 1), 3, 3, 0) == []                         # one tile: the wrap stays inside
    assert act((F.B + 1, 2 * F.B + 3, 2 * F.BT, 1), 3, 3, 0) == [6]        # heading 0's lower neighbour is the top tile
    assert act((2 * F.B + 1, F.B, F.BT + 1, 1), 3, 3, F.BT) == [0]         # the one-layer tile: both ways the same tile
    assert act((2 * F.B + 1, F.B, F.BT + 1, 0), 3, 3, 0) == []
    assert len(act((F.B + 1, 2 * F.B + 3, 2 * F.BT, 0), F.B - 1, F.B - 1, F.BT - 1)) == 4   # a corner and a layer above


def test_fallback_predicate_and_round_cap(table):
    cases = [(0.0, 0.25, 0.5, 1), (1e3, 0.25, 0.5, 8), (2.0 ** 53, 0.25, 0.5, 1), (2.0 ** 51, 0.25, 1e-9, 8),
             (2.0 ** 51, 0.5, 1e-9, 1), (2.0 ** 51, 0.26, 0.3, 8), (F.INF, 0.25, 0.5, 1)]
    tok = run(table, "".join("U %s %s %s %d\n" % (hx(c), hx(p), hx(d), nt) for c, p, d, nt in cases) + "K 0\nK 41\n")
    exp = [int(F.unique(c, F.grid_lattice(1, 1, nt, 0, p, d))) for c, p, d, nt in cases]
    assert [int(v) for v in tok[:len(cases)]] == exp == [1, 1, 0, 0, 1, 1, 0]
    assert [int(v) for v in tok[len(cases):]] == [1, 42]


# ------------------------------------------------------------------------------------------ what the method rests on
def test_the_field_alone_gives_parents_and_settle_order():
    """The issue's claims, on every map: the search's parent is the candidate with the least (cost, node), and a node's
    place in the settle order is its rank by (cost, node)."""
    for k in F.maps():
        lat, free = F.maps()[k][:2]
        e = F.expected(k)
        assert np.array_equal(F.parent_rule(lat, free, e["cost"]), e["parent"]), k
        assert e["order"] == sorted(e["order"], key=lambda n: (e["cost"][n], n)), k


def test_any_relaxation_order_reaches_the_field():
    """An in-place relaxation in random order from +inf ends at the search's bits."""
    rng = random.Random(3)
    for k in ("random", "door_in_another_layer", "open_%dx%dx3_w1" % (F.B + 1, F.B - 1)):
        lat, free = F.maps()[k][:2]
        free = np.asarray(free, bool)
        e = F.expected(k)
        cost = np.full(T.n_nodes(lat), F.INF)
        cost[e["src"]] = 0.0
        nodes = [int(n) for n in np.flatnonzero(free.reshape(-1))]
        nbrs = {n: F.neighbours(lat, free, *F.split(lat, n)) for n in nodes}
        changed = True
        while changed:
            changed = False
            rng.shuffle(nodes)
            for n in nodes:
                c = min([float(cost[u]) + w for u, w in nbrs[n]] + [float(cost[n])])
                if c < cost[n]:
                    cost[n], changed = c, True
        assert np.array_equal(cost.view(np.uint64), e["cost"].view(np.uint64)), k


# ------------------------------------------------------------------------------------------ non-vacuity
def test_maps_hold_what_the_gpu_tests_rest_on():
    m = F.maps()
    # ties: a node with two or more parent candidates
    lat, free = m["open_%dx%dx3_w1" % (F.B + 1, F.B - 1)][:2]
    cost = F.expected("open_%dx%dx3_w1" % (F.B + 1, F.B - 1))["cost"]
    assert max(len(F.parent_candidates(lat, free, cost, n)) for n in range(len(cost))) >= 2
    # the maze's route is long and re-enters tiles
    r = F.expected("maze")["route"]
    assert r["status"] == T.OK and len(r["chain"]) - 1 > 4 * F.B and F.n_tiles(m["maze"][0]) >= 9
    tiles = [F.tile_of(m["maze"][0], *c) for c in r["chain"]]
    assert sum(a != b for a, b in zip(tiles, tiles[1:])) > 3 * F.n_tiles(m["maze"][0])
    # The random map.  Nodes are free independently; at a free share of 0.3 no seed of several thousand reaches half of
    # the free nodes, and at 0.7 every seed reaches 99 % of them, so the share is the one between at which both of the
    # conditions below hold.
    lat, free = m["random"][:2]
    e = F.expected("random")
    n_free, reached = int(np.asarray(free).sum()), len(e["order"])
    assert F.n_tiles(lat) == 8 and n_free - reached > 0.1 * n_free and reached > 0.5 * n_free
    assert e["route"]["status"] == T.OK
    # the other cases are what their names say
    assert len(F.expected("isolated_source")["order"]) == 1
    assert F.expected("isolated_source")["route"]["status"] == T.ERR_NO_SOLUTION
    u = F.expected("unreachable_to")
    assert u["route"]["status"] == T.ERR_NO_SOLUTION and u["route"]["n_settled"] == len(u["order"]) > 1
    assert len(F.expected("from_is_to")["route"]["chain"]) == 1
    assert sorted(set(F.expected("door_in_another_layer")["route"]["chain"][:, 2].tolist())) == [0, 1, 2]
    d = F.expected("forbidden_diagonal_on_a_tile_corner")["route"]
    lat = m["forbidden_diagonal_on_a_tile_corner"][0]
    assert len(d["chain"]) == 3 and d["cost"] == lat.pitch + lat.pitch
    s = m["source_in_the_last_partial_tile"][0]
    assert F.tile_of(s, *F.expected("source_in_the_last_partial_tile")["route"]["from_node"]) == F.n_tiles(s) - 1
    # sources whose only way on lies in another tile: every free neighbour of the source is in a tile that is not its own
    for k in ("corridor_from_the_seam", "headings_from_the_seam", "headings_through_the_wrap", "source_on_a_tile_corner"):
        lat, free = m[k][:2]
        e = F.expected(k)
        src = e["route"]["from_node"]
        nb = F.neighbours(lat, np.asarray(free, bool), *src)
        mates = [u for u, _ in nb if F.tile_of(lat, *F.split(lat, u)) == F.tile_of(lat, *src)]
        assert e["route"]["status"] == T.OK and nb, k
        if k in ("headings_through_the_wrap", "source_on_a_tile_corner"):
            assert not mates, k
        assert F.tile_of(lat, *e["route"]["to_node"]) != F.tile_of(lat, *src) or k == "source_on_a_tile_corner", k
    # (the two seam sources have tile mates, all behind them: none of them lies on the seam the route crosses)
    assert F.expected("corridor_from_the_seam")["route"]["from_node"] == (F.B - 1, 0, 0)
    assert F.ONE_TILE and all(F.n_tiles(m[k][0]) == 1 for k in F.ONE_TILE)
    assert any(m[k][0].wrap_theta and m[k][0].n_theta > 1 for k in F.ONE_TILE)
    assert all(T.n_nodes(v[0]) < 20000 for v in m.values())


# ------------------------------------------------------------------------------------------ the ABI without a GPU
def test_tile_shape_is_the_mirrors():
    t = (ctypes.c_int * 3)()
    L.lib().smp_field_tile_shape(t)
    assert tuple(t) == L.FIELD_TILE


def test_far_opts_default_leaves_the_route_on_the_host():
    o = L.FarOpts()
    o.route_device = 7
    L.lib().smp_far_opts_default(ctypes.byref(o))
    assert o.route_device == 0 and o.snap_cells == 2 and o.pitch == 0.1
    assert ctypes.sizeof(L.FarOpts) == 88 and L.FarOpts.route_device.offset == 80
    assert ctypes.sizeof(L.FieldInfo) == 56 and L.FieldInfo.tile_runs.offset == 32


def test_null_arguments_are_refused_before_any_device_call():
    lib = L.lib()
    lat = L.BaseLattice(0.0, 0.0, 0.1, 2, 2, 0.0, 0.5, 1, 0, (ctypes.c_double * 5)(*T.ARM))
    bits = (ctypes.c_uint32 * 1)(15)
    src = (ctypes.c_int32 * 3)(0, 0, 0)
    info = L.FieldInfo()
    assert lib.smp_base_cost_field(None, ctypes.byref(lat), bits, src, None, None, ctypes.byref(info)) == L.SMP_ERR_ARG
    a = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    rows, n_out, rinfo = ctypes.POINTER(ctypes.c_double)(), ctypes.c_int64(5), L.RouteInfo()
    rc = lib.smp_base_route_gpu(None, ctypes.byref(lat), bits, a, a, 0, ctypes.byref(rows), ctypes.byref(n_out), None,
                                ctypes.byref(rinfo), ctypes.byref(info))
    assert rc == L.SMP_ERR_ARG and n_out.value == 0 and not rows and tuple(rinfo.from_node) == (-1, -1, -1)
