"""Attached objects on the CPU: smp_robot_attach against the JSON path on an independently augmented model
(attach_restatement.py), its pair and error rules, the sphere covers, and the HIP-free unit (csrc/smp_attach.cpp with
csrc/smp_host.cpp) through a stand-alone ASAN / UBSAN driver (tests/cpp/attach_table.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import attach_restatement as A
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import Robot, cover_box, cover_cylinder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squirrel_motion_planner_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
HAND = A.HAND


@pytest.fixture(scope="module")
def base():
    return A.base_model()


def _json_robot(model, tmp_path, tag):
    return Robot(model_json=A.write_json(model, str(tmp_path / ("aug_%s.json" % tag))))


def test_restatement_reproduces_the_committed_cb(base):
    ok, n = A.committed_cb_reproduced(base)
    assert n == 50 and ok == n


@pytest.mark.parametrize("n", [2, 10, 16])
def test_attach_equals_the_json_path(base, tmp_path, n):
    c, r = A.bar(n)
    got = Robot().attach(HAND, c, r)
    want = _json_robot(A.augmented(base, HAND, c, r), tmp_path, n)
    assert got.link_names == want.link_names and got.link_names[-1] == "attached_object"
    assert got.device_bytes() == want.device_bytes()
    assert Robot().device_bytes() != got.device_bytes()


def test_attach_on_a_urdf_built_robot(base, tmp_path):
    urdf = open(os.path.join(GOLD, "robotino_plan.urdf")).read()
    srdf = open(os.path.join(GOLD, "robotino_plan.srdf")).read()
    c, r = A.bar(10)
    got = Robot.from_urdf(urdf, srdf).attach(HAND, c, r)
    want = _json_robot(A.augmented(base, HAND, c, r), tmp_path, "urdf")
    assert got.link_names == want.link_names
    assert got.device_bytes() == want.device_bytes()


def test_two_successive_attaches(base, tmp_path):
    """The result of an attach takes a further object: a second one on another body (and so paired with the first)."""
    c1, r1 = A.bar(2)
    c2, r2 = [(0.0, 0.0, 0.30), (0.05, 0.0, 0.30)], [0.04, 0.05]
    got = Robot().attach(HAND, c1, r1).attach("base_link", c2, r2, name="tray")
    m = A.augmented(A.augmented(base, HAND, c1, r1), "base_link", c2, r2, name="tray")
    names = [e["name"] for e in m["links"]]
    assert [names.index("attached_object"), names.index("tray")] in m["self_pairs"]
    want = _json_robot(m, tmp_path, "two")
    assert got.link_names == want.link_names and got.link_names[-2:] == ["attached_object", "tray"]
    assert got.device_bytes() == want.device_bytes()


def test_pair_rules(base, tmp_path):
    """14 new pairs without touch links, in lexicographic order; touch links remove exactly their pairs."""
    c, r = A.bar(2)
    m = A.augmented(base, HAND, c, r)
    new = len(base["links"])
    added = [p for p in m["self_pairs"] if p[1] == new]
    assert len(m["self_pairs"]) == len(base["self_pairs"]) + 14 == 179 and len(added) == 14
    assert m["self_pairs"] == sorted(m["self_pairs"]) and base["self_pairs"] == sorted(base["self_pairs"])
    assert [p for p in m["self_pairs"] if p[1] != new] == base["self_pairs"]
    names = [e["name"] for e in base["links"]]
    touch = [names[added[0][0]], names[added[5][0]]]
    mt = A.augmented(base, HAND, c, r, touch_links=touch)
    assert [p for p in m["self_pairs"] if p not in mt["self_pairs"]] == [added[0], added[5]]
    got = Robot().attach(HAND, c, r, touch_links=touch)
    assert got.device_bytes() == _json_robot(mt, tmp_path, "touch").device_bytes()
    assert got.device_bytes() != Robot().attach(HAND, c, r).device_bytes()
    # the library's own count: sphere pairs grow by the partners' spheres times the object's
    b, a, t = Robot().self_rounds_info(), Robot().attach(HAND, c, r).self_rounds_info(), got.self_rounds_info()
    assert a["n_sph"] == b["n_sph"] + 2 and a["n_spairs"] + a["n_ppairs"] > t["n_spairs"] + t["n_ppairs"] > b["n_spairs"] + b["n_ppairs"]


def test_self_round_regimes():
    """A2 (58 items) keeps the self rounds, A10 (66 items) runs two items per lane and the flat lists."""
    a2, a10 = Robot().attach(HAND, *A.bar(2)).self_rounds_info(), Robot().attach(HAND, *A.bar(10)).self_rounds_info()
    assert a2["n_sph"] + a2["n_prim"] == 58 and a2["qualifies"] == 1
    assert a10["n_sph"] + a10["n_prim"] == 66 and a10["qualifies"] == 0


def _status(link=HAND, name="attached_object", centres=((0.0, 0.0, 0.1),), radii=(0.05,), touch=(), robot=None):
    try:
        (robot or Robot()).attach(link, centres, radii, name, touch)
    except L.SmpError as e:
        return e.status
    return L.SMP_OK


def test_attach_errors():
    nan, inf = float("nan"), float("inf")
    assert _status() == L.SMP_OK
    assert _status(link="no_such_link") == L.SMP_ERR_ARG
    assert _status(name=HAND) == L.SMP_ERR_ARG
    assert _status(name="") == L.SMP_ERR_ARG
    assert _status(touch=("no_such_link",)) == L.SMP_ERR_ARG
    assert _status(touch=("base_link_origin",)) == L.SMP_ERR_ARG  # a link without collision geometry
    assert _status(link="base_link_origin") == L.SMP_ERR_ARG       # no planning joint above it
    assert _status(centres=(), radii=()) == L.SMP_ERR_ARG
    for bad in (nan, inf, -inf):
        assert _status(centres=((0.0, bad, 0.1),)) == L.SMP_ERR_ARG
        assert _status(radii=(bad,)) == L.SMP_ERR_ARG
    for bad in (0.0, -0.05, 0.46):
        assert _status(radii=(bad,)) == L.SMP_ERR_ARG
    assert _status(radii=(0.45,)) == L.SMP_OK
    # a duplicate of an attached object's own name
    one = Robot().attach(HAND, *A.bar(2))
    assert _status(robot=one) == L.SMP_ERR_ARG and _status(robot=one, name="second") == L.SMP_OK
    # NULL arguments of the C call
    h = ctypes.c_void_p()
    assert L.lib().smp_robot_attach(None, ctypes.byref(L.Attach()), ctypes.byref(h)) == L.SMP_ERR_ARG
    assert L.lib().smp_robot_attach(Robot().h, None, ctypes.byref(h)) == L.SMP_ERR_ARG
    assert L.lib().smp_robot_attach(Robot().h, ctypes.byref(L.Attach()), ctypes.byref(h)) == L.SMP_ERR_ARG


def test_attach_capacity():
    assert _status(centres=A.bar(16)[0], radii=A.bar(16)[1]) == L.SMP_OK
    assert _status(centres=A.bar(17)[0], radii=A.bar(17)[1]) == L.SMP_ERR_CAPACITY  # sphere pairs: 768
    assert _status(centres=A.bar(23)[0], radii=A.bar(23)[1]) == L.SMP_ERR_CAPACITY  # spheres: 72
    # collision links: 27 of 32, so the sixth object no longer fits
    r = Robot()
    for k in range(5):
        r = r.attach("base_link", [(0.0, 0.0, 0.3)], [0.03], name="o%d" % k)
    assert _status(robot=r, link="base_link", name="o5") == L.SMP_ERR_CAPACITY
    base = Robot().device_bytes()
    assert Robot().device_bytes() == base  # the base robot is untouched by all of the above


# ------------------------------------------------------------------------------------------ covers
def _inside_some(points, centres, radii):
    d = np.linalg.norm(points[:, None, :] - centres[None, :, :], axis=2)
    return (d <= radii[None, :]).any(axis=1)


@pytest.mark.parametrize("half,tol,mx", [((0.03, 0.03, 0.10), 0.01, 16), ((0.2, 0.05, 0.02), 0.005, 16),
                                         ((0.05, 0.3, 0.05), 0.002, 6), ((0.04, 0.04, 0.04), 0.02, 16)])
def test_cover_box(half, tol, mx):
    c, r = cover_box(half, tol=tol, max_spheres=mx)
    ax = int(np.argmax(half))
    o = [half[i] for i in range(3) if i != ax]
    m, pos, rad = A.cover_formula(half[ax], math.sqrt(o[0] * o[0] + o[1] * o[1]), tol, mx)
    assert len(c) == len(r) == m <= mx
    assert np.array_equal(c[:, ax], np.array(pos)) and not c[:, [i for i in range(3) if i != ax]].any()
    assert np.array_equal(r, np.full(m, rad))
    pts = np.random.default_rng(7).uniform(-1.0, 1.0, (10000, 3)) * np.array(half)
    pts[:8] = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * np.array(half)
    assert _inside_some(pts, c, r * (1 + 1e-12)).all()


def test_cover_of_the_test_bar_and_pose():
    c, r = cover_box((0.03, 0.03, 0.10), tol=0.01)
    assert len(c) == 4
    # placed in the link's frame: rotated a quarter turn about x and moved
    pose = [1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.1, 0.2, 0.3]
    cp, rp = cover_box((0.03, 0.03, 0.10), pose=pose, tol=0.01)
    want = np.array([[0.0 + 0.1, -z + 0.2, 0.0 + 0.3] for z in c[:, 2]])
    assert np.array_equal(rp, r) and np.array_equal(cp, want)


@pytest.mark.parametrize("radius,hl,tol,mx", [(0.03, 0.1, 0.01, 16), (0.1, 0.02, 0.01, 16), (0.02, 0.4, 0.001, 5)])
def test_cover_cylinder(radius, hl, tol, mx):
    c, r = cover_cylinder(radius, hl, tol=tol, max_spheres=mx)
    m, pos, rad = A.cover_formula(hl, radius, tol, mx)
    assert len(c) == m and np.array_equal(c[:, 2], np.array(pos)) and not c[:, :2].any()
    assert np.array_equal(r, np.full(m, rad))
    rng = np.random.default_rng(9)
    ang, rr = rng.uniform(0, 2 * math.pi, 10000), radius * np.sqrt(rng.uniform(0, 1, 10000))
    rr[:100] = radius
    z = rng.uniform(-hl, hl, 10000)
    z[:50], z[50:100] = -hl, hl
    pts = np.column_stack([rr * np.cos(ang), rr * np.sin(ang), z])
    assert _inside_some(pts, c, r * (1 + 1e-12)).all()


def test_cover_errors():
    for kw in (dict(half=(0.0, 0.1, 0.1)), dict(half=(0.1, 0.1, float("nan"))), dict(half=(0.1, 0.1, 0.1), tol=0.0),
               dict(half=(0.1, 0.1, 0.1), tol=float("inf")), dict(half=(0.1, 0.1, 0.1), max_spheres=0)):
        with pytest.raises(L.SmpError) as e:
            cover_box(**kw)
        assert e.value.status == L.SMP_ERR_ARG
    with pytest.raises(L.SmpError):
        cover_cylinder(-0.1, 0.1)
    with pytest.raises(L.SmpError):
        cover_cylinder(0.1, 0.0)


# ------------------------------------------------------------------------------------------ the stand-alone unit
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attach") / "attach_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "attach_table.cpp"), os.path.join(CSRC, "smp_attach.cpp"),
           os.path.join(CSRC, "smp_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _attach_line(link, name, centres, radii, touch=()):
    vals = [float(x).hex() for c in centres for x in c] + [float(x).hex() for x in radii]
    return " ".join(["A", link, name, str(len(radii)), str(len(touch))] + list(touch) + vals) + "\n"


def test_standalone_unit_under_sanitizers(table, base, tmp_path):
    """The same cases through the HIP-free unit under ASAN / UBSAN: device models equal to the JSON path's, the error
    and capacity statuses, the covers, and seeded malformed requests (none may crash, each gets a defined status)."""
    text, want = "", []
    for n in (2, 10, 16):
        c, r = A.bar(n)
        text += "R\n" + _attach_line(HAND, "attached_object", c, r) + "D\n"
        want.append(_json_robot(A.augmented(base, HAND, c, r), tmp_path, "t%d" % n))
    c1, r1 = A.bar(2)
    c2, r2 = [(0.0, 0.0, 0.30), (0.05, 0.0, 0.30)], [0.04, 0.05]
    text += "R\n" + _attach_line(HAND, "attached_object", c1, r1) + _attach_line("base_link", "tray", c2, r2) + "D\n"
    want.append(_json_robot(A.augmented(A.augmented(base, HAND, c1, r1), "base_link", c2, r2, name="tray"), tmp_path, "t2"))
    text += "R\n" + _attach_line(HAND, "x", *A.bar(17)) + _attach_line(HAND, "x", [(0, 0, 0.1)], [0.46])
    text += _attach_line("no_such_link", "x", [(0, 0, 0.1)], [0.05]) + _attach_line(HAND, HAND, [(0, 0, 0.1)], [0.05])
    text += _attach_line(HAND, "x", [(0, 0, 0.1)], [0.05], touch=("nope",)) + _attach_line("-", "x", [(0, 0, 0.1)], [0.05])
    text += "A %s x 0 0\n" % HAND + "A %s x -3 0\n" % HAND
    text += "R\nF 11 300\n" + _attach_line(HAND, "attached_object", *A.bar(10)) + "F 12 300\n"
    text += "B %s %s %s %s 16\n" % tuple(float(x).hex() for x in (0.03, 0.03, 0.10, 0.01))
    text += "C %s %s %s 5\n" % tuple(float(x).hex() for x in (0.02, 0.4, 0.001))
    p = subprocess.run([table, A.MODEL_JSON], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    devs = [bytes.fromhex(l.split()[1]) for l in lines if l.startswith("dev ")]
    links = [l.split()[1:] for l in lines if l.startswith("links")]
    assert len(devs) == 4
    for d, l, w in zip(devs, links, want):
        assert d == w.device_bytes() and l == w.link_names
    st = [int(l.split()[1]) for l in lines if l.startswith("status")]
    assert st[:5] == [0] * 5
    assert st[5:13] == [L.SMP_ERR_CAPACITY] + [L.SMP_ERR_ARG] * 7
    fz = [[int(x) for x in l.split()[1:]] for l in lines if l.startswith("fuzz")]
    assert len(fz) == 2 and all(sum(f) == 300 and f[1] > 50 for f in fz)
    assert fz[0][0] > 0 and all(f[2] > 0 for f in fz)  # some fit, some exceed a capacity
    i = lines.index("cover 0 4")
    got = np.array([[float.fromhex(x) for x in l.split()] for l in lines[i + 1:i + 5]])
    c, r = cover_box((0.03, 0.03, 0.10), tol=0.01)
    assert np.array_equal(got[:, :3], c) and np.array_equal(got[:, 3], r)
    j = lines.index("cover 0 5")
    got = np.array([[float.fromhex(x) for x in l.split()] for l in lines[j + 1:j + 6]])
    c, r = cover_cylinder(0.02, 0.4, tol=0.001, max_spheres=5)
    assert np.array_equal(got[:, :3], c) and np.array_equal(got[:, 3], r)
