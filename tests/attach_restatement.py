"""An independent restatement of smp_robot_attach for the tests: the committed model's dict with one more link, built
in plain Python with the model generator's to_body arithmetic (tools/gen_robot_model.py:346-364, restated here, not
imported).  The dict feeds the CPU oracle (OracleRobot) directly and, written to a temporary JSON file, the library's
own JSON path (Robot(model_json=...)), which smp_robot_attach must equal byte for byte.

The restatement first has to reproduce what it claims to restate: committed_cb_reproduced() recomputes every committed
sphere's `cb` from its `c` and compares the bits."""
import copy
import json
import math
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_JSON = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")

IDENT_R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def base_model():
    with open(MODEL_JSON) as f:
        return json.load(f)


def bits(x):
    return struct.pack("<d", x)


def rot_vec(a, v):
    return [a[r * 3 + 0] * v[0] + a[r * 3 + 1] * v[1] + a[r * 3 + 2] * v[2] for r in range(3)]


def rot_mul(a, b):
    return [a[r * 3 + 0] * b[0 * 3 + c] + a[r * 3 + 1] * b[1 * 3 + c] + a[r * 3 + 2] * b[2 * 3 + c]
            for r in range(3) for c in range(3)]


def frame_mul(f1, f2):
    mp = rot_vec(f1[0], f2[1])
    return (rot_mul(f1[0], f2[0]), [mp[i] + f1[1][i] for i in range(3)])


def body_of(tree, i):
    while tree[i]["joint"] < 0:
        i = tree[i]["parent"]
    return i


def to_body(tree, b, i, c):
    """Point c of link i's frame in the frame of body link b: the frames from b (exclusive) down to i multiplied left
    to right, then applied to c; no arithmetic at all when i is b."""
    path = []
    while i != b:
        path.append(i)
        i = tree[i]["parent"]
    if not path:
        return list(c)
    f = None
    for k in reversed(path):
        fk = (tree[k]["R"], tree[k]["p"])
        f = fk if f is None else frame_mul(f, fk)
    m = rot_vec(f[0], c)
    return [m[d] + f[1][d] for d in range(3)]


def committed_cb_reproduced(model=None):
    """Number of committed spheres whose cb this file's to_body reproduces bit for bit, and the sphere count."""
    model = model or base_model()
    tree = model["links"]
    ok = 0
    for s in model["spheres"]:
        cb = to_body(tree, body_of(tree, s["link"]), s["link"], s["c"])
        ok += all(bits(cb[d]) == bits(s["cb"][d]) for d in range(3))
    return ok, len(model["spheres"])


def augmented(model, link, centres, radii, name="attached_object", touch_links=()):
    """A deep copy of `model` with the object attached (the issue's rules, one by one)."""
    m = copy.deepcopy(model)
    tree = m["links"]
    names = [e["name"] for e in tree]
    parent = names.index(link)
    assert name not in names
    new = len(tree)
    tree.append({"name": name, "parent": parent, "joint": -1, "type": "None", "axis": [0.0, 0.0, 0.0],
                 "origin": [0.0, 0.0, 0.0], "R": list(IDENT_R), "p": [0.0, 0.0, 0.0], "collision": True})
    b = body_of(tree, new)
    body = m["bodies"].index(b)
    for c, r in zip(centres, radii):
        c = [float(x) for x in c]
        m["spheres"].append({"link": new, "c": c, "r": float(r), "body": body, "cb": to_body(tree, b, new, c)})
    ss = [s for s in m["spheres"] if s["link"] == new]
    c = [0.0, 0.0, 0.0]
    for q in ss:
        c = [c[d] + q["c"][d] for d in range(3)]
    c = [c[d] / len(ss) for d in range(3)]
    r = 0.0
    for q in ss:
        dx, dy, dz = q["c"][0] - c[0], q["c"][1] - c[1], q["c"][2] - c[2]
        r = max(r, math.sqrt(dx * dx + dy * dy + dz * dz) + q["r"])
    r = r + 1e-6
    lb_body = {e["link"]: e["body"] for e in m["link_bounds"]}
    touch = {names.index(t) for t in touch_links}
    pairs = [list(p) for p in m["self_pairs"]]
    for e in m["link_bounds"]:
        if lb_body[e["link"]] != body and e["link"] not in touch:
            pairs.append([e["link"], new])
    m["self_pairs"] = sorted(pairs)
    m["link_bounds"].append({"link": new, "c": c, "r": r, "body": body, "cb": to_body(tree, b, new, c)})
    return m


def write_json(model, path):
    with open(path, "w") as f:
        json.dump(model, f)
    return path


# ------------------------------------------------------------------------------------------ the test object
HAND = "hand_palm_link"


def bar(n):
    """The test bar (half extents 0.03, 0.03, 0.10, centred at (0, 0, 0.15) of hand_palm_link) as n spheres."""
    centres = [(0.0, 0.0, 0.05 + 0.20 * (k + 0.5) / n) for k in range(n)]
    radii = [math.sqrt((0.1 / n) ** 2 + 0.03 ** 2 + 0.03 ** 2)] * n
    return centres, radii


# ------------------------------------------------------------------------------------------ the self filter
def world_items(rb, orc, q):
    """Sphere centres (S, 3) and primitive centres / x axes (P, 5) of OracleRobot rb at q from the oracle's body frames,
    as the checker forms them (the three-term sum, then the translation)."""
    import numpy as np
    B = orc.body_fk(np.asarray(q, np.float64).reshape(1, 8))[0]  # (n_body, 12)
    cb = rb.sph_cb.reshape(-1, 3)
    Bs = B[rb.sph_body]
    wc = np.stack([(Bs[:, 3 * r] * cb[:, 0] + Bs[:, 3 * r + 1] * cb[:, 1] + Bs[:, 3 * r + 2] * cb[:, 2]) + Bs[:, 9 + r]
                   for r in range(3)], axis=1)
    P = rb.n_prim
    pw = np.zeros((P, 5))
    if P:
        Bp, pc, ab = B[rb.prim_body[:P]], rb.prim_cb.reshape(-1, 3)[:P], rb.prim_ab.reshape(-1, 3)[:P]
        for r in range(3):
            pw[:, r] = (Bp[:, 3 * r] * pc[:, 0] + Bp[:, 3 * r + 1] * pc[:, 1] + Bp[:, 3 * r + 2] * pc[:, 2]) + Bp[:, 9 + r]
        pw[:, 3] = Bp[:, 0] * ab[:, 0] + Bp[:, 1] * ab[:, 1] + Bp[:, 2] * ab[:, 2]
        pw[:, 4] = Bp[:, 3] * ab[:, 0] + Bp[:, 4] * ab[:, 1] + Bp[:, 5] * ab[:, 2]
    return wc, pw


def carve_geometry(keys_all, res, z_offset=-0.02):
    """(kmin, dims, origin) of the grid smp_planner_set_scene_keys builds for the key list (after floor insertion)."""
    import numpy as np
    from oracle import oracle as O
    keys_all = np.asarray(keys_all, np.int64).reshape(-1, 3)
    pad = O.grid_pad_cells(res)
    kmin, kmax = keys_all.min(0) - pad, keys_all.max(0) + pad
    o = [float(kmin[0] - O.KEY_OFFSET) * res, float(kmin[1] - O.KEY_OFFSET) * res,
         float(kmin[2] - O.KEY_OFFSET) * res + z_offset]
    return kmin, tuple(int(v) for v in kmax - kmin + 1), o


def carve_mask(rb, orc, keys, keys_all, res, q, pad, links=None, z_offset=-0.02):
    """smp_carve_keys restated (include/smp_gpu.h "Self filter"): per key of `keys`, (carved by a sphere, carved by a
    primitive) as two bool arrays; the key is carved iff either holds.  keys_all: the list that fixes the grid geometry
    (keys plus the floor keys).  The single-cell terms are clearance_restatement's: _gapv for the spheres, prim_term
    over a grid that holds that one cell for the primitives (asked only for cells near enough to matter: a cell whose
    centre is farther from the primitive's centre than its bounding ball, the cell's half diagonal and pad together
    cannot be within pad of it)."""
    import types

    import numpy as np

    import clearance_restatement as C
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    kmin, dims, o = carve_geometry(keys_all, res, z_offset)
    sel = [True] * rb.n_links if not links else [n in set(links) for n in rb.link_names]
    wc, pw = world_items(rb, orc, q)
    ijk = (keys - kmin).astype(np.float64)
    lo = [o[d] + ijk[:, d] * res for d in range(3)]
    hi = [o[d] + (ijk[:, d] + 1.0) * res for d in range(3)]
    by_sphere = np.zeros(len(keys), bool)
    for s in range(rb.n_sph):
        if not sel[rb.sph_link[s]]:
            continue
        gx, gy, gz = (C._gapv(wc[s][d], lo[d], hi[d]) for d in range(3))
        by_sphere |= (np.sqrt(gx * gx + gy * gy + gz * gz) - rb.sph_r[s]) <= pad
    by_prim = np.zeros(len(keys), bool)
    grid = types.SimpleNamespace(ox=o[0], oy=o[1], oz=o[2], res=res, nx=dims[0], ny=dims[1], nz=dims[2],
                                 occ=np.zeros((dims[2], dims[1], dims[0]), bool))
    ctr = np.stack([0.5 * (lo[d] + hi[d]) for d in range(3)], axis=1)
    for p in range(rb.n_prim):
        if not sel[rb.prim_link[p]]:
            continue
        ty, h = int(rb.prim_type[p]), rb.prim_h.reshape(-1, 3)[p]
        hz = h[2] if ty == 1 else h[1]
        ball = math.sqrt(rb.prim_rxy[p] ** 2 + hz * hz) + 0.5 * math.sqrt(3.0) * res + pad + 1e-6
        for i in np.flatnonzero(np.linalg.norm(ctr - pw[p, :3], axis=1) <= ball):
            x, y, z = (int(v) for v in keys[i] - kmin)
            grid.occ[z, y, x] = True
            by_prim[i] |= C.prim_term(grid, ty, h, pw[p], pad + 1.0) <= pad
            grid.occ[z, y, x] = False
    return by_sphere, by_prim


def cover_formula(ha, rho, tol, max_spheres):
    """Count, axis positions and radius of smp_cover_box / smp_cover_cylinder (include/smp_gpu.h), restated."""
    t = rho + tol
    reach = math.sqrt(t * t - rho * rho)
    m = min(max_spheres, max(1, int(math.ceil(ha / reach))))
    step = ha / m
    return m, [-ha + (2 * k + 1) * step for k in range(m)], math.sqrt(step * step + rho * rho)
