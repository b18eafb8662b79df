"""Host-side mirror of the reference planner interface, over the C ABI.

`BiRRTstarPlanner` keeps the member names, argument meaning and bool/error behaviour of
birrt_star_motion_planning::BiRRTstarPlanner (birrt_star.h:27-110) as the squirrel_8dof_planner node uses it
(squirrel_8dof_planner.cpp:1221-1248): initialize, setOctree, setDisabledLinkMapCollisions,
reset_planner_and_config, setPlanningSceneInfo, init_planner, run_planner, getJointTrajectoryRef,
isConfigValid, isEdgeValid (and shortcutTrajectory, a simplification pass the reference lacks).  Every call lands in
libsmp_gpu.so (HIP kernels on the GPU); nothing here computes planning or collision results on the CPU.
"""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import check, lib

_pd = ctypes.POINTER(ctypes.c_double)


def default_params(**kw):
    p = L.Params()
    lib().smp_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Robot:
    """Robot model (KDL chain + collision model): from the committed model JSON, or (from_urdf) from the robot
    description the node holds -- URDF and SRDF text plus the sphere covers of the mesh links."""

    def __init__(self, model_json=L.MODEL_JSON, _handle=None):
        if _handle is not None:
            self.h = _handle
            return
        with open(model_json, "rb") as f:
            text = f.read()
        h = ctypes.c_void_p()
        check(lib().smp_robot_create_json(text, ctypes.byref(h)), "smp_robot_create_json")
        self.h = h

    @classmethod
    def from_urdf(cls, urdf, srdf, spheres=None):
        """smp_robot_create_urdf: KDLRobotModel + CollisionChecker construction from the description text
        (birrt_star.cpp:36-73, collision_checker.hpp:176-393)."""
        if spheres is None:
            spheres = open(L.SPHERES_JSON).read()
        enc = lambda t: t.encode() if isinstance(t, str) else bytes(t)
        h = ctypes.c_void_p()
        check(lib().smp_robot_create_urdf(enc(urdf), enc(srdf), enc(spheres), ctypes.byref(h)), "smp_robot_create_urdf")
        return cls(_handle=h)

    def device_bytes(self):
        """The device model (RobotDev) as bytes -- for comparing construction paths."""
        n = lib().smp_probe_robot_dev(self.h, None, 0)
        b = ctypes.create_string_buffer(n)
        lib().smp_probe_robot_dev(self.h, b, n)
        return b.raw

    @property
    def link_names(self):
        n = lib().smp_robot_num_links(self.h)
        return [lib().smp_robot_link_name(self.h, i).decode() for i in range(n)]

    def attach(self, link, centres, radii, name="attached_object", touch_links=()):
        """smp_robot_attach: a new Robot with a grasped object as one more collision link `name`, rigidly fixed to
        `link` and covered by spheres (centres (n, 3) in `link`'s frame, radii (n,)); no self pair with touch_links.
        This robot is untouched, and the result can take a further object."""
        c = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3))
        r = np.ascontiguousarray(np.asarray(radii, np.float64).reshape(-1))
        if len(c) != len(r):
            raise ValueError("attach: %d centres but %d radii" % (len(c), len(r)))
        touch = [t.encode() for t in touch_links]
        a = L.Attach()
        a.link, a.name, a.n_spheres = link.encode(), name.encode(), len(r)
        a.centres, a.radii = c.ctypes.data_as(_pd), r.ctypes.data_as(_pd)
        a.touch_links, a.n_touch = (ctypes.c_char_p * max(len(touch), 1))(*touch), len(touch)
        h = ctypes.c_void_p()
        check(lib().smp_robot_attach(self.h, ctypes.byref(a), ctypes.byref(h)), "smp_robot_attach")
        return Robot(_handle=h)

    def self_rounds_info(self):
        """smp_robot_self_rounds' info: n_sph, n_prim, n_spairs, n_ppairs, qualifies, rounds, lanes, max_rounds."""
        info = (ctypes.c_int32 * 8)()
        check(lib().smp_robot_self_rounds(self.h, info, None, None, None, None, None, None), "smp_robot_self_rounds")
        return dict(zip(("n_sph", "n_prim", "n_spairs", "n_ppairs", "qualifies", "rounds", "lanes", "max_rounds"),
                        list(info)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().smp_robot_destroy(self.h)
            self.h = None


def _cover(status, c, r, n, what):
    check(status, what)
    return c[:n.value].copy(), r[:n.value].copy()


def _pose12(pose):
    if pose is None:
        return None, None
    p = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(12))
    return p, p.ctypes.data_as(_pd)


def cover_box(half, pose=None, tol=0.01, max_spheres=16):
    """smp_cover_box: (centres (m, 3), radii (m,)) of a conservative sphere cover of a box with half extents `half`,
    on its longest axis; pose = 12 values (R row-major, then p) placing the box in the link's frame, None: identity."""
    h = np.ascontiguousarray(np.asarray(half, np.float64).reshape(3))
    keep, pp = _pose12(pose)
    c, r, n = np.zeros((max(max_spheres, 1), 3)), np.zeros(max(max_spheres, 1)), ctypes.c_int()
    return _cover(lib().smp_cover_box(h.ctypes.data_as(_pd), pp, float(tol), int(max_spheres), c.ctypes.data_as(_pd),
                                      r.ctypes.data_as(_pd), ctypes.byref(n)), c, r, n, "smp_cover_box")


def cover_cylinder(radius, half_length, pose=None, tol=0.01, max_spheres=16):
    """smp_cover_cylinder: the same for a cylinder along its own z axis."""
    keep, pp = _pose12(pose)
    c, r, n = np.zeros((max(max_spheres, 1), 3)), np.zeros(max(max_spheres, 1)), ctypes.c_int()
    return _cover(lib().smp_cover_cylinder(float(radius), float(half_length), pp, float(tol), int(max_spheres),
                                           c.ctypes.data_as(_pd), r.ctypes.data_as(_pd), ctypes.byref(n)),
                  c, r, n, "smp_cover_cylinder")


class Scene:
    """Occupancy scene: octomap leaf keys (or a .bt stream) -> padded bitset + squared-EDT prefilter."""

    def __init__(self, h):
        self.h = h

    @classmethod
    def from_keys(cls, keys, res, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        keys = np.ascontiguousarray(np.asarray(keys).reshape(-1, 3), np.uint16)
        o = L.SceneOpts()
        lib().smp_scene_opts_default(ctypes.byref(o))
        o.resolution = res
        o.z_offset = z_offset
        if floor_center is not None:
            o.insert_floor = 1
            o.floor_center[0], o.floor_center[1] = floor_center
            o.floor_distance = floor_distance
        h = ctypes.c_void_p()
        check(lib().smp_scene_from_keys(keys.ctypes.data_as(ctypes.c_void_p), len(keys), ctypes.byref(o),
                                        ctypes.byref(h)), "smp_scene_from_keys")
        return cls(h)

    @staticmethod
    def _opts(z_offset, floor_center, floor_distance):
        o = L.SceneOpts()
        lib().smp_scene_opts_default(ctypes.byref(o))
        o.z_offset = z_offset
        if floor_center is not None:
            o.insert_floor = 1
            o.floor_center[0], o.floor_center[1] = floor_center
            o.floor_distance = floor_distance
        return o

    @classmethod
    def from_bt(cls, data, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """Octomap binary file (.bt) bytes."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        o = cls._opts(z_offset, floor_center, floor_distance)
        h = ctypes.c_void_p()
        check(lib().smp_scene_from_bt(buf, len(data), ctypes.byref(o), ctypes.byref(h)), "smp_scene_from_bt")
        return cls(h)

    @classmethod
    def from_ot(cls, data, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """Octomap full-format file (.ot) bytes (the octomap_server's map, launch/simulation.launch:51)."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        o = cls._opts(z_offset, floor_center, floor_distance)
        h = ctypes.c_void_p()
        check(lib().smp_scene_from_ot(buf, len(data), ctypes.byref(o), ctypes.byref(h)), "smp_scene_from_ot")
        return cls(h)

    @classmethod
    def from_octomap_msg(cls, id, resolution, binary, data, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """octomap_msgs/Octomap fields (squirrel_8dof_planner.cpp:875-883): binaryMsgToMap / fullMsgToMap."""
        data = bytes(data)
        buf = ctypes.create_string_buffer(data, max(len(data), 1))
        o = cls._opts(z_offset, floor_center, floor_distance)
        h = ctypes.c_void_p()
        check(lib().smp_scene_from_octomap_msg(id.encode() if isinstance(id, str) else id, float(resolution),
                                               int(bool(binary)), buf, len(data), ctypes.byref(o), ctypes.byref(h)),
              "smp_scene_from_octomap_msg")
        return cls(h)

    @classmethod
    def from_grid(cls, bits, d2, dims, origin, res):
        bits = np.ascontiguousarray(bits, np.uint64)
        d2 = np.ascontiguousarray(d2, np.uint16)
        dd = (ctypes.c_int * 3)(*dims)
        oo = (ctypes.c_double * 3)(*origin)
        h = ctypes.c_void_p()
        check(lib().smp_scene_from_grid(bits.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p), dd,
                                        oo, res, ctypes.byref(h)), "smp_scene_from_grid")
        return cls(h)

    def info(self):
        dims = (ctypes.c_int * 3)()
        org = (ctypes.c_double * 3)()
        res = ctypes.c_double()
        nocc = ctypes.c_int64()
        bmin = (ctypes.c_double * 3)()
        bmax = (ctypes.c_double * 3)()
        check(lib().smp_scene_info(self.h, dims, org, ctypes.byref(res), ctypes.byref(nocc), bmin, bmax))
        return dict(dims=tuple(dims), origin=tuple(org), res=res.value, n_occupied=nocc.value,
                    bbox_min=tuple(bmin), bbox_max=tuple(bmax))

    def export(self):
        i = self.info()
        nx, ny, nz = i["dims"]
        wx = (nx + 63) // 64
        bits = np.zeros(wx * ny * nz, np.uint64)
        d2 = np.zeros(nx * ny * nz, np.uint16)
        check(lib().smp_scene_export(self.h, bits.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p)))
        return bits, d2

    def __del__(self):
        if getattr(self, "h", None):
            lib().smp_scene_destroy(self.h)
            self.h = None


class GpuPlanner:
    """Thin owner of an smp_planner (one GPU, one robot, one scene at a time)."""

    def __init__(self, robot=None, device=0, **params):
        self.robot = robot or Robot()
        self.params = default_params(**params)
        h = ctypes.c_void_p()
        check(lib().smp_planner_create(device, self.robot.h, ctypes.byref(self.params), ctypes.byref(h)),
              "smp_planner_create")
        self.h = h
        self.scene = None

    def set_robot(self, robot):
        """smp_planner_set_robot: swaps the planner's robot in place (Robot.attach after a grasp, the base robot after
        the release); scene, disabled links, trees and query buffers stay."""
        check(lib().smp_planner_set_robot(self.h, robot.h), "smp_planner_set_robot")
        self.robot = robot

    @staticmethod
    def _carve(q, pad, links):
        c = L.Carve()
        for j in range(8):
            c.q[j] = float(q[j])
        c.pad = float(pad)
        names = [n.encode() for n in (links or ())]
        keep = (ctypes.c_char_p * max(len(names), 1))(*names)
        c.links, c.n_links = keep, len(names)
        return c, keep

    def set_carve(self, q=None, pad=0.0, links=None):
        """smp_planner_set_carve: the sticky self filter of set_scene_keys / _bt / _ot / _octomap_msg -- the robot's
        volume at pose q (the pose the map was taken at), grown by pad metres, is carved out of the occupied keys inside
        the device scene build.  links: the collision links to carve (None: all, attached objects included).
        q=None turns it off.  set_scene and set_scene_device do not carve."""
        if q is None:
            check(lib().smp_planner_set_carve(self.h, None), "smp_planner_set_carve")
            return
        c, keep = self._carve(q, pad, links)
        check(lib().smp_planner_set_carve(self.h, ctypes.byref(c)), "smp_planner_set_carve")

    def carve_keys(self, keys, res, q, pad=0.0, links=None, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """smp_carve_keys: one flag per key (1: carved by the self filter at q and pad), uint8 (n,).  The floor keys of
        floor_center take part in the grid geometry only."""
        keys = np.ascontiguousarray(np.asarray(keys).reshape(-1, 3), np.uint16)
        o = Scene._opts(z_offset, floor_center, floor_distance)
        o.resolution = res
        c, keep = self._carve(q, pad, links)
        out = np.zeros(len(keys), np.uint8)
        check(lib().smp_carve_keys(self.h, keys.ctypes.data_as(ctypes.c_void_p), len(keys), ctypes.byref(o),
                                   ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), None), "smp_carve_keys")
        return out

    def last_carve(self):
        """smp_planner_last_carve: n_carved, kernel_ms, total_ms of the last carving build or carve_keys call."""
        info = L.CarveInfo()
        check(lib().smp_planner_last_carve(self.h, ctypes.byref(info)), "smp_planner_last_carve")
        return {f: getattr(info, f) for f, _ in L.CarveInfo._fields_}

    def set_scene(self, scene):
        check(lib().smp_planner_set_scene(self.h, scene.h), "smp_planner_set_scene")
        self.scene = scene

    # The scene built on the GPU (smp_planner_set_scene_*): the same device arrays as Scene.from_* + set_scene, derived
    # by kernels from the occupied keys.  Each returns the smp_scene_build fields as a dict.
    def _built(self, status, info, what):
        check(status, what)
        self.scene = None
        d = {f: getattr(info, f) for f, _ in L.SceneBuild._fields_}
        for f in ("dims", "origin", "bbox_min", "bbox_max"):
            d[f] = tuple(d[f])
        return d

    def set_scene_keys(self, keys, res, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        keys = np.ascontiguousarray(np.asarray(keys).reshape(-1, 3), np.uint16)
        o = Scene._opts(z_offset, floor_center, floor_distance)
        o.resolution = res
        info = L.SceneBuild()
        return self._built(lib().smp_planner_set_scene_keys(self.h, keys.ctypes.data_as(ctypes.c_void_p), len(keys),
                                                            ctypes.byref(o), ctypes.byref(info)),
                           info, "smp_planner_set_scene_keys")

    def set_scene_bt(self, data, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """Octomap binary file (.bt) bytes."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        o = Scene._opts(z_offset, floor_center, floor_distance)
        info = L.SceneBuild()
        return self._built(lib().smp_planner_set_scene_bt(self.h, buf, len(data), ctypes.byref(o), ctypes.byref(info)),
                           info, "smp_planner_set_scene_bt")

    def set_scene_ot(self, data, z_offset=-0.02, floor_center=None, floor_distance=3.0):
        """Octomap full-format file (.ot) bytes."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        o = Scene._opts(z_offset, floor_center, floor_distance)
        info = L.SceneBuild()
        return self._built(lib().smp_planner_set_scene_ot(self.h, buf, len(data), ctypes.byref(o), ctypes.byref(info)),
                           info, "smp_planner_set_scene_ot")

    def set_scene_octomap_msg(self, id, resolution, binary, data, z_offset=-0.02, floor_center=None,
                              floor_distance=3.0):
        """octomap_msgs/Octomap fields (squirrel_8dof_planner.cpp:875-883)."""
        data = bytes(data)
        buf = ctypes.create_string_buffer(data, max(len(data), 1))
        o = Scene._opts(z_offset, floor_center, floor_distance)
        info = L.SceneBuild()
        return self._built(lib().smp_planner_set_scene_octomap_msg(
            self.h, id.encode() if isinstance(id, str) else id, float(resolution), int(bool(binary)), buf, len(data),
            ctypes.byref(o), ctypes.byref(info)), info, "smp_planner_set_scene_octomap_msg")

    def scene_arrays(self):
        """The planner's device-resident scene copied to the host: (layout, bricks, d2, d2b or None, slab) as numpy
        arrays (smp_planner_scene_device with host buffers as destinations)."""
        v = self.scene_device()
        bricks = np.zeros(v.n_bricks, np.uint64)
        d2 = np.zeros(v.n_cells, np.uint16)
        d2b = np.zeros(v.n_cells, np.uint8) if v.has_d2b else None
        slab = np.zeros(v.n_prim * v.dims[0] * v.dims[1], np.uint16)
        v = self.scene_device(bricks.ctypes.data, d2.ctypes.data, d2b.ctypes.data if v.has_d2b else 0,
                              slab.ctypes.data if slab.size else 0)
        return v, bricks, d2, d2b, slab

    def scene_device(self, bricks=0, d2=0, d2b=0, slab=0):
        """smp_planner_scene_device: geometry and sizes of the planner's device-resident scene; each non-zero device
        address (e.g. a torch tensor's data_ptr() on any GPU) receives a device-to-device copy of that array."""
        v = L.SceneDevice()
        v.bricks, v.d2, v.d2b, v.slab = bricks or None, d2 or None, d2b or None, slab or None
        check(lib().smp_planner_scene_device(self.h, ctypes.byref(v)), "smp_planner_scene_device")
        return v

    def set_scene_device(self, layout, bricks, d2, d2b=0, slab=0):
        """smp_planner_set_scene_device: the scene from device arrays laid out as `layout` (scene_device() of the
        sending planner), given by device address; copied, so the caller may release them afterwards."""
        v = L.SceneDevice()
        ctypes.pointer(v)[0] = layout
        v.bricks, v.d2, v.d2b, v.slab = bricks or None, d2 or None, d2b or None, slab or None
        check(lib().smp_planner_set_scene_device(self.h, ctypes.byref(v)), "smp_planner_set_scene_device")
        self.scene = None

    def set_disabled_map_links(self, names):
        arr = (ctypes.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        check(lib().smp_set_disabled_map_links(self.h, arr, len(names)))

    def check_configs(self, q, check_self=True, check_map=True):
        q = np.asarray(q, np.float64).reshape(-1, 8)
        soa = np.ascontiguousarray(q.T)
        out = np.zeros(len(q), np.uint8)
        check(lib().smp_check_configs(self.h, soa.ctypes.data_as(_pd), len(q), int(check_self), int(check_map),
                                      out.ctypes.data_as(ctypes.c_void_p)), "smp_check_configs")
        return out

    def check_sequence(self, poses, check_self=True, check_map=True):
        """Index of the first pose in collision (-1: all valid), one batched check (fold / unfold keyframes)."""
        q = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 8))
        first = ctypes.c_int64()
        check(lib().smp_check_sequence(self.h, q.ctypes.data_as(_pd), len(q), int(check_self), int(check_map),
                                       ctypes.byref(first)), "smp_check_sequence")
        return first.value

    def check_clear(self, q, check_self=True, check_map=True, margin=None):
        """smp_check_configs_margin: 1 per configuration that is valid and farther than margin = (map, self) metres
        from the map and from self-collision (include/smp_gpu.h "Margin checks"), else 0.  margin=None is (0, 0): the
        validity check."""
        q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, 8))
        out = np.zeros(len(q), np.uint8)
        check(lib().smp_check_configs_margin(self.h, q.ctypes.data_as(_pd), len(q), int(check_self), int(check_map),
                                             _margin(margin), out.ctypes.data_as(ctypes.c_void_p)),
              "smp_check_configs_margin")
        return out

    def check_edges(self, frm, to, check_self=True, check_map=True, margin=None):
        """Batched isEdgeValid (birrt_star.cpp:6864-6895) at the density rule of smp_check_edges: (first_invalid,
        n_points) per edge frm[i] -> to[i]; first_invalid is the index of the first colliding point, -1 if free.
        margin = (map, self): smp_check_edges_margin, the first point that is not clear at those margins."""
        a, b = _edge_rows("check_edges", frm, to)
        first = np.zeros(len(a), np.int64)
        npts = np.zeros(len(a), np.int32)
        args = (first.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), npts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        head = (self.h, a.ctypes.data_as(_pd), b.ctypes.data_as(_pd), len(a), int(check_self), int(check_map))
        if margin is None:
            check(lib().smp_check_edges(*head, *args), "smp_check_edges")
        else:
            check(lib().smp_check_edges_margin(*head, _margin(margin), *args), "smp_check_edges_margin")
        return first, npts

    def shortcut_path(self, path, check_self=True, check_map=True, window=0, margin=None):
        """smp_shortcut_path: every waypoint pair within `window` (0: all pairs) checked as a dense edge in one launch,
        the cheapest route through the valid ones, via nodes inserted.  Returns (path (m, 8), info dict); a blocked
        path raises SmpError with status SMP_ERR_NO_SOLUTION, its `info` attribute holding the dict.
        margin = (map, self): smp_shortcut_path_margin, the route through the pairs that are clear at those margins."""
        w = np.ascontiguousarray(np.asarray(path, np.float64).reshape(-1, 8))
        out = _pd()
        n_out = ctypes.c_int64()
        info = L.ShortcutInfo()
        head = (self.h, w.ctypes.data_as(_pd), len(w), int(check_self), int(check_map), int(window))
        tail = (ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(info))
        if margin is None:
            return _returned_path("smp_shortcut_path", lib().smp_shortcut_path(*head, *tail), out, n_out, info)
        rc = lib().smp_shortcut_path_margin(*head, _margin(margin), *tail)
        return _returned_path("smp_shortcut_path_margin", rc, out, n_out, info)

    def sample_detours(self, frm, to, samples, half_width, seed=1, round=0, check_self=True, check_map=True,
                       margin=None):
        """smp_sample_detours: for every gap frm[g] -> to[g], `samples` one-via detours drawn around the gap's centre
        within `half_width` and both legs of each checked densely, one launch.  Returns a dict of v (G, S, 8), M1, M2
        and free (G, S).  margin = (map, self): smp_sample_detours_margin, free = both legs clear at those margins."""
        a, b = _edge_rows("sample_detours", frm, to)
        n = len(a) * max(int(samples), 0)
        out = (L.Detour * max(n, 1))()
        head = (self.h, a.ctypes.data_as(_pd), b.ctypes.data_as(_pd), len(a), int(samples), float(half_width), int(seed),
                int(round), int(check_self), int(check_map))
        if margin is None:
            check(lib().smp_sample_detours(*head, out), "smp_sample_detours")
        else:
            check(lib().smp_sample_detours_margin(*head, _margin(margin), out), "smp_sample_detours_margin")
        rec = np.frombuffer(out, dtype=np.dtype([("v", np.float64, 8), ("M1", np.int32), ("M2", np.int32),
                                                 ("free", np.int32), ("pad", np.int32)]), count=n)
        shape = (len(a), int(samples))
        return dict(v=rec["v"].reshape(shape + (8,)).copy(), M1=rec["M1"].reshape(shape).copy(),
                    M2=rec["M2"].reshape(shape).copy(), free=rec["free"].reshape(shape).copy())

    def repair_path(self, path, check_self=True, check_map=True, samples=256, rounds=4, seed=1, margin=None):
        """smp_repair_path: the blocked stretches of `path` gathered into gaps between valid waypoints and each bridged
        by the cheapest free one-via detour, the half width doubling per round.  Returns (path (m, 8), info dict) with
        the via nodes of every edge inserted; gaps that stay open raise SmpError with status SMP_ERR_NO_SOLUTION, its
        `info` attribute holding the dict (as every other failure does).  margin = (map, self):
        smp_repair_path_margin, "valid / free" read as "clear at those margins"."""
        w = np.ascontiguousarray(np.asarray(path, np.float64).reshape(-1, 8))
        out = _pd()
        n_out = ctypes.c_int64()
        info = L.RepairInfo()
        opts = L.RepairOpts(int(samples), int(rounds), int(seed))
        head = (self.h, w.ctypes.data_as(_pd), len(w), int(check_self), int(check_map), ctypes.byref(opts))
        tail = (ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(info))
        if margin is None:
            return _returned_path("smp_repair_path", lib().smp_repair_path(*head, *tail), out, n_out, info)
        rc = lib().smp_repair_path_margin(*head, _margin(margin), *tail)
        return _returned_path("smp_repair_path_margin", rc, out, n_out, info)

    def base_free_map(self, lattice, margin=None):
        """smp_base_free_map: the base's free space on `lattice` (base_lattice_fit's, or a dict of smp_base_lattice's
        fields) with the arm held at lattice.arm, every node answered by the map check in one launch.  Returns
        (free (n_theta, ny, nx) bool, info dict); margin: a map margin in metres (or a (map, self) pair, whose self part
        is ignored), None: the boolean check."""
        lat = _lattice(lattice)
        n = max(lat.nx, 0) * max(lat.ny, 0) * max(lat.n_theta, 0)
        bits = np.zeros(max((n + 31) // 32, 1) if n <= L.SMP_LATTICE_MAX_NODES else 1, np.uint32)
        info = L.BaseMapInfo()
        m = None if margin is None else _margin(margin if np.ndim(margin) else (margin, 0.0))
        check(lib().smp_base_free_map(self.h, ctypes.byref(lat), m, bits.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.byref(info)), "smp_base_free_map")
        free = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
        self.base_map_bits = bits  # the words as the call left them (the unused bits of the last one are 0)
        return free.reshape(lat.n_theta, lat.ny, lat.nx), {f: getattr(info, f) for f, _ in L.BaseMapInfo._fields_}

    @staticmethod
    def base_route(lattice, free, frm, to, snap_cells=2):
        """smp_base_route over a free map of base_free_map: the module's base_route (host only)."""
        return base_route(lattice, free, frm, to, snap_cells)

    def base_cost_field(self, lattice, free, source, want_parent=True):
        """smp_base_cost_field: the cheapest cost from node source = (ix, iy, t) to every node of `lattice` over the
        free map `free` (base_free_map's array), computed on the device.  Returns (cost (n_theta, ny, nx) float64, +inf
        where blocked or unreachable; parent (n_theta, ny, nx) int32 node numbers, -1 for the source and +inf nodes, or
        None with want_parent=False; info dict of smp_field_info)."""
        lat = _lattice(lattice)
        bits = _packed_free("base_cost_field", lat, free)
        n = lat.nx * lat.ny * lat.n_theta
        cost = np.empty(n, np.float64)
        parent = np.empty(n, np.int32) if want_parent else None
        info = L.FieldInfo()
        src = (ctypes.c_int32 * 3)(*[int(v) for v in source])
        check(lib().smp_base_cost_field(self.h, ctypes.byref(lat), bits.ctypes.data_as(ctypes.c_void_p), src,
                                        cost.ctypes.data_as(_pd),
                                        parent.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_parent else None,
                                        ctypes.byref(info)), "smp_base_cost_field")
        shape = (lat.n_theta, lat.ny, lat.nx)
        return cost.reshape(shape), parent.reshape(shape) if want_parent else None, _fields(info)

    def base_route_gpu(self, lattice, free, frm, to, snap_cells=2):
        """smp_base_route_gpu: base_route with the search on the device.  Returns (rows, chain, info dict, field info
        dict); a failure raises SmpError with the two dicts as its `info` and `field` attributes."""
        lat = _lattice(lattice)
        bits = _packed_free("base_route_gpu", lat, free)
        finfo = L.FieldInfo()
        try:
            call = lambda *a: lib().smp_base_route_gpu(self.h, *a, ctypes.byref(finfo))
            r, c, d = _route_call("smp_base_route_gpu", call, lat, bits, frm, to, snap_cells)
        except L.SmpError as err:
            err.field = _fields(finfo)
            raise
        return r, c, d, _fields(finfo)

    def plan_far(self, query, **opts):
        """smp_plan_far: the staged plan for a goal across the room -- the free map of the folded-arm base lattice over
        the query's environment, the route over it, the route checked densely and shortened, then plan() for the last
        handover_distance metres.  opts: smp_far_opts' fields (pitch, n_theta, arm, handover_distance, map_margin,
        window, snap_cells, route_device -- 1: the route search on the device, the same answer).  Returns plan()'s
        dict, its `path` led by the `far`["n_route_rows"] rows of the base stage; `far` holds smp_far_info (stage, map,
        route, handover_node, n_route_rows, check, route_ms, total_ms).  Per-query outcomes come back in `status`;
        failures of the call itself raise, as plan()'s do."""
        o = L.FarOpts()
        lib().smp_far_opts_default(ctypes.byref(o))
        for k, v in opts.items():
            if k == "arm":
                for j in range(5):
                    o.arm[j] = float(v[j])
            else:
                setattr(o, k, v)
        r, info = L.Result(), L.FarInfo()
        rc = lib().smp_plan_far(self.h, ctypes.byref(query), ctypes.byref(o), ctypes.byref(r), ctypes.byref(info))
        d = _result_dict(r)
        lib().smp_result_free(ctypes.byref(r))
        if rc in _CALL_FAILURES:
            raise L.SmpError(rc, "smp_plan_far")
        d["far"] = dict(stage=info.stage, map=_fields(info.map), route=_route_info(info.route),
                        handover_node=tuple(info.handover_node), n_route_rows=info.n_route_rows,
                        check=_fields(info.check), route_ms=info.route_ms, total_ms=info.total_ms)
        return d

    def clearance(self, q, max_dist=0.3, with_self=True, with_map=True):
        """smp_clearance_configs: distance of every configuration to the map (capped at max_dist) and to self-collision,
        one launch.  Returns a structured array (CLEARANCE_DTYPE: map, self, map_link, self_a, self_b; link indices
        into robot.link_names, -1 for none); `clearance_info` keeps the call's point count and timing."""
        q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, 8))
        out = np.zeros(len(q), CLEARANCE_DTYPE)
        info = L.ClearanceInfo()
        check(lib().smp_clearance_configs(self.h, q.ctypes.data_as(_pd), len(q), float(max_dist), int(with_self),
                                          int(with_map), out.ctypes.data_as(ctypes.POINTER(L.Clearance)),
                                          ctypes.byref(info)), "smp_clearance_configs")
        self.clearance_info = {f: getattr(info, f) for f, _ in L.ClearanceInfo._fields_}
        return out

    def edge_clearance(self, frm, to, max_dist=0.3, with_self=True, with_map=True):
        """smp_clearance_edges: the minima of both clearances over every dense edge frm[i] -> to[i] (the density rule of
        smp_check_edges), the lowest points attaining them and those points' witness links, one launch.  Returns a
        structured array (EDGE_CLEARANCE_DTYPE); `clearance_info` keeps the call's point count and timing."""
        a, b = _edge_rows("edge_clearance", frm, to)
        out = np.zeros(len(a), EDGE_CLEARANCE_DTYPE)
        info = L.ClearanceInfo()
        check(lib().smp_clearance_edges(self.h, a.ctypes.data_as(_pd), b.ctypes.data_as(_pd), len(a), float(max_dist),
                                        int(with_self), int(with_map),
                                        out.ctypes.data_as(ctypes.POINTER(L.EdgeClearance)), ctypes.byref(info)),
              "smp_clearance_edges")
        self.clearance_info = {f: getattr(info, f) for f, _ in L.ClearanceInfo._fields_}
        return out

    def path_clearance(self, waypoints, max_dist=0.3, with_self=True, with_map=True):
        """The adjacent edges of a path through edge_clearance, and a summary: per kind the path's minimum, the first
        edge attaining it, that edge's point and the witness link names (None where there is none).  Returns
        (edges, summary)."""
        w = np.asarray(waypoints, np.float64).reshape(-1, 8)
        if len(w) < 2:
            raise ValueError("path_clearance: a path has at least two waypoints")
        e = self.edge_clearance(w[:-1], w[1:], max_dist, with_self, with_map)
        names = self.robot.link_names
        name = lambda l: names[l] if l >= 0 else None
        im, is_ = int(np.argmin(e["map"])), int(np.argmin(e["self"]))
        has_m, has_s = e["map_point"][im] >= 0, e["self_point"][is_] >= 0
        summary = dict(map=float(e["map"][im]), map_edge=im if has_m else -1, map_point=int(e["map_point"][im]),
                       map_link=name(int(e["map_link"][im])),
                       self=float(e["self"][is_]), self_edge=is_ if has_s else -1,
                       self_point=int(e["self_point"][is_]),
                       self_links=(name(int(e["self_a"][is_])), name(int(e["self_b"][is_]))),
                       n_points=int(e["n_points"].sum()))
        return e, summary

    def get_collisions(self, q):
        """getCollisions (birrt_star.cpp:6910-6914): (self pairs [(link a, link b)] in pair order, map-colliding links
        in name order) of one configuration, as link names; disabled links are listed too, as in the reference."""
        qa = np.ascontiguousarray(np.asarray(q, np.float64).reshape(8))
        names = self.robot.link_names
        cap_s, cap_m = 256, len(names)
        sp = (ctypes.c_int32 * (2 * cap_s))()
        ml = (ctypes.c_int32 * max(cap_m, 1))()
        ns, nm = ctypes.c_int(), ctypes.c_int()
        check(lib().smp_get_collisions(self.h, qa.ctypes.data_as(_pd), sp, cap_s, ctypes.byref(ns), ml, cap_m,
                                       ctypes.byref(nm)), "smp_get_collisions")
        if ns.value > cap_s or nm.value > cap_m:
            raise L.SmpError(L.SMP_ERR_ARG, "smp_get_collisions: more results than capacity")
        return ([(names[sp[2 * k]], names[sp[2 * k + 1]]) for k in range(ns.value)],
                [names[ml[k]] for k in range(nm.value)])

    def ik_solve(self, ee_poses, q_inits, deviation=None, max_iter=1000):
        """getFullPoseFromEEPose's controller (run_VDLS_Control_Connector) for n (end-effector pose, start
        configuration) pairs, one wavefront each.  ee_poses: (n, 6) or one (6,) pose for every start; deviation: (6, 2)
        error bands (default: findGoalPose's).  Returns dict of arrays q (n, 8), reached, iterations, error, manip."""
        q_inits = np.asarray(q_inits, np.float64).reshape(-1, 8)
        ee = np.asarray(ee_poses, np.float64).reshape(-1, 6)
        if len(ee) == 1:
            ee = np.repeat(ee, len(q_inits), 0)
        if len(ee) != len(q_inits):
            raise ValueError("ik_solve: %d end-effector poses for %d start configurations" % (len(ee), len(q_inits)))
        dev = np.asarray(IK_DEVIATION if deviation is None else deviation, np.float64).reshape(6, 2)
        n = len(q_inits)
        reqs = (L.IkRequest * max(n, 1))()
        for i in range(n):
            r = reqs[i]
            for k in range(6):
                r.ee_pose[k] = float(ee[i, k])
                r.deviation[k][0], r.deviation[k][1] = float(dev[k, 0]), float(dev[k, 1])
            for j in range(8):
                r.q_init[j] = float(q_inits[i, j])
            r.max_iter = int(max_iter)
        res = (L.IkResult * max(n, 1))()
        check(lib().smp_ik_solve(self.h, reqs, n, res), "smp_ik_solve")
        return dict(q=np.array([list(r.q) for r in res[:n]]).reshape(n, 8),
                    reached=np.array([r.reached for r in res[:n]], np.int32),
                    iterations=np.array([r.iterations for r in res[:n]], np.int32),
                    fallback=np.array([r.fallback_iterations for r in res[:n]], np.int32),
                    error=np.array([list(r.error) for r in res[:n]]).reshape(n, 6),
                    manip=np.array([r.manipulability for r in res[:n]]))

    def find_goal_pose(self, ee_pose, pose_current, discretization_deg=20.0, check_self=True, check_map=True):
        """Planner::findGoalPose -> (result 0 found / 1 collision / 2 no IK solution, pose_goal or None, info dict)."""
        ee = np.ascontiguousarray(ee_pose, np.float64).reshape(6)
        cur = np.ascontiguousarray(pose_current, np.float64).reshape(8)
        goal = np.zeros(8)
        res = ctypes.c_int()
        info = L.GoalSearch()
        check(lib().smp_find_goal_pose(self.h, ee.ctypes.data_as(_pd), cur.ctypes.data_as(_pd),
                                       float(discretization_deg), int(check_self), int(check_map),
                                       goal.ctypes.data_as(_pd), ctypes.byref(res), ctypes.byref(info)),
              "smp_find_goal_pose")
        d = {f: getattr(info, f) for f, _ in L.GoalSearch._fields_}
        return res.value, (goal if res.value == 0 else None), d

    def last_kernel_ms(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        check(lib().smp_last_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    @staticmethod
    def make_query(start, goal, env_x=(0, 0), env_y=(0, 0), check_self=True, check_map=True, iterations=None,
                   seconds=None, samples=None, seed=1, query_id=0):
        """One query; the budget is `seconds`, else `samples` (collision-checked configurations), else
        `iterations` (default 1000)."""
        q = L.Query()
        for j in range(8):
            q.start[j] = float(start[j])
            q.goal[j] = float(goal[j])
        q.env_x[0], q.env_x[1] = env_x
        q.env_y[0], q.env_y[1] = env_y
        q.check_self, q.check_map = int(check_self), int(check_map)
        if seconds is not None:
            q.budget_kind, q.budget = L.BUDGET_SECONDS, float(seconds)
        elif samples is not None:
            q.budget_kind, q.budget = L.BUDGET_SAMPLES, float(samples)
        else:
            q.budget_kind, q.budget = L.BUDGET_ITERATIONS, float(1000 if iterations is None else iterations)
        q.seed = seed
        q.query_id = query_id
        return q

    def plan_batch(self, queries):
        n = len(queries)
        qa = (L.Query * n)(*queries)
        ra = (L.Result * n)()
        rc = lib().smp_plan_batch(self.h, qa, n, ra)
        out = []
        for r in ra:
            d = _result_dict(r)
            lib().smp_result_free(ctypes.byref(r))
            out.append(d)
        # per-query outcomes (a path, no path, invalid start / goal / budget, a full tree) come back in the results;
        # a failure of the call itself (HIP error, no device, the no-progress guard) raises
        failed = [d["status"] for d in out if d["status"] in _CALL_FAILURES]
        if rc in _CALL_FAILURES or failed:
            raise L.SmpError(rc if rc in _CALL_FAILURES else failed[0], "smp_plan_batch")
        return out

    def plan(self, query):
        return self.plan_batch([query])[0]

    @staticmethod
    def share_scene(planners, src=0):
        """smp_planners_share_scene: planners[src]'s scene to the others (xGMI peer copies across GPUs)."""
        arr = (ctypes.c_void_p * len(planners))(*[p.h.value for p in planners])
        check(lib().smp_planners_share_scene(arr, len(planners), int(src)), "smp_planners_share_scene")
        for k, p in enumerate(planners):
            if k != src:
                p.scene = planners[src].scene

    @staticmethod
    def plan_multi(planners, queries):
        """smp_plan_multi: query i on planners[i % len(planners)], all planners concurrently; results in query
        order (per-query outcomes in the dicts, call failures raise as plan_batch)."""
        n = len(queries)
        arr = (ctypes.c_void_p * len(planners))(*[p.h.value for p in planners])
        qa = (L.Query * n)(*queries)
        ra = (L.Result * n)()
        rc = lib().smp_plan_multi(arr, len(planners), qa, n, ra)
        if rc == L.SMP_ERR_ARG and all(r.status == L.SMP_ERR_ARG for r in ra):
            raise L.SmpError(rc, "smp_plan_multi")
        out = []
        for r in ra:
            d = _result_dict(r)
            lib().smp_result_free(ctypes.byref(r))
            out.append(d)
        failed = [d["status"] for d in out if d["status"] in _CALL_FAILURES]
        if rc in _CALL_FAILURES or failed:
            raise L.SmpError(rc if rc in _CALL_FAILURES else failed[0], "smp_plan_multi")
        return out

    def tree(self, which):
        n = lib().smp_get_tree(self.h, which, None, None, None)
        if n < 0:
            raise L.SmpError(L.SMP_ERR_ARG, "smp_get_tree")
        par = np.zeros(n, np.int32)
        conf = np.zeros((n, 8))
        cost = np.zeros((n, 3))
        lib().smp_get_tree(self.h, which, par.ctypes.data_as(ctypes.c_void_p), conf.ctypes.data_as(ctypes.c_void_p),
                           cost.ctypes.data_as(ctypes.c_void_p))
        return par, conf, cost

    def export_state(self):
        """The state of query 0 of the last plan / plan_batch call (the library keeps that query's buffers and tree
        sizes; after a batch it is the batch's first query, not its last) in the form oracle.Oracle.resume() takes.
        Test infrastructure: the oracle continues the GPU's run from it -- large-tree parity and the CPU timed at the
        GPU's tree sizes -- and tests/tree_audit.py audits it, after single-query calls."""
        iv = np.zeros(16, np.int64)
        dv = np.zeros(25)
        check(lib().smp_probe_export_state(self.h, iv.ctypes.data_as(ctypes.c_void_p), dv.ctypes.data_as(_pd)),
              "smp_probe_export_state")
        st = {"iv": iv[:12].copy(), "dv": dv}
        for which, name in ((0, "start"), (1, "goal")):
            par, conf, cost = self.tree(which)
            n = len(par)
            fc, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
            es, et = np.zeros((n, 8)), np.zeros((n, 8))
            check(lib().smp_probe_export_tree(self.h, which, fc.ctypes.data_as(ctypes.c_void_p),
                                              ns.ctypes.data_as(ctypes.c_void_p), es.ctypes.data_as(_pd),
                                              et.ctypes.data_as(_pd)), "smp_probe_export_tree")
            # the reference's out-edge order: the GPU's child lists (head insertion) reversed
            off = np.zeros(n + 1, np.int32)
            ids = []
            for i in range(n):
                off[i] = len(ids)
                ch = []
                c = int(fc[i])
                while c >= 0:
                    ch.append(c)
                    c = int(ns[c])
                ids.extend(reversed(ch))
            off[n] = len(ids)
            st[name] = {"parent": par, "conf": conf, "cost": cost, "e_start": es, "e_target": et, "child_off": off,
                        "child_ids": np.array(ids, np.int32), "edges": int(iv[12 + which]),
                        "rewires": int(iv[14 + which])}
        return st

    def __del__(self):
        if getattr(self, "h", None):
            lib().smp_planner_destroy(self.h)
            self.h = None


# records of GpuPlanner.clearance / edge_clearance (smp_clearance, smp_edge_clearance)
CLEARANCE_DTYPE = np.dtype([("map", np.float64), ("self", np.float64), ("map_link", np.int32), ("self_a", np.int32),
                            ("self_b", np.int32), ("pad", np.int32)])
EDGE_CLEARANCE_DTYPE = np.dtype([("map", np.float64), ("self", np.float64), ("map_point", np.int32),
                                 ("self_point", np.int32), ("map_link", np.int32), ("self_a", np.int32),
                                 ("self_b", np.int32), ("n_points", np.int32)])

# findGoalPose's endEffectorDeviations (squirrel_8dof_planner.cpp:1131-1137)
IK_DEVIATION = [(-0.005, 0.005)] * 3 + [(-0.025, 0.025)] * 3

_CALL_FAILURES = (L.SMP_ERR_HIP, L.SMP_ERR_NO_DEVICE, L.SMP_ERR_PARSE)


def _fields(s):
    return {f: getattr(s, f) for f, _ in s._fields_}


def _route_info(r):
    return dict(from_node=tuple(r.from_node), to_node=tuple(r.to_node), n_chain=r.n_chain, n_settled=r.n_settled,
                cost=r.cost)


def _lattice(lattice):
    """smp_base_lattice of an L.BaseLattice or of a dict of its fields."""
    if isinstance(lattice, L.BaseLattice):
        return lattice
    lat = L.BaseLattice()
    for k, v in (lattice._asdict() if hasattr(lattice, "_asdict") else dict(lattice)).items():
        if k == "arm":
            for j in range(5):
                lat.arm[j] = float(v[j])
        else:
            setattr(lat, k, v)
    return lat


def base_lattice_fit(env_x, env_y, pitch, n_theta, theta0=0.0, arm=(-0.7, 1.9, 0.0, 1.7, 0.0)):
    """smp_base_lattice_fit: the lattice over the environment env_x x env_y at `pitch` with n_theta headings of a full
    circle from theta0 and the arm held at `arm` (default: pose_folded_arm).  Host only."""
    ex, ey, a = (ctypes.c_double * 2)(*env_x), (ctypes.c_double * 2)(*env_y), (ctypes.c_double * 5)(*arm)
    lat = L.BaseLattice()
    check(lib().smp_base_lattice_fit(ex, ey, float(pitch), int(n_theta), float(theta0), a, ctypes.byref(lat)),
          "smp_base_lattice_fit")
    return lat


def base_route(lattice, free, frm, to, snap_cells=2):
    """smp_base_route: the cheapest route over the free nodes of `lattice` (free: base_free_map's (n_theta, ny, nx)
    array) from the node of frm = (x, y, theta) to the node of to; blocked ends snap to a free node within snap_cells
    rings.  Returns (rows (m, 8) with straight runs merged, chain (n_chain, 3) of (ix, iy, t), info dict).  Host only.
    A failure raises SmpError with the dict as its `info` attribute."""
    lat = _lattice(lattice)
    return _route_call("smp_base_route", lib().smp_base_route, lat, _packed_free("base_route", lat, free), frm, to,
                       snap_cells)


def _packed_free(what, lat, free):
    """The words of a free map (n_theta, ny, nx) of `lat`: bit n % 32 of word n / 32."""
    f = np.asarray(free, bool).reshape(-1)
    if len(f) != lat.nx * lat.ny * lat.n_theta:
        raise ValueError("%s: %d flags for a lattice of %d nodes" % (what, len(f), lat.nx * lat.ny * lat.n_theta))
    packed = np.packbits(np.concatenate([f, np.zeros(-len(f) % 32, bool)]), bitorder="little")
    return np.ascontiguousarray(packed).view(np.uint32) if len(packed) else np.zeros(1, np.uint32)


def _route_call(name, fn, lat, bits, frm, to, snap_cells):
    """One route call (smp_base_route's arguments from the lattice on): (rows, chain, info dict)."""
    a, b = (ctypes.c_double * 3)(*frm), (ctypes.c_double * 3)(*to)
    rows, n_out, chain, info = _pd(), ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)(), L.RouteInfo()
    rc = fn(ctypes.byref(lat), bits.ctypes.data_as(ctypes.c_void_p), a, b, int(snap_cells),
            ctypes.byref(rows), ctypes.byref(n_out), ctypes.byref(chain), ctypes.byref(info))
    d = _route_info(info)
    if rc != L.SMP_OK:
        err = L.SmpError(rc, name)
        err.info = d
        raise err
    try:
        r = np.ctypeslib.as_array(rows, shape=(n_out.value, 8)).copy()
        c = np.ctypeslib.as_array(chain, shape=(info.n_chain, 3)).copy()
    finally:
        lib().smp_buffer_free(rows)
        lib().smp_buffer_free(chain)
    return r, c, d


def _margin(margin):
    """smp_margin* of a (map, self) pair; None is the NULL margin."""
    if margin is None:
        return None
    m, s = margin
    return ctypes.byref(L.Margin(float(m), float(s)))


def _edge_rows(what, frm, to):
    """The contiguous (n, 8) start and end rows of a table of edges or gaps."""
    a = np.ascontiguousarray(np.asarray(frm, np.float64).reshape(-1, 8))
    b = np.ascontiguousarray(np.asarray(to, np.float64).reshape(-1, 8))
    if len(a) != len(b):
        raise ValueError("%s: %d start and %d end configurations" % (what, len(a), len(b)))
    return a, b


def _returned_path(what, rc, out, n_out, info):
    """(path (m, 8), info dict) of a call that hands back a path buffer, which is freed here; a failure raises SmpError
    with the dict as its `info` attribute."""
    d = {f: getattr(info, f) for f, _ in info._fields_}
    if rc != L.SMP_OK:
        err = L.SmpError(rc, what)
        err.info = d
        raise err
    try:
        res = np.ctypeslib.as_array(out, shape=(n_out.value, 8)).copy()
    finally:
        lib().smp_buffer_free(out)
    return res, d


def _result_dict(r):
    s = r.stats
    d = {f: getattr(s, f) for f, _ in L.Stats._fields_}
    d["cost_best"] = list(s.cost_best)
    d["cost_theoretical"] = list(s.cost_theoretical)
    names = ["sample", "nearest", "expand", "near", "choose_parent", "rewire", "connect", "collide_tiles",
             "n_tiles", "edge_costs", "via_chains", "n_via_steps", "tile_local_frames|job_publish", "tile_chain|job_own_tiles",
             "tile_centres_w0|job_wait", "tile_tests|n_jobs", "tiles_in_expand", "tiles_in_choose", "tiles_in_rewire",
             "tiles_in_connect", "checked_expand", "checked_choose", "checked_rewire", "checked_connect",
             "slots_expand", "slots_choose", "slots_rewire", "slots_connect"]
    d["phases"] = {n: s.phase_seconds[i] for i, n in enumerate(names)}
    d["phase_raw"] = list(s.phase_seconds)
    d["scout_phases"] = list(s.scout_phase_seconds)
    d["status"] = r.status
    n = r.n_waypoints
    d["path"] = np.ctypeslib.as_array(r.waypoints, shape=(n, 8)).copy() if n else np.zeros((0, 8))
    m = r.n_cost_rows
    d["cost_rows"] = np.ctypeslib.as_array(r.cost_rows, shape=(m, 5)).copy() if m else np.zeros((0, 5))
    return d


class BiRRTstarPlanner:
    """Drop-in mirror of birrt_star_motion_planning::BiRRTstarPlanner for the C-space (search_space = 1) path.

    Call sequence of the node (squirrel_8dof_planner.cpp:1221-1248):
        initialize(); setOctree(...); setDisabledLinkMapCollisions([...]);
        reset_planner_and_config(); setPlanningSceneInfo(x, y, name);
        init_planner(start, goal, 1, self, map) -> bool; run_planner(1, 1, T, False, 0.0, n) -> bool;
        getJointTrajectoryRef()
    Extra (not in the reference): seed / query_id for reproducible runs, `stats` of the last run.
    """

    def __init__(self, device=0, seed=1):
        self.device = device
        self.seed = seed
        self.query_id = 0
        self._gpu = None
        self._detached = None  # the robot before attachObject, while an object is attached
        self._self_filter = False
        self._env = [(0.0, 0.0), (0.0, 0.0)]
        self._start = self._goal = None
        self._flags = (True, True)
        self._traj = []
        self.stats = None

    def initialize(self, planning_group="robotino_robot", **params):
        if planning_group != "robotino_robot":
            raise ValueError("only the robotino_robot group (robotino_plan.srdf:4-6) is modelled")
        self._gpu = GpuPlanner(device=self.device, **params)

    def setOctree(self, octree, resolution=None, floor_center=None, floor_distance=3.0):
        """octree: .bt or .ot file bytes, or an (n, 3) array of occupied octomap keys (then `resolution` is
        required).  The first line tells the formats apart (AbstractOcTree::read / OcTree::readBinary)."""
        if self._self_filter:
            # the self filter lives in the device scene build (same arrays as the host path, carved)
            if isinstance(octree, (bytes, bytearray)):
                full = bytes(octree).startswith(b"# Octomap OcTree file")
                (self._gpu.set_scene_ot if full else self._gpu.set_scene_bt)(octree, floor_center=floor_center,
                                                                              floor_distance=floor_distance)
            else:
                self._gpu.set_scene_keys(octree, resolution, floor_center=floor_center, floor_distance=floor_distance)
            return
        if isinstance(octree, (bytes, bytearray)):
            full = bytes(octree).startswith(b"# Octomap OcTree file")
            sc = (Scene.from_ot if full else Scene.from_bt)(octree, floor_center=floor_center,
                                                            floor_distance=floor_distance)
        else:
            sc = Scene.from_keys(octree, resolution, floor_center=floor_center, floor_distance=floor_distance)
        self._gpu.set_scene(sc)

    def setDisabledLinkMapCollisions(self, links):
        self._gpu.set_disabled_map_links(list(links))

    def attachObject(self, link, centres, radii, name="attached_object", touch_links=()):
        """Not in the reference (birrt_star.h:411-414 keeps attached objects as a stub): after a grasp, the object as
        spheres in `link`'s frame becomes a collision link `name` of the planner's robot (Robot.attach, then
        GpuPlanner.set_robot); every later check, plan and pass honours it.  Further objects stack."""
        if not self._detached:
            self._detached = self._gpu.robot
        self._gpu.set_robot(self._gpu.robot.attach(link, centres, radii, name, touch_links))

    def attachBox(self, link, half, pose=None, tol=0.01, name="attached_object", touch_links=(), max_spheres=16):
        """Not in the reference: attachObject for a bounding box (half extents, placed in `link`'s frame by pose = R
        row-major then p; None: centred on the frame), covered by cover_box within `tol`."""
        centres, radii = cover_box(half, pose, tol, max_spheres)
        self.attachObject(link, centres, radii, name, touch_links)

    def setSelfFilter(self, pose_current=None, pad=0.0, links=None):
        """Not in the reference: before each setOctree, the pose the octomap was taken at (poseCurrent).  The robot's
        own voxels -- all collision links, or `links`, e.g. the grasped object's name -- grown by pad metres are then
        carved out of the map inside setOctree.  pose_current=None turns the filter off."""
        self._gpu.set_carve(pose_current, pad, links)
        self._self_filter = pose_current is not None

    def detachObject(self):
        """Not in the reference: after the release, the robot as it was before the first attachObject."""
        if self._detached:
            self._gpu.set_robot(self._detached)
            self._detached = None

    def setPlanningSceneInfo(self, size_x, size_y, scene_name="scenario"):
        self._env = [(float(size_x[0]), float(size_x[1])), (float(size_y[0]), float(size_y[1]))]

    def reset_planner_and_config(self):
        self._env = [(0.0, 0.0), (0.0, 0.0)]
        self._start = self._goal = None
        self._traj = []

    def isConfigValid(self, config, check_self_collision=True, check_map_collision=True):
        return bool(self._gpu.check_configs([config], check_self_collision, check_map_collision)[0])

    def isEdgeValid(self, start_conf, end_conf, check_self_collision=True, check_map_collision=True):
        """birrt_star.h:103-104 for the edge start_conf -> end_conf: (valid, last_valid_node_idx), the index as the
        reference leaves it (birrt_star.cpp:6878-6895): the last point of a free edge, else the last free point before
        the first colliding one (0 when the first point collides)."""
        first, npts = self._gpu.check_edges([start_conf], [end_conf], check_self_collision, check_map_collision)
        f = int(first[0])
        return f < 0, (int(npts[0]) - 1 if f < 0 else max(f - 1, 0))

    def isEdgeClear(self, start_conf, end_conf, margin, check_self_collision=True, check_map_collision=True):
        """Not in the reference: isEdgeValid with a safety margin = (map, self) in metres (GpuPlanner.check_edges):
        (clear, last_clear_node_idx), the index read as isEdgeValid's."""
        first, npts = self._gpu.check_edges([start_conf], [end_conf], check_self_collision, check_map_collision,
                                            margin=margin)
        f = int(first[0])
        return f < 0, (int(npts[0]) - 1 if f < 0 else max(f - 1, 0))

    def shortcutTrajectory(self, trajectory, check_self_collision=True, check_map_collision=True, window=0,
                           margin=None):
        """Shortens `trajectory` (a list of 8-value poses, e.g. getJointTrajectoryRef()) in place
        (GpuPlanner.shortcut_path); False, trajectory untouched, when the path is blocked or has fewer than two poses.
        The node would call it between getJointTrajectoryRef and normalizeTrajectory.  `shortcut_info` keeps the
        call's counts, costs and timing.  margin = (map, self) in metres keeps the route that far from the map and
        from self-collision (GpuPlanner.shortcut_path's margin)."""
        if len(trajectory) < 2:
            return False
        try:
            path, self.shortcut_info = self._gpu.shortcut_path(trajectory, check_self_collision, check_map_collision,
                                                               window, margin=margin)
        except L.SmpError as e:
            if e.status != L.SMP_ERR_NO_SOLUTION:
                raise
            self.shortcut_info = e.info
            return False
        trajectory[:] = [list(map(float, w)) for w in path]
        return True

    def repairTrajectory(self, trajectory, check_self_collision=True, check_map_collision=True, samples=256,
                         rounds=4, seed=1, margin=None):
        """Repairs `trajectory` (a list of 8-value poses, e.g. getJointTrajectoryRef()) in place
        (GpuPlanner.repair_path): its blocked stretches are bridged by one-via detours and the via nodes of every edge
        are inserted.  False, trajectory untouched, when a stretch stays blocked, an end pose is invalid or there are
        fewer than two poses.  The node would call it between getJointTrajectoryRef and shortcutTrajectory.
        `repair_info` keeps the call's counts, costs and timing.  margin = (map, self) in metres repairs every stretch
        that is not clear at those margins (GpuPlanner.repair_path's margin); repair with a margin, then shortcut with
        the same one."""
        if len(trajectory) < 2:
            return False
        try:
            path, self.repair_info = self._gpu.repair_path(trajectory, check_self_collision, check_map_collision,
                                                           samples, rounds, seed, margin=margin)
        except L.SmpError as e:
            if e.status not in (L.SMP_ERR_NO_SOLUTION, L.SMP_ERR_START_INVALID, L.SMP_ERR_GOAL_INVALID):
                raise
            self.repair_info = e.info
            return False
        trajectory[:] = [list(map(float, w)) for w in path]
        return True

    def getClearance(self, joint_positions, max_dist=0.3, check_self_collision=True, check_map_collision=True):
        """Not in the reference: the configuration's distance to the map and to self-collision with the nearest links
        (GpuPlanner.clearance), as a dict of map, map_link, self, self_links (link names, None where there is none)."""
        r = self._gpu.clearance([joint_positions], max_dist, check_self_collision, check_map_collision)[0]
        names = self._gpu.robot.link_names
        name = lambda l: names[l] if l >= 0 else None
        return dict(map=float(r["map"]), map_link=name(int(r["map_link"])), self=float(r["self"]),
                    self_links=(name(int(r["self_a"])), name(int(r["self_b"]))))

    def getEdgeClearance(self, start_conf, end_conf, max_dist=0.3, check_self_collision=True,
                         check_map_collision=True):
        """The same along the dense edge start_conf -> end_conf (isEdgeValid's points): the minima, the lowest points
        attaining them and those points' links (GpuPlanner.edge_clearance), as a dict."""
        r = self._gpu.edge_clearance([start_conf], [end_conf], max_dist, check_self_collision, check_map_collision)[0]
        names = self._gpu.robot.link_names
        name = lambda l: names[l] if l >= 0 else None
        return dict(map=float(r["map"]), map_point=int(r["map_point"]), map_link=name(int(r["map_link"])),
                    self=float(r["self"]), self_point=int(r["self_point"]),
                    self_links=(name(int(r["self_a"])), name(int(r["self_b"]))), n_points=int(r["n_points"]))

    def getTrajectoryClearance(self, max_dist=0.3, check_self_collision=True, check_map_collision=True):
        """GpuPlanner.path_clearance's summary for the last planned trajectory (getJointTrajectoryRef); None when it
        has fewer than two poses."""
        if len(self._traj) < 2:
            return None
        return self._gpu.path_clearance(self._traj, max_dist, check_self_collision, check_map_collision)[1]

    def getCollisions(self, joint_positions, self_collisions, map_collisions):
        """birrt_star.cpp:6910-6914: appends to the two lists, as the reference does."""
        s, m = self._gpu.get_collisions(joint_positions)
        self_collisions.extend(s)
        map_collisions.extend(m)

    def init_planner(self, start_conf, goal_conf, search_space=1, check_self_collision=True, check_map_collision=True):
        if len(start_conf) != 8 or len(goal_conf) != 8 or search_space != 1:
            return False  # birrt_star.cpp:338-342 (control-space search is out of scope)
        v = self._gpu.check_configs([start_conf, goal_conf], check_self_collision, check_map_collision)
        if not v[0] or not v[1]:
            return False  # birrt_star.cpp:350-362
        self._start, self._goal = list(start_conf), list(goal_conf)
        self._flags = (check_self_collision, check_map_collision)
        return True

    def run_planner(self, search_space=1, flag_iter_or_time=1, max_iter_time=30.0, show_tree_vis=False,
                    iter_sleep=0.0, planner_run_number=0):
        if self._start is None or search_space != 1:
            return False
        kw = dict(seconds=max_iter_time) if flag_iter_or_time else dict(iterations=int(max_iter_time))
        q = GpuPlanner.make_query(self._start, self._goal, self._env[0], self._env[1], self._flags[0],
                                  self._flags[1], seed=self.seed, query_id=self.query_id, **kw)
        r = self._gpu.plan(q)
        self.stats = r
        if r["status"] not in (L.SMP_OK, L.SMP_ERR_NO_SOLUTION):
            raise L.SmpError(r["status"], "run_planner")
        self._traj = [list(map(float, w)) for w in r["path"]]
        return r["status"] == L.SMP_OK

    def run_planner_far(self, flag_iter_or_time=1, max_iter_time=30.0, **opts):
        """Not in the reference, where the branch is dead (squirrel_8dof_planner.cpp:505-508, 595-598): run_planner for
        a goal across the room, the node's two-stage plan (GpuPlanner.plan_far) -- opts: arm (pose_folded_arm),
        map_margin (astar_safety_distance), handover_distance (distance_birrt_star_planning), pitch, n_theta, window,
        snap_cells, route_device.  `far_info` keeps the stages' record; the trajectory is the base stage's
        far_info["n_route_rows"] rows followed by the 8-DoF plan's."""
        if self._start is None:
            return False
        kw = dict(seconds=max_iter_time) if flag_iter_or_time else dict(iterations=int(max_iter_time))
        q = GpuPlanner.make_query(self._start, self._goal, self._env[0], self._env[1], self._flags[0],
                                  self._flags[1], seed=self.seed, query_id=self.query_id, **kw)
        r = self._gpu.plan_far(q, **opts)
        self.stats, self.far_info = r, r["far"]
        if r["status"] not in (L.SMP_OK, L.SMP_ERR_NO_SOLUTION, L.SMP_ERR_START_INVALID, L.SMP_ERR_GOAL_INVALID):
            raise L.SmpError(r["status"], "run_planner_far")
        self._traj = [list(map(float, w)) for w in r["path"]] if r["status"] == L.SMP_OK else []
        return r["status"] == L.SMP_OK

    def getJointTrajectoryRef(self):
        return self._traj

    def getFullPoseFromEEPose(self, endEffectorPose, endEffectorDeviations, poseInit, poseSolution):
        """birrt_star.cpp:1627-1686: the VDLS controller from poseInit towards endEffectorPose (x, y, z, roll, pitch,
        yaw); on REACHED fills the list poseSolution with the final configuration and returns True."""
        r = self._gpu.ik_solve([endEffectorPose], [poseInit], deviation=endEffectorDeviations)
        if not r["reached"][0]:
            return False
        poseSolution[:] = [float(v) for v in r["q"][0]]
        return True


def normalize_trajectory(raw, normalized_pose):
    """Planner::normalizeTrajectory (squirrel_8dof_planner.cpp:1557-1637) through the C ABI: the resampled poses as
    an (m, dim) array, or None where the reference returns without touching its output (dim < 1, <= 1 pose)."""
    np_ = np.ascontiguousarray(np.asarray(normalized_pose, np.float64).reshape(-1))
    raw = np.ascontiguousarray(np.asarray(raw, np.float64))
    dim = len(np_)
    if raw.ndim != 2 or len(raw) <= 1 or dim < 1 or raw.shape[1] != dim:
        return None
    n_out = ctypes.c_int64()
    check(lib().smp_normalize_trajectory(raw.ctypes.data_as(_pd), len(raw), dim, np_.ctypes.data_as(_pd), None, 0,
                                         ctypes.byref(n_out)), "smp_normalize_trajectory")
    out = np.zeros((n_out.value, dim))
    check(lib().smp_normalize_trajectory(raw.ctypes.data_as(_pd), len(raw), dim, np_.ctypes.data_as(_pd),
                                         out.ctypes.data_as(_pd), n_out.value, ctypes.byref(n_out)),
          "smp_normalize_trajectory")
    return out
