"""ctypes driver of the C++ facade (``lib/libohm_tsd_slam.so``): ``ThreadLocalize`` / ``ThreadMapping``
wired as ``SlamNode::initialize`` wires them (SlamNode.cpp:27-129), fed through ``laserCallBack``.
Used by the tests and by ``bench.py``; the facade itself is C++ (``csrc/host``)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(capi.LIB_DIR, "libohm_tsd_slam.so")

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_ip = C.POINTER(C.c_int)

HOST_ABI = {
    "tsd_node_create": (C.c_void_p, [C.c_char_p]),
    "tsd_node_set_double": (None, [C.c_void_p, C.c_char_p, C.c_double]),
    "tsd_node_set_int": (None, [C.c_void_p, C.c_char_p, C.c_int]),
    "tsd_node_set_bool": (None, [C.c_void_p, C.c_char_p, C.c_int]),
    "tsd_node_set_string": (None, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "tsd_node_initialize": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_node_declared_parameters": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "tsd_node_set_synchronous": (None, [C.c_void_p, C.c_int]),
    "tsd_node_set_fused": (None, [C.c_void_p, C.c_int]),
    "tsd_node_laser": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int, C.c_double, C.c_double, C.c_longlong]),
    "tsd_node_start_at": (C.c_int, [C.c_void_p, C.c_int, _dp, _fp, C.c_int, C.c_double, C.c_double, C.c_longlong]),
    "tsd_node_wait_idle": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_node_processed": (C.c_ulonglong, [C.c_void_p, C.c_int]),
    "tsd_node_report": (None, [C.c_void_p, C.c_int, _dp]),
    "tsd_node_pose_msg": (None, [C.c_void_p, C.c_int, _dp]),
    "tsd_node_preregistration": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "tsd_node_pose_topic": (C.c_char_p, [C.c_void_p, C.c_int]),
    "tsd_node_tf_msg": (None, [C.c_void_p, C.c_int, _dp, C.c_char_p, C.c_int]),
    "tsd_node_set_transform": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, _dp, _dp]),
    "tsd_node_laser_ahead": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int, C.c_double, C.c_double, C.c_longlong]),
    "tsd_node_play": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_fp), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, C.c_longlong]),
    "tsd_node_batch_stats": (None, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "tsd_node_grid_ctx": (C.c_void_p, [C.c_void_p]),
    "tsd_node_publish_map": (C.c_int, [C.c_void_p]),
    "tsd_node_map_frames": (C.c_ulonglong, [C.c_void_p]),
    "tsd_node_map_updates": (C.c_ulonglong, [C.c_void_p]),
    "tsd_node_map_update_msg": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_surface": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_map_msg": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_costmaps": (C.c_ulonglong, [C.c_void_p]),
    "tsd_node_costmap_radius": (C.c_int, [C.c_void_p]),
    "tsd_node_costmap": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int, C.c_char_p, C.c_int]),
    "tsd_node_costmap_update": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_frontier_cloud": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_frontier_min_size": (C.c_uint, [C.c_void_p]),
    "tsd_node_frontiers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, _ip, _ip, C.c_void_p, _ip, _dp]),
    "tsd_node_frontiers_fetch": (None, [C.c_void_p, C.c_void_p]),
    "tsd_fleet_frontiers": (C.c_int, [C.c_void_p, C.c_uint, _ip, _ip, C.c_void_p, _ip, _dp]),
    "tsd_node_frontier_lock": (None, [C.c_void_p]),
    "tsd_node_frontier_unlock": (None, [C.c_void_p]),
    "tsd_fleet_frontiers_fetch": (None, [C.c_void_p, C.c_void_p]),
    "tsd_node_explore_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, _ip,
                                        C.POINTER(capi.RouteInfo), C.c_void_p, _ip, _dp]),
    "tsd_node_explore_plan_fetch": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_fleet_explore_plan": (C.c_int, [C.c_void_p, C.c_uint, C.c_int, _ip, C.POINTER(capi.RouteInfo), C.c_void_p, _ip, _dp]),
    "tsd_fleet_explore_plan_fetch": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_node_explore_gains": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_void_p, _ip]),
    "tsd_fleet_explore_assign": (C.c_int, [C.c_void_p, C.c_double, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, _ip, _ip]),
    "tsd_node_explore_waypoints": (C.c_int, [C.c_void_p, C.c_double, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _ip]),
    "tsd_fleet_explore_waypoints": (C.c_int, [C.c_void_p, C.c_double, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _ip]),
    "tsd_fleet_explore_dispatch": (C.c_int, [C.c_void_p, C.c_uint, C.c_double, C.c_uint, C.c_int, C.c_double, C.c_uint, C.c_int, C.c_int, _ip,
                                             C.POINTER(capi.RouteFieldsInfo), C.c_void_p, _dp]),
    "tsd_fleet_explore_dispatch_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_node_explore_drive": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, C.c_int, _dp, C.c_void_p, _ip, _dp]),
    "tsd_fleet_explore_drive": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, C.c_int, _dp, C.c_void_p, _ip, _dp]),
    "tsd_fleet_explore_drive_apart": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, C.c_int, C.c_double, C.c_void_p, C.c_int, _dp, C.c_void_p, _ip, _dp,
                                                C.c_void_p, C.c_void_p, _dp, C.c_int]),
    "tsd_node_explore_drive_live": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, _dp,
                                              C.c_void_p, _ip, _dp, _ip, _ip]),
    "tsd_fleet_explore_drive_live": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, C.c_int, C.c_double, C.c_void_p, C.c_int, _dp, C.c_int, C.c_double,
                                               C.c_double, _dp, C.c_void_p, _ip, _dp, C.c_void_p, C.c_void_p, _dp, C.c_int, _ip, C.c_void_p]),
    "tsd_node_get_map": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_map_image_msg": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_node_grid_lock": (None, [C.c_void_p]),
    "tsd_node_grid_unlock": (None, [C.c_void_p]),
    "tsd_node_destroy": (None, [C.c_void_p]),
    "tsd_fleet_create": (C.c_void_p, [C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    "tsd_fleet_destroy": (None, [C.c_void_p]),
    "tsd_fleet_publish_merged": (C.c_int, [C.c_void_p]),
    "tsd_fleet_merged_frames": (C.c_ulonglong, [C.c_void_p]),
    "tsd_fleet_merged_map_msg": (C.c_ulonglong, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_fleet_get_merged_map": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_fleet_fuse_tsd": (C.c_void_p, [C.c_void_p, _ip]),
    "tsd_fleet_set_transforms": (C.c_int, [C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_fleet_fused_lock": (None, [C.c_void_p]),
    "tsd_fleet_fused_unlock": (None, [C.c_void_p]),
    "tsd_fleet_fused_image_msg": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_char_p, C.c_int]),
    "tsd_host_sensor_ingest_f32": (None, [_fp, C.c_int, C.c_double, C.c_double, C.c_double, _dp, _u8p, C.c_int]),
    "tsd_host_sensor_chain": (None, [C.c_int, C.c_double, C.c_double, _dp, _dp, C.c_double, _fp, _dp, _dp, _dp,
                                     _dp, _u8p, _ip]),
    "tsd_host_calc_angle": (C.c_double, [_dp]),
    "tsd_host_is_registration_error": (C.c_int, [_dp, C.c_double, C.c_double]),
    "tsd_host_is_pose_change_significant": (C.c_int, [_dp, _dp]),
    "tsd_host_mat3_inv": (None, [_dp, _dp]),
    "tsd_host_backproject": (C.c_int, [_dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]),
}

_lib = None


def load_library():
    global _lib
    if _lib is None:
        capi.load_library()   # dependency (resolved through rpath as well)
        if not os.path.exists(LIB_PATH):
            raise capi.TsdError(f"{LIB_PATH} not found: run __graft_entry__.build()")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in HOST_ABI.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


REPORT_FIELDS = ("rms", "pairs", "iterations", "icp_state", "valid_model", "valid_scene", "reg_error", "pushed",
                 "no_model", "initialised")


def declared_parameters(params: dict | None = None, name: str = "tsd_slam") -> dict:
    """(type, declared default) of every parameter the facade declares for a node configured with `params` -- SlamNode,
    the ThreadLocalize constructors and ThreadLocalize::init -- without touching a device."""
    lib = load_library()
    h = lib.tsd_node_create(name.encode())
    for k, v in (params or {}).items():
        kb = k.encode()
        if isinstance(v, bool):
            lib.tsd_node_set_bool(h, kb, int(v))
        elif isinstance(v, int):
            lib.tsd_node_set_int(h, kb, v)
        elif isinstance(v, float):
            lib.tsd_node_set_double(h, kb, v)
        else:
            lib.tsd_node_set_string(h, kb, str(v).encode())
    need = lib.tsd_node_declared_parameters(h, None, 0)
    buf = C.create_string_buffer(need)
    lib.tsd_node_declared_parameters(h, buf, need)
    lib.tsd_node_destroy(h)
    out = {}
    for line in buf.value.decode().splitlines():
        k, t, v = line.split("|", 2)
        out[k] = (t, {"bool": lambda x: x == "true", "int": int, "double": float, "string": str}[t](v))
    return out


class SlamNode:
    """``SlamNode`` wiring: parameters (SURVEY Appendix D names), one grid, one mapping thread, N
    localisers.  ``synchronous=True`` runs the event-loop body inside ``laser()`` (strict
    ray-cast -> ICP -> push order); otherwise the reference's threads/queues are used."""

    def __init__(self, params: dict, device: int = 0, synchronous: bool = True, name: str = "tsd_slam",
                 fused: bool = True):
        self.lib = load_library()
        self.h = self.lib.tsd_node_create(name.encode())
        for k, v in params.items():
            kb = k.encode()
            if isinstance(v, bool):
                self.lib.tsd_node_set_bool(self.h, kb, int(v))
            elif isinstance(v, int):
                self.lib.tsd_node_set_int(self.h, kb, v)
            elif isinstance(v, float):
                self.lib.tsd_node_set_double(self.h, kb, v)
            else:
                self.lib.tsd_node_set_string(self.h, kb, str(v).encode())
        self.lib.tsd_node_set_synchronous(self.h, int(synchronous))
        self.lib.tsd_node_set_fused(self.h, int(fused))
        rc = self.lib.tsd_node_initialize(self.h, device)
        if rc != 0:
            self.lib.tsd_node_destroy(self.h)
            self.h = None
            raise capi.TsdError(f"tsd_node_initialize failed ({rc}): no usable GPU; the hot path has no CPU fall-back")
        self._stamp = 0
        self._params, self._name, self._declared = dict(params), name, None

    def robot_parameters(self, robot: int = 0) -> dict:
        """What the robot's localiser reads from the node's parameters -- ThreadLocalize's constructor (laser_min_range, icp_iterations,
        dist_filter_max / _min) and ThreadLocalize::init (max_range, min_range) -- as set for this node or as declared by default."""
        if self._declared is None:
            self._declared = {k: v for k, (_, v) in declared_parameters(self._params, self._name).items()}
        d = self._declared
        prefix = ""
        if d["robot_nbr"] > 1:
            prefix = d[f"robot_{robot}/name"]
            prefix += "" if prefix.endswith("/") or not prefix else "/"
        out = {"laser_min_range": d["laser_min_range"]}
        out.update({k: d[prefix + k] for k in ("icp_iterations", "dist_filter_max", "dist_filter_min")})
        out.update({k: d[f"{self._name}/{prefix}{k}"] for k in ("max_range", "min_range")})
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_node_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_synchronous(self, on: bool):
        self.lib.tsd_node_set_synchronous(self.h, int(on))

    def laser(self, ranges_f32, angle_min, angle_increment, robot: int = 0, stamp_ns: int | None = None, ahead=None):
        """``ahead``: the scan the NEXT call will deliver (known in a replay): announced to the localiser, which stages it on
        the device while this scan's registration runs."""
        r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
        if stamp_ns is None:
            self._stamp += 25_000_000
            stamp_ns = self._stamp
        if ahead is not None:
            a = np.ascontiguousarray(ahead, dtype=np.float32)
            self.lib.tsd_node_laser_ahead(self.h, robot, a.ctypes.data_as(_fp), a.size, angle_min, angle_increment, stamp_ns + 25_000_000)
        rc = self.lib.tsd_node_laser(self.h, robot, r.ctypes.data_as(_fp), r.size, angle_min, angle_increment, stamp_ns)
        if rc != 0:
            raise capi.TsdError(f"tsd_node_laser failed ({rc})")

    def start_at(self, pose, ranges_f32, angle_min, angle_increment, robot: int = 0, stamp_ns: int | None = None):
        """ThreadLocalize::startAt: start the robot's localiser at the sensor pose ``pose`` (3 x 3) with ``ranges_f32`` as its first scan
        -- no freeFootprint, no initial push: the map in the grid stays as it is -- or re-seat a running one there."""
        r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
        p = np.ascontiguousarray(pose, dtype=np.float64).reshape(9)
        if stamp_ns is None:
            self._stamp += 25_000_000
            stamp_ns = self._stamp
        rc = self.lib.tsd_node_start_at(self.h, robot, p.ctypes.data_as(_dp), r.ctypes.data_as(_fp), r.size, angle_min,
                                        angle_increment, stamp_ns)
        if rc != 0:
            raise capi.TsdError(f"tsd_node_start_at failed ({rc}): scans of the robot are still queued or being processed")

    def relocalize(self, ranges_f32, angle_min, angle_increment, x0, y0, step_xy, nx, ny, ntheta, theta0=0.0, dtheta=0.0,
                   cos_sin=None, theta_wraps=False, K=16, min_pairs=0, robot: int = 0) -> dict:
        """Find the scan in the grid's map and, when found, start (or re-seat) the robot's localiser there: the scan is ingested the
        way laserCallBack and SensorPolar2D do it, ``TsdGridDevice.relocalize`` searches the lattice and refines its peaks, and
        ``start_at`` takes the pose.  The ranges' limits and the registration's parameters are the robot's own, read from the node's
        parameters (``robot_parameters``).  Returns relocalize's dict."""
        prm = self.robot_parameters(robot)
        max_range, min_range = prm["max_range"], prm["min_range"]
        r = np.array(ranges_f32, dtype=np.float32)
        r[r < prm["laser_min_range"]] = 0.0                                # ThreadLocalize::clampRanges
        n = r.size
        scan_geometry = (angle_min, angle_increment)                       # (start_at takes the scan as the driver delivered it)
        if angle_increment < 0.0 and angle_min > 0:                        # clockwise scanner (ThreadLocalize.cpp:491-497)
            r, angle_min, angle_increment = r[::-1].copy(), -angle_min, -angle_increment
        data, mask = np.zeros(n), np.zeros(n, dtype=np.uint8)
        self.lib.tsd_host_sensor_ingest_f32(r.ctypes.data_as(_fp), n, angle_increment, angle_min, max_range, data.ctypes.data_as(_dp),
                                            mask.ctypes.data_as(_u8p), 0)
        eye = np.eye(3).reshape(9)
        pose, rays, rays_local, scene = np.zeros(9), np.zeros(2 * n), np.zeros(2 * n), np.zeros(2 * n)
        smask, valid = np.zeros(n, dtype=np.uint8), C.c_int(0)
        self.lib.tsd_host_sensor_chain(n, angle_increment, angle_min, eye.ctypes.data_as(_dp), eye.ctypes.data_as(_dp), 1.0,
                                       r.ctypes.data_as(_fp), pose.ctypes.data_as(_dp), rays.ctypes.data_as(_dp),
                                       rays_local.ctypes.data_as(_dp), scene.ctypes.data_as(_dp), smask.ctypes.data_as(_u8p), C.byref(valid))
        points = scene.reshape(-1, 2)[smask.astype(bool)]
        g = self.grid()
        icp = g.icp_params(prm["icp_iterations"], prm["dist_filter_max"], prm["dist_filter_min"])
        out = g.relocalize(points, rays_local, data, mask, min_range, max_range, icp, x0, y0, step_xy, nx, ny, ntheta, theta0=theta0,
                           dtheta=dtheta, cos_sin=cos_sin, theta_wraps=theta_wraps, K=K, min_pairs=min_pairs)
        if out["found"]:
            self.start_at(out["pose"], ranges_f32, *scan_geometry, robot=robot)
        return out

    def play(self, scans, first: int, count: int, angle_min, angle_increment):
        """Replay scans[r][first:first+count] of every robot r from one native publisher thread per robot (`rosbag play`):
        ``scans`` = list (one per robot) of C-contiguous float32 arrays [n_scans, beams]."""
        arrs = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
        ptrs = (_fp * len(arrs))(*[a.ctypes.data_as(_fp) for a in arrs])
        rc = self.lib.tsd_node_play(self.h, len(arrs), ptrs, first, count, arrs[0].shape[1], angle_min, angle_increment,
                                    self._stamp + 25_000_000, 25_000_000)
        self._stamp += 25_000_000 * (first + count)
        if rc != 0:
            raise capi.TsdError(f"tsd_node_play failed ({rc})")

    def batch_stats(self):
        b, s = C.c_ulonglong(0), C.c_ulonglong(0)
        self.lib.tsd_node_batch_stats(self.h, C.byref(b), C.byref(s))
        return int(b.value), int(s.value)

    def wait_idle(self, timeout_ms: int = 10000) -> bool:
        return self.lib.tsd_node_wait_idle(self.h, timeout_ms) == 0

    def processed(self, robot: int = 0) -> int:
        return int(self.lib.tsd_node_processed(self.h, robot))

    def report(self, robot: int = 0) -> dict:
        buf = np.zeros(29)
        self.lib.tsd_node_report(self.h, robot, buf.ctypes.data_as(_dp))
        out = {"pose": buf[:9].reshape(3, 3).copy(), "T": buf[9:18].reshape(3, 3).copy()}
        out["rms"] = float(buf[18])
        for i, k in enumerate(REPORT_FIELDS[1:]):
            out[k] = int(buf[19 + i])
        out["stamp_ns"] = int(buf[28])
        return out

    def preregistration(self, robot: int = 0) -> dict | None:
        """the robot's last pre-registration (registration_modes 1 and 2; mode 3 where it ran unfused), None if there was none.
        `prob` is the winning probability in modes 2 and 3 and bestRatio (cntMatch / maxCntMatch of the winner) in mode 1."""
        buf = np.zeros(16)
        if not self.lib.tsd_node_preregistration(self.h, robot, buf.ctypes.data_as(_dp)):
            return None
        return dict(T=buf[:9].reshape(3, 3).copy(), prob=float(buf[9]), idx=int(buf[10]), i=int(buf[11]), candidates=int(buf[12]),
                    valid_model=int(buf[13]), valid_scene=int(buf[14]), control=int(buf[15]))

    def pose_msg(self, robot: int = 0) -> dict:
        buf = np.zeros(8)
        self.lib.tsd_node_pose_msg(self.h, robot, buf.ctypes.data_as(_dp))
        return {"position": buf[:3].copy(), "orientation_xyzw": buf[3:7].copy(), "count": int(buf[7]),
                "topic": self.lib.tsd_node_pose_topic(self.h, robot).decode()}

    def tf_msg(self, robot: int = 0) -> dict:
        """the last TransformStamped the robot's tf broadcaster sent (map -> odom, ThreadLocalize.cpp:603-689)"""
        buf = np.zeros(8)
        frames = C.create_string_buffer(256)
        self.lib.tsd_node_tf_msg(self.h, robot, buf.ctypes.data_as(_dp), frames, 256)
        parent, child = frames.value.decode().split("|")
        return {"translation": buf[:3].copy(), "rotation_xyzw": buf[3:7].copy(), "count": int(buf[7]),
                "frame_id": parent, "child_frame_id": child}

    def set_transform(self, parent: str, child: str, xyz, q_xyzw, robot: int = 0):
        """feed the robot's tf buffer (a TransformListener's job under ROS): frame `child` expressed in frame `parent`"""
        t = np.ascontiguousarray(xyz, dtype=np.float64)
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64)
        rc = self.lib.tsd_node_set_transform(self.h, robot, parent.encode(), child.encode(), t.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
        if rc != 0:
            raise ValueError("tsd_node_set_transform refused %s -> %s" % (parent, child))

    # ---- ThreadGrid (ThreadGrid.cpp:16-142): <node>/map, <node>/map/image, <node>/get_map
    def publish_map(self):
        """one ThreadGrid publication now, on the caller's thread (what every occ_grid_time_interval wake-up does)"""
        rc = self.lib.tsd_node_publish_map(self.h)
        if rc != 0:
            raise capi.TsdError(f"tsd_node_publish_map failed ({rc})")

    def map_frames(self) -> int:
        """ThreadGrid publications so far (timer wake-ups and publish_map())"""
        return int(self.lib.tsd_node_map_frames(self.h))

    @staticmethod
    def _map_dict(fn):
        info = np.zeros(12)
        frame = C.create_string_buffer(256)
        fn(None, info.ctypes.data_as(_dp), frame, 256)
        data = np.zeros(int(info[1]) * int(info[2]), dtype=np.int8)
        ret = fn(data.ctypes.data, info.ctypes.data_as(_dp), frame, 256)
        return ret, {"resolution": float(info[0]), "width": int(info[1]), "height": int(info[2]),
                     "origin_position": info[3:6].copy(), "origin_orientation_xyzw": info[6:10].copy(),
                     "stamp_ns": int(info[10]), "map_load_time_ns": int(info[11]), "frame_id": frame.value.decode(),
                     "data": data.reshape(int(info[2]), int(info[1]))}

    def map_msg(self) -> dict:
        """the last nav_msgs/OccupancyGrid on <node>/map (data as (height, width) int8) and its publish count"""
        n, m = self._map_dict(lambda d, i, f, c: self.lib.tsd_node_map_msg(self.h, d, i, f, c))
        m["count"] = int(n)
        return m

    def get_map(self) -> dict:
        """the get_map service's answer: the last map with a fresh stamp"""
        ok, m = self._map_dict(lambda d, i, f, c: self.lib.tsd_node_get_map(self.h, d, i, f, c))
        if not ok:
            raise capi.TsdError("get_map refused")
        return m

    def map_updates(self) -> int:
        """map_msgs/OccupancyGridUpdate messages on <node>/map_updates so far (parameter publish_map_updates)"""
        return int(self.lib.tsd_node_map_updates(self.h))

    def map_update_msg(self) -> dict:
        """the last map_msgs/OccupancyGridUpdate on <node>/map_updates (data as (height, width) int8) and the number published"""
        info = np.zeros(5)
        frame = C.create_string_buffer(256)
        self.lib.tsd_node_map_update_msg(self.h, None, info.ctypes.data_as(_dp), frame, 256)
        w, h = int(info[2]), int(info[3])
        data = np.zeros(w * h, dtype=np.int8)
        n = self.lib.tsd_node_map_update_msg(self.h, data.ctypes.data, info.ctypes.data_as(_dp), frame, 256)
        return {"x": int(info[0]), "y": int(info[1]), "width": w, "height": h, "stamp_ns": int(info[4]),
                "frame_id": frame.value.decode(), "data": data.reshape(h, w), "count": int(n)}

    def costmaps(self) -> int:
        """messages on <node>/costmap and <node>/costmap_updates so far (parameter publish_costmap; 0 with it off)"""
        return int(self.lib.tsd_node_costmaps(self.h))

    def costmap_radius_cells(self) -> int:
        """the inflation radius in cells: ceil(costmap_inflation_radius / cellsize), at most 255 (0 with publish_costmap off)"""
        return int(self.lib.tsd_node_costmap_radius(self.h))

    def costmap_msg(self) -> dict:
        """the last nav_msgs/OccupancyGrid on <node>/costmap (``map_msg``'s fields), its publish count and the topic's name
        (``topic`` None: the parameter is off, there is no such topic)"""
        topic = C.create_string_buffer(256)
        n, m = self._map_dict(lambda d, i, f, c: self.lib.tsd_node_costmap(self.h, d, i, f, c, topic, 256))
        m["count"] = int(n)
        m["topic"] = topic.value.decode() or None
        return m

    def costmap_update_msg(self) -> dict:
        """the last map_msgs/OccupancyGridUpdate on <node>/costmap_updates (``map_update_msg``'s fields) and the number published"""
        info = np.zeros(5)
        frame = C.create_string_buffer(256)
        self.lib.tsd_node_costmap_update(self.h, None, info.ctypes.data_as(_dp), frame, 256)
        w, h = int(info[2]), int(info[3])
        data = np.zeros(w * h, dtype=np.int8)
        n = self.lib.tsd_node_costmap_update(self.h, data.ctypes.data, info.ctypes.data_as(_dp), frame, 256)
        return {"x": int(info[0]), "y": int(info[1]), "width": w, "height": h, "stamp_ns": int(info[4]),
                "frame_id": frame.value.decode(), "data": data.reshape(h, w), "count": int(n)}

    def frontier_msg(self) -> dict:
        """the last sensor_msgs/PointCloud2 on <node>/frontiers (parameter publish_frontiers), one point per frontier of at least
        frontier_min_size cells in ascending root index: ``points`` as a structured array of FRONTIER_POINT -- float32 x y z, the
        centroid in the map's frame, (float32)((sum / size + 0.5) * resolution + origin) -- and the number published (0: no message)"""
        info = np.zeros(4)
        text = C.create_string_buffer(512)
        self.lib.tsd_node_frontier_cloud(self.h, None, info.ctypes.data_as(_dp), text, 512)
        w, step = int(info[0]), int(info[1])
        data = np.zeros(max(w * step, 1), dtype=np.uint8)
        n = self.lib.tsd_node_frontier_cloud(self.h, data.ctypes.data, info.ctypes.data_as(_dp), text, 512)
        frame, fields = text.value.decode().split("|")
        pts = data[:w * step].view(FRONTIER_POINT) if w and step == FRONTIER_POINT.itemsize else np.zeros(0, dtype=FRONTIER_POINT)
        return {"width": w, "height": 1 if n else 0, "point_step": step, "stamp_ns": int(info[2]), "frame_id": frame,
                "fields": [f for f in fields.split(",") if f], "points": pts, "count": int(n)}

    def frontier_min_size(self) -> int:
        return int(self.lib.tsd_node_frontier_min_size(self.h))

    def frontiers(self, seeds=None, min_size=None) -> dict:
        """The frontiers of the map published last (tsd_frontiers_frame), reachability included: ``records`` (capi.FRONTIER_DTYPE, at
        least ``min_size`` cells -- default frontier_min_size -- in ascending root index), ``centroids`` (n, 2) float64 in the map's
        frame [m], (sum / size + 0.5) * resolution + origin, ``seeds`` the (x, y) cells taken, ``seeds_used``.  seeds None: one per
        robot, the cell of its current pose; else (x, y) cells of the map."""
        if seeds is None:
            xy, ns = None, -1
        else:
            xy = np.ascontiguousarray(np.asarray(list(seeds), dtype=np.int32).reshape(-1, 2))
            ns = xy.shape[0]
        return _frontier_dict(lambda c, u, so, no, oc: self.lib.tsd_node_frontiers(
            self.h, None if xy is None or ns == 0 else xy.ctypes.data, ns, int(min_size or 0), c, u, so, no, oc),
            lambda out: self.lib.tsd_node_frontiers_fetch(self.h, out), "tsd_node_frontiers")

    def explore_plan(self, min_size=None, source="map", max_weight=1, max_len=4096) -> dict:
        """Where to drive next, in one call on the map published last: what ``frontiers()`` returns with the robot's cell as the
        seed, plus ``goals`` (capi.ROUTE_GOAL_DTYPE, one per frontier: the cheapest cell to reach, its cost d -- 5 per straight and 7
        per diagonal step, times the weight of the cell entered -- and the seed it is cheapest from; capi.ROUTE_NONE / -1 for a
        frontier the robot cannot reach), ``goal_xy`` (n, 2) float64 in the map's frame [m], (cell + 0.5) * resolution + origin (NaN
        without a goal), ``paths`` (a list of (len, 2) float64 arrays in metres, ordered seed to goal, the ``max_len`` cells nearest to
        the goal where the path is longer), ``path_lens`` (the full lengths in cells) and ``route`` (tsd_route_info as a dict).
        source "map": unit weights on the free cells; "costmap": the cost map of the last publication (parameter publish_costmap),
        traversable below the inscribed band, weights tsd_route_weights(98, max_weight)."""
        self._plan_goals = None
        out = _plan_dict(lambda c, i, so, no, oc: self.lib.tsd_node_explore_plan(
            self.h, None, -1, int(min_size or 0), capi.ROUTE_SOURCES[source], int(max_weight), int(max_len), c, i, so, no, oc),
            lambda *out: self.lib.tsd_node_explore_plan_fetch(self.h, *out), self.map_msg()["width"], max_len, "tsd_node_explore_plan")
        self._plan_goals = len(out["goals"])
        self._plan_frame = (self.map_msg()["width"], int(max_len), out["origin"], out["resolution"])
        return out

    def explore_waypoints(self, lookahead_m: float, slack=0, max_way=256) -> dict:
        """The paths of the plan made last straightened for a controller (tsd_route_waypoints): ``waypoints`` -- per goal an (n, 2)
        float64 array in the map's frame [m], (cell + 0.5) * resolution + origin, ordered seed to goal like ``explore_plan``'s paths,
        consecutive points joined by a straight segment that is drivable cell by cell under the routes' rule, spans at most
        ``lookahead_m`` of path (rounded to cells, at most capi.WAYPOINT_MAX_LOOKAHEAD: ``lookahead_cells``) and costs at most
        ``slack`` more than the stretch of path it replaces; cut at ``max_way`` points --, ``info`` (capi.WAYPOINT_INFO_DTYPE per
        goal: the path's len, the full count n_way -- 0 without a path and where the path is longer than the plan's ``max_len`` --,
        the segments' cost, the goal's dist).  Refused without a plan and once the map has been published again."""
        if getattr(self, "_plan_goals", None) is None:
            raise capi.TsdError("explore_waypoints: no plan (explore_plan first)")
        return _waypoint_dict(lambda *a: self.lib.tsd_node_explore_waypoints(self.h, *a), self._plan_goals, self._plan_frame, lookahead_m,
                              slack, max_way, "tsd_node_explore_waypoints")

    def explore_drive(self, goal: int, pose, v_max: float, w_max: float, horizon_s: float, footprint=None, n_speeds=5,
                      weights=(1, 1, 0, 0), nose_m=0.0, nose_miss=0, margin=2000, live_points=None, live_radius_m=0.0, live_skip_m=0.0) -> dict:
        """The velocity of the next step towards goal ``goal`` (an index into the goals of the plan made last) for a robot at
        ``pose`` = (x, y [m], yaw [rad]) in the map's frame: a cost-to-go field seeded AT the goal's cell on the plan's source
        (tsd_route_frame, limit: the goal's dist + ``margin``), then tsd_drive_rollout -- ``n_speeds`` speeds v_max * i / (V - 1) by
        the turns 0, +-1 .. +-round(w_max * dt * 4096 / 2 pi) headings per step of dt = resolution / v_max, over
        T = min(256, ceil(horizon_s / dt)) steps, every arc tested cell by cell with the ``footprint`` points ((x, y) [m] in the
        robot's frame, x forward) and rated by ``weights`` = (a_end, a_nose, a_cost, a_turn) on the field at its end and ``nose_m``
        ahead of it.  Returns ``v`` [m/s] and ``w`` [rad/s] (0 without an admissible arc: ``admissible`` == 0), ``end_xy`` (the arc's
        end cell [m], NaN without one), ``next_pose`` (x, y, yaw after one step), ``choice`` (capi.DRIVE_CHOICE_DTYPE), ``steps``,
        ``n_speeds``, ``n_turns``, ``n_body`` and ``dt``.  The goal-seeded field replaces the plan's route result on the device:
        ``explore_waypoints`` is refused from then on until the next ``explore_plan``.  Refused without a plan, once the map has been
        published again, for a goal without a cell, and where the turn list would exceed 129 entries.

        ``live_points``: the end points of the current scans, (N, 2) [m] in the map's frame (``scan_points``).  What the scanner sees
        this instant is on the published map only after the next publication; with the points given every arc that comes within
        ``live_radius_m`` (to the nearest cell) of one of them is refused as well (tsd_drive_live_set, reason 7 of the rule), but
        for the points within ``live_skip_m`` (rounded up to cells) of the robot's own pose, which are dropped.  The layer lives for
        this call only.  The answer then also holds ``live_kept`` (the points not dropped) and ``blocked_live`` (the samples the
        layer refused).  The field is still planned on the published map: a closed door stalls the robot in front of it until the
        map catches up.  ``None`` is the call above, unchanged."""
        if getattr(self, "_plan_goals", None) is None:
            raise capi.TsdError("explore_drive: no plan (explore_plan first)")
        if live_points is not None:
            pts = _live_points(live_points)
            kept, blocked = C.c_int(0), C.c_int(0)

            def call(pose_p, limits, ints, foot, n_foot, out, choice, shape, dt):
                return self.lib.tsd_node_explore_drive_live(self.h, int(goal), pose_p, limits, ints, foot, n_foot,
                                                            pts.ctypes.data_as(_dp) if pts.shape[0] else None, int(pts.shape[0]),
                                                            float(live_radius_m), float(live_skip_m), out, choice, shape, dt, C.byref(kept),
                                                            C.byref(blocked))

            out = _drive(call, [pose], v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin,
                         "tsd_node_explore_drive_live")[0]
            out.update(live_kept=kept.value, blocked_live=blocked.value)
            return out
        return _drive(lambda *a: self.lib.tsd_node_explore_drive(self.h, int(goal), *a), [pose], v_max, w_max, horizon_s, footprint, n_speeds,
                      weights, nose_m, nose_miss, margin, "tsd_node_explore_drive")[0]

    def explore_gains(self, view_radius_m: float, unknown_depth=0) -> np.ndarray:
        """What each goal of the plan made last is worth: the capi.VIEW_GAIN_DTYPE records (cell, gain, unknown, visible), one per
        goal and in the goals' order, of a scanner standing on the goal and seeing ``view_radius_m`` far all around on the map the
        plan was made on -- the radius rounded to cells, at most capi.VIEW_MAX_RADIUS; ``unknown_depth`` > 0 ends a ray behind that
        many unknown cells.  Zeros for a goal without a cell.  Refused without a plan and once the map has been published again."""
        n = getattr(self, "_plan_goals", None)
        if n is None:
            raise capi.TsdError("explore_gains: no plan (explore_plan first)")
        out = np.zeros(n, dtype=capi.VIEW_GAIN_DTYPE)
        radius = C.c_int(0)
        rc = self.lib.tsd_node_explore_gains(self.h, float(view_radius_m), int(unknown_depth), out.ctypes.data, C.byref(radius))
        if rc != 0:
            raise capi.TsdError(f"tsd_node_explore_gains failed ({rc})")
        self.view_radius_cells = radius.value
        return out

    def surface_msg(self) -> dict:
        """the last sensor_msgs/PointCloud2 on <node>/surface (parameter publish_surface_cloud): ``points`` as (width, 6) float32 in
        the order of ``fields`` (x y z normal_x normal_y normal_z) and the number published (0: no message, the parameter is off)"""
        info = np.zeros(4)
        text = C.create_string_buffer(512)
        self.lib.tsd_node_surface(self.h, None, info.ctypes.data_as(_dp), text, 512)
        w, step = int(info[0]), int(info[1])
        data = np.zeros(max(w * step, 1), dtype=np.uint8)
        n = self.lib.tsd_node_surface(self.h, data.ctypes.data, info.ctypes.data_as(_dp), text, 512)
        frame, fields = text.value.decode().split("|")
        fields = [f for f in fields.split(",") if f]
        pts = data[:w * step].view(np.float32).reshape(w, step // 4) if w and step else np.zeros((0, len(fields)), dtype=np.float32)
        return {"width": w, "height": 1 if n else 0, "point_step": step, "stamp_ns": int(info[2]), "frame_id": frame, "fields": fields,
                "points": pts, "count": int(n)}

    def map_image_msg(self) -> dict:
        """the last sensor_msgs/Image on <node>/map/image (data as (height, width, 3) uint8) and its publish count"""
        info = np.zeros(5)
        text = C.create_string_buffer(256)
        self.lib.tsd_node_map_image_msg(self.h, None, info.ctypes.data_as(_dp), text, 256)
        h, w, step = int(info[0]), int(info[1]), int(info[2])
        data = np.zeros(step * h, dtype=np.uint8)
        n = self.lib.tsd_node_map_image_msg(self.h, data.ctypes.data, info.ctypes.data_as(_dp), text, 256)
        enc, frame = text.value.decode().split("|")
        return {"height": h, "width": w, "step": step, "is_bigendian": int(info[3]), "stamp_ns": int(info[4]),
                "encoding": enc, "frame_id": frame, "data": data.reshape(h, w, 3) if h and w else data, "count": int(n)}

    def grid(self) -> "GridView":
        return GridView(self.lib.tsd_node_grid_ctx(self.h), self)


FRONTIER_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("size", "<u4"), ("min_x", "<i4"), ("min_y", "<i4"),
                           ("max_x", "<i4"), ("max_y", "<i4")])


def _frontier_dict(call, fetch, what):
    count, used, n_seeds = C.c_int(0), C.c_int(0), C.c_int(0)
    seeds = np.zeros(2 * capi.FRONTIER_MAX_SEEDS, dtype=np.int32)
    origin_cs = np.zeros(3)
    rc = call(C.byref(count), C.byref(used), seeds.ctypes.data, C.byref(n_seeds), origin_cs.ctypes.data_as(_dp))
    if rc != 0:
        raise capi.TsdError(f"{what} failed ({rc}): no map published yet?")
    rec = np.zeros(count.value, dtype=capi.FRONTIER_DTYPE)
    if count.value:
        fetch(rec.ctypes.data)
    size = rec["size"].astype(np.float64)
    cen = np.stack([(rec["sum_x"].astype(np.float64) / size + 0.5) * origin_cs[2] + origin_cs[0],
                    (rec["sum_y"].astype(np.float64) / size + 0.5) * origin_cs[2] + origin_cs[1]], axis=1)
    return {"records": rec, "centroids": cen, "seeds": [tuple(int(v) for v in seeds[2 * k:2 * k + 2]) for k in range(n_seeds.value)],
            "seeds_used": used.value, "origin": origin_cs[:2].copy(), "resolution": float(origin_cs[2])}


def _plan_dict(call, fetch, width, max_len, what):
    counts = (C.c_int * 3)()
    info, n_seeds = capi.RouteInfo(), C.c_int(0)
    seeds = np.zeros(2 * capi.FRONTIER_MAX_SEEDS, dtype=np.int32)
    origin_cs = np.zeros(3)
    rc = call(counts, C.byref(info), seeds.ctypes.data, C.byref(n_seeds), origin_cs.ctypes.data_as(_dp))
    if rc != 0:
        raise capi.TsdError(f"{what} failed ({rc}): no map (or, for the cost map, no cost map) published yet?")
    n, n_cells = counts[0], counts[1]
    rec = np.zeros(n, dtype=capi.FRONTIER_DTYPE)
    goals = np.zeros(n, dtype=capi.ROUTE_GOAL_DTYPE)
    lens = np.zeros(n, dtype=np.int32)
    cells = np.zeros(max(n_cells, 1), dtype=np.uint32)
    if n:
        fetch(rec.ctypes.data, goals.ctypes.data, lens.ctypes.data, cells.ctypes.data)
    res, origin = float(origin_cs[2]), origin_cs[:2].copy()

    def metres(c):
        c = np.asarray(c, dtype=np.int64)
        return np.stack([((c % width) + 0.5) * res + origin[0], ((c // width) + 0.5) * res + origin[1]], axis=-1)

    size = rec["size"].astype(np.float64)
    cen = np.stack([(rec["sum_x"].astype(np.float64) / size + 0.5) * res + origin[0],
                    (rec["sum_y"].astype(np.float64) / size + 0.5) * res + origin[1]], axis=1)
    goal_xy = metres(goals["cell"]).reshape(n, 2)
    goal_xy[goals["cell"] == capi.ROUTE_NONE] = np.nan
    # the paths lie one after the other, min(len, max_len) cells each, goal first
    paths, at = [], 0
    stored = np.minimum(np.maximum(lens, 0), int(max_len))
    assert int(stored.sum()) == n_cells
    for k in range(n):
        paths.append(metres(cells[at:at + stored[k]][::-1]).reshape(-1, 2))
        at += int(stored[k])
    return {"records": rec, "centroids": cen, "goals": goals, "goal_xy": goal_xy, "paths": paths, "path_lens": lens,
            "route": info.as_dict(), "seeds": [tuple(int(v) for v in seeds[2 * k:2 * k + 2]) for k in range(n_seeds.value)],
            "seeds_used": counts[2], "origin": origin, "resolution": res}


def scan_points(pose, ranges, angle_min: float, angle_increment: float, max_range: float) -> np.ndarray:
    """The end points of a scan taken at ``pose`` = (x, y [m], yaw [rad]) in the map's frame, float64 (N, 2): beam i ends at
    pose + ranges[i] * (cos, sin)(yaw + angle_min + i * angle_increment).  Readings that are not finite or beyond ``max_range`` are dropped -- they
    ended on nothing.  What ``explore_drive`` takes as ``live_points``."""
    r = np.asarray(ranges, dtype=np.float64).ravel()
    a = float(pose[2]) + float(angle_min) + float(angle_increment) * np.arange(r.size, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(r) & (r <= float(max_range))
    return np.stack([float(pose[0]) + r[ok] * np.cos(a[ok]), float(pose[1]) + r[ok] * np.sin(a[ok])], axis=1)


def _live_points(points) -> np.ndarray:
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    if pts.shape[0] > capi.DRIVE_LIVE_MAX_POINTS:
        raise capi.TsdError(f"explore_drive: {pts.shape[0]} live points, at most {capi.DRIVE_LIVE_MAX_POINTS}")
    return pts


def _drive(call, poses, v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin, what):
    """one explore_drive call for len(poses) robots: per robot a dict, the call's shape and dt shared by all"""
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
    n = poses.shape[0]
    limits = np.array([v_max, w_max, horizon_s, nose_m], dtype=np.float64)
    ints = (C.c_int * 7)(int(n_speeds), *[int(w) for w in weights], int(nose_miss), int(margin))
    foot = np.zeros((0, 2)) if footprint is None else np.ascontiguousarray(np.asarray(footprint, dtype=np.float64).reshape(-1, 2))
    out = np.zeros((n, 8))
    choice = np.zeros(n, dtype=capi.DRIVE_CHOICE_DTYPE)
    shape, dt = (C.c_int * 4)(), C.c_double(0.0)
    rc = call(poses.ctypes.data_as(_dp), limits.ctypes.data_as(_dp), ints, foot.ctypes.data_as(_dp) if foot.shape[0] else None,
              int(foot.shape[0]), out.ctypes.data_as(_dp), choice.ctypes.data, shape, C.byref(dt))
    if rc != 0:
        raise capi.TsdError(f"{what} failed ({rc}): no plan or dispatch of the map published last, a pose outside the map, limits that are "
                            "not positive, or a turn list beyond 129 entries (w_max * cell_size / v_max too large)?")
    return [{"v": float(out[r, 0]), "w": float(out[r, 1]), "end_xy": out[r, 2:4].copy(), "admissible": int(out[r, 4]),
             "next_pose": out[r, 5:8].copy(), "choice": choice[r], "steps": shape[0], "n_speeds": shape[1], "n_turns": shape[2],
             "n_body": shape[3], "dt": dt.value} for r in range(n)]


def _waypoint_dict(call, n, frame, lookahead_m, slack, max_way, what):
    width, max_len, origin, res = frame
    max_way = int(max_way)
    way = np.zeros((n, max(max_way, 1)), dtype=np.uint32)
    info = np.zeros(n, dtype=capi.WAYPOINT_INFO_DTYPE)
    cells = C.c_int(0)
    rc = call(float(lookahead_m), int(slack), max_len, max_way, way.ctypes.data, info.ctypes.data, C.byref(cells))
    if rc != 0:
        raise capi.TsdError(f"{what} failed ({rc}): no plan of the map published last, or max_way < 1?")
    out = []
    for k in range(n):
        c = way[k, :min(max(int(info["n_way"][k]), 0), max_way)].astype(np.int64)
        out.append(np.stack([((c % width) + 0.5) * res + origin[0], ((c // width) + 0.5) * res + origin[1]], axis=-1).reshape(-1, 2))
    return {"waypoints": out, "info": info, "lookahead_cells": cells.value}


class SlamFleet:
    """Several :class:`SlamNode` s on ONE GPU, each with its own grid, and their merged map (``ThreadGridGroup``): every node's
    ``x_offset`` / ``y_offset`` places its grid, offsets that do not differ by whole cells are refused.  The first node publishes
    ``<node>/merged_map`` and answers ``<node>/get_merged_map``.  Maps turned against each other, or a fraction of a cell apart, are
    merged after ``set_transforms`` (with what ``align`` found).  Close the fleet before its nodes."""

    def __init__(self, nodes):
        self.lib = load_library()
        self.nodes = list(nodes)
        hs = (C.c_void_p * max(len(self.nodes), 1))(*[n.h for n in self.nodes])
        err = C.create_string_buffer(512)
        self.h = self.lib.tsd_fleet_create(len(self.nodes), hs, err, 512)
        if not self.h:
            raise capi.TsdError(f"tsd_fleet_create refused: {err.value.decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def publish_merged_map(self) -> dict:
        """one merge and publication now, on the caller's thread; the published message (as ``merged_map_msg``)"""
        rc = self.lib.tsd_fleet_publish_merged(self.h)
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_publish_merged failed ({rc})")
        return self.merged_map_msg()

    def frontiers(self, min_size=1) -> dict:
        """The frontiers of the merged map published last with one seed per node -- the cell of that node's current pose in the
        merged map, carried there by the group's placement -- as ``SlamNode.frontiers`` returns them: what an exploration allocator
        for the fleet consumes."""
        return _frontier_dict(lambda c, u, so, no, oc: self.lib.tsd_fleet_frontiers(self.h, int(min_size), c, u, so, no, oc),
                              lambda out: self.lib.tsd_fleet_frontiers_fetch(self.h, out), "tsd_fleet_frontiers")

    def explore_plan(self, min_size=1, max_len=4096) -> dict:
        """``SlamNode.explore_plan`` on the merged map published last with one seed per node (``frontiers()``'s seeds), unit weights
        on the free cells: ``goals["seed"]`` is the node nearest to each frontier -- the assignment an exploration allocator starts
        from -- and each path starts at that node's cell."""
        self._plan_goals = None
        width = self.merged_map_msg()["width"]
        out = _plan_dict(lambda c, i, so, no, oc: self.lib.tsd_fleet_explore_plan(self.h, int(min_size), int(max_len), c, i, so, no, oc),
                         lambda *out: self.lib.tsd_fleet_explore_plan_fetch(self.h, *out), width, max_len, "tsd_fleet_explore_plan")
        self._plan_goals = len(out["goals"])
        self._plan_frame = (width, int(max_len), out["origin"], out["resolution"])
        return out

    def explore_waypoints(self, lookahead_m: float, slack=0, max_way=256) -> dict:
        """``SlamNode.explore_waypoints`` for the merged map's plan made last: every goal's path, from the node nearest to it,
        straightened into waypoints.  Refused without a plan and once the merged map has been published again."""
        if getattr(self, "_plan_goals", None) is None:
            raise capi.TsdError("explore_waypoints: no plan (explore_plan first)")
        return _waypoint_dict(lambda *a: self.lib.tsd_fleet_explore_waypoints(self.h, *a), self._plan_goals, self._plan_frame, lookahead_m,
                              slack, max_way, "tsd_fleet_explore_waypoints")

    def explore_assign(self, view_radius_m: float, gain_weight: int, unknown_depth=0) -> dict:
        """Which node drives where, on the merged map's plan made last (tsd_view_assign): ``goal_of_robot`` int32 per node -- an index
        into the plan's goals, -1 for a node that gets none --, ``picked`` (capi.VIEW_GAIN_DTYPE per node: the goal's record as its
        round saw it), ``rounds`` and ``radius_cells``.  A goal scores gain * ``gain_weight`` - dist; the best goal goes to the node
        it is nearest to, what that node will see is claimed, and the rest is scored again.  A node is only ever offered the goals it
        is nearest to.  Refused without a plan and once the merged map has been published again."""
        n = len(self.nodes)
        goal_of = np.full(n, -1, dtype=np.int32)
        picked = np.zeros(n, dtype=capi.VIEW_GAIN_DTYPE)
        rounds, radius = C.c_int(0), C.c_int(0)
        rc = self.lib.tsd_fleet_explore_assign(self.h, float(view_radius_m), int(gain_weight), int(unknown_depth), goal_of.ctypes.data,
                                               picked.ctypes.data, C.byref(rounds), C.byref(radius))
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_explore_assign failed ({rc})")
        return {"goal_of_robot": goal_of, "picked": picked, "rounds": rounds.value, "radius_cells": radius.value}

    def explore_dispatch(self, view_radius_m: float, gain_weight: int, lookahead_m: float, slack=0, unknown_depth=0, min_size=1,
                         max_len=4096, max_way=256) -> dict:
        """Every node's next goal and the way to it in one call on the merged map published last, with one seed per node
        (``frontiers()``'s seeds) and a cost-to-go field PER NODE: ``frontiers`` (as ``frontiers()`` returns them), ``goals`` (the
        matrix, capi.ROUTE_GOAL_DTYPE of shape (nodes, frontiers): node r's cheapest cell of frontier f), ``goal_of_robot`` (a
        frontier index per node, -1 for a node that gets none), ``goal`` (capi.ROUTE_GOAL_DTYPE per node: its row's entry of that
        frontier, cell ROUTE_NONE for -1), ``picked`` (capi.VIEW_GAIN_DTYPE per node), ``rounds``, ``waypoints`` (per node an (n, 2)
        array in metres, the node's own cell first and the goal last; empty for -1), ``waypoint_cells`` and ``waypoint_info``
        (capi.WAYPOINT_INFO_DTYPE per node), ``fields`` (tsd_route_fields_info as a dict), ``radius_cells``, ``lookahead_cells``,
        ``origin`` and ``resolution``.  The pair of node and frontier with the best gain * ``gain_weight`` - dist wins, node and
        frontier leave, what the node will see is claimed; unlike ``explore_assign`` a node may be given a frontier another node is
        nearer to.  Refused before the first merged map."""
        n = len(self.nodes)
        counts = (C.c_int * 6)()
        info = capi.RouteFieldsInfo()
        seeds = np.zeros(2 * capi.FRONTIER_MAX_SEEDS, dtype=np.int32)
        origin_cs = np.zeros(3)
        max_len, max_way = int(max_len), int(max_way)
        rc = self.lib.tsd_fleet_explore_dispatch(self.h, int(min_size), float(view_radius_m), int(gain_weight), int(unknown_depth),
                                                 float(lookahead_m), int(slack), max_len, max_way, counts, C.byref(info), seeds.ctypes.data,
                                                 origin_cs.ctypes.data_as(_dp))
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_explore_dispatch failed ({rc}): no merged map published yet, or max_len / max_way < 1?")
        nf = counts[0]
        rec = np.zeros(nf, dtype=capi.FRONTIER_DTYPE)
        goals = np.zeros((n, nf), dtype=capi.ROUTE_GOAL_DTYPE)
        goal_of = np.full(n, -1, dtype=np.int32)
        picked = np.zeros(n, dtype=capi.VIEW_GAIN_DTYPE)
        way = np.zeros((n, max_way), dtype=np.uint32)
        winfo = np.zeros(n, dtype=capi.WAYPOINT_INFO_DTYPE)
        rc = self.lib.tsd_fleet_explore_dispatch_fetch(self.h, rec.ctypes.data, goals.ctypes.data, goal_of.ctypes.data, picked.ctypes.data,
                                                       way.ctypes.data, winfo.ctypes.data)
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_explore_dispatch_fetch failed ({rc}): the merged map has been published again")
        res, origin = float(origin_cs[2]), origin_cs[:2].copy()
        width = self.merged_map_msg()["width"]
        size = rec["size"].astype(np.float64)
        cen = np.stack([(rec["sum_x"].astype(np.float64) / size + 0.5) * res + origin[0],
                        (rec["sum_y"].astype(np.float64) / size + 0.5) * res + origin[1]], axis=1)
        frontiers = {"records": rec, "centroids": cen, "seeds": [tuple(int(v) for v in seeds[2 * k:2 * k + 2]) for k in range(n)],
                     "seeds_used": counts[5], "origin": origin, "resolution": res}
        goal = np.zeros(n, dtype=capi.ROUTE_GOAL_DTYPE)
        goal["cell"], goal["dist"], goal["seed"] = capi.ROUTE_NONE, capi.ROUTE_NONE, -1
        cells, metres = [], []
        for r in range(n):
            if goal_of[r] >= 0:
                goal[r] = goals[r, goal_of[r]]
            c = way[r, :min(max(int(winfo["n_way"][r]), 0), max_way)].astype(np.int64)
            cells.append(c.astype(np.uint32))
            metres.append(np.stack([((c % width) + 0.5) * res + origin[0], ((c // width) + 0.5) * res + origin[1]], axis=-1).reshape(-1, 2))
        return {"frontiers": frontiers, "goals": goals, "goal_of_robot": goal_of, "goal": goal, "picked": picked, "rounds": counts[2],
                "waypoints": metres, "waypoint_cells": cells, "waypoint_info": winfo, "fields": info.as_dict(), "radius_cells": counts[3],
                "lookahead_cells": counts[4], "origin": origin, "resolution": res}

    def explore_drive(self, poses, v_max: float, w_max: float, horizon_s: float, footprint=None, n_speeds=5, weights=(1, 1, 0, 0),
                      nose_m=0.0, nose_miss=0, margin=2000, separation_m=0.0, priority=None, live_points=None, live_radius_m=0.0,
                      live_skip_m=0.0) -> list:
        """``SlamNode.explore_drive`` for every node at once, towards the goal the last ``explore_dispatch`` gave it: ``poses`` one
        (x, y [m], yaw [rad]) per node in the merged map's frame; one fields call on the merged map seeded at the nodes' goal cells
        (unit weights, as the dispatch plans), then one tsd_drive_fields_rollout, node r on layer r.  A list of one dict per node; a
        node without a goal gets ``v`` = ``w`` = 0 and ``admissible`` == 0.  The goal-seeded layers replace the dispatch's fields
        result on the device.  Refused without a dispatch and once the merged map has been published again.

        ``separation_m`` > 0 keeps the nodes off each other (tsd_drive_fleet_rollout): they decide one after the other, and an arc
        that comes within ``separation_m`` (centre to centre) of an arc chosen before it, at the same time step and without moving
        away from it, is refused; a node without a goal is a parked robot the others keep clear of.  ``priority``: the nodes'
        indices, the first decides first.  By default the nodes with a goal go in ascending cost-to-go at their pose -- the one
        nearer its goal first --, ties by index, the others behind them.  Each dict then also holds ``blocked`` (the samples the node
        lost to the others), ``tracks`` (the chosen arc, ``steps`` + 1 points (x, y) [m]; the pose itself without one) and ``rank``
        (its place in the order used).  With 0.0 the call is the one above, unchanged.

        ``live_points``, ``live_radius_m``, ``live_skip_m``: as for ``SlamNode.explore_drive`` -- the end points of all nodes' current
        scans in the merged map's frame as ONE layer for all nodes, with the points within ``live_skip_m`` of ANY node's pose dropped
        (one node's scanner sees the other's body).  Every dict then also holds ``live_kept`` and the node's ``blocked_live``.
        ``None`` is the call above, unchanged."""
        if len(poses) != len(self.nodes):
            raise capi.TsdError("explore_drive: one pose per node")
        if not separation_m > 0.0 and (separation_m != 0.0 or priority is not None):
            raise capi.TsdError("explore_drive: separation_m must be 0 or positive, and a priority needs a separation")
        if live_points is not None:
            return self._explore_drive_live(poses, v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin,
                                            float(separation_m), priority, _live_points(live_points), float(live_radius_m), float(live_skip_m))
        if not separation_m > 0.0:
            return _drive(lambda *a: self.lib.tsd_fleet_explore_drive(self.h, *a), poses, v_max, w_max, horizon_s, footprint, n_speeds, weights,
                          nose_m, nose_miss, margin, "tsd_fleet_explore_drive")
        n = len(self.nodes)
        prio = np.zeros(0, dtype=np.int32) if priority is None else np.ascontiguousarray(priority, dtype=np.int32).ravel()
        order, blocked = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        tracks = np.zeros((n * (capi.DRIVE_MAX_STEPS + 1), 2))

        def call(poses_p, limits, ints, foot, n_foot, out, choice, shape, dt):
            return self.lib.tsd_fleet_explore_drive_apart(self.h, poses_p, limits, ints, foot, n_foot, float(separation_m),
                                                          prio.ctypes.data if prio.size else None, int(prio.size), out, choice, shape, dt,
                                                          order.ctypes.data, blocked.ctypes.data, tracks.ctypes.data_as(_dp), int(tracks.size))

        out = _drive(call, poses, v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin, "tsd_fleet_explore_drive_apart")
        t1 = out[0]["steps"] + 1
        for r in range(n):
            out[r].update(blocked=int(blocked[r]), tracks=tracks[r * t1:(r + 1) * t1].copy(), rank=int(np.nonzero(order == r)[0][0]))
        return out

    def _explore_drive_live(self, poses, v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin, separation_m, priority,
                            pts, radius_m, skip_m):
        """explore_drive with live points (tsd_fleet_explore_drive_live), with or without a separation"""
        n = len(self.nodes)
        prio = np.zeros(0, dtype=np.int32) if priority is None else np.ascontiguousarray(priority, dtype=np.int32).ravel()
        order, blocked, blocked_live = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        tracks = np.zeros((n * (capi.DRIVE_MAX_STEPS + 1), 2))
        kept = C.c_int(0)

        def call(poses_p, limits, ints, foot, n_foot, out, choice, shape, dt):
            return self.lib.tsd_fleet_explore_drive_live(self.h, poses_p, limits, ints, foot, n_foot, separation_m,
                                                         prio.ctypes.data if prio.size else None, int(prio.size),
                                                         pts.ctypes.data_as(_dp) if pts.shape[0] else None, int(pts.shape[0]), radius_m, skip_m,
                                                         out, choice, shape, dt, order.ctypes.data, blocked.ctypes.data,
                                                         tracks.ctypes.data_as(_dp), int(tracks.size), C.byref(kept), blocked_live.ctypes.data)

        out = _drive(call, poses, v_max, w_max, horizon_s, footprint, n_speeds, weights, nose_m, nose_miss, margin, "tsd_fleet_explore_drive_live")
        t1 = out[0]["steps"] + 1
        for r in range(n):
            out[r].update(live_kept=kept.value, blocked_live=int(blocked_live[r]))
            if separation_m > 0.0:
                out[r].update(blocked=int(blocked[r]), tracks=tracks[r * t1:(r + 1) * t1].copy(), rank=int(np.nonzero(order == r)[0][0]))
        return out

    def merged_frames(self) -> int:
        return int(self.lib.tsd_fleet_merged_frames(self.h))

    def merged_map_msg(self) -> dict:
        """the last nav_msgs/OccupancyGrid on <node>/merged_map (data as (height, width) int8) and its publish count"""
        n, m = SlamNode._map_dict(lambda d, i, f, c: self.lib.tsd_fleet_merged_map_msg(self.h, d, i, f, c))
        m["count"] = int(n)
        return m

    def get_merged_map(self) -> dict:
        ok, m = SlamNode._map_dict(lambda d, i, f, c: self.lib.tsd_fleet_get_merged_map(self.h, d, i, f, c))
        if not ok:
            raise capi.TsdError("get_merged_map refused")
        return m

    def fuse_tsd(self) -> "GridView":
        """TSD-level fusion of the nodes' grids (``ThreadGridGroup::fuse``) into a grid the fleet owns -- as large as node 0's,
        placed where node 0's lies, every other grid shifted by the whole-cell distance of its map origin.  The view is an
        ordinary grid (ray cast, localise, push, store, colour image) and stays valid until the fleet is closed; every call
        fuses anew."""
        rc = C.c_int(0)
        ctx = self.lib.tsd_fleet_fuse_tsd(self.h, C.byref(rc))
        if not ctx:
            raise capi.TsdError(f"tsd_fleet_fuse_tsd failed ({rc.value})")
        return GridView(ctx, _FusedLock(self))

    def align(self, i, j, **lattice) -> dict:
        """The pose of node j's map in node i's (``TsdGridDevice.align_to``: tsd_map_align(grid i, grid j)): ``T`` carries node j's
        map coordinates into node i's, ``cell_off`` is the whole-cell shift ``fuse`` and the merge group would take for the pair.
        Holds both nodes' grid locks, taken in ascending node index, for the whole call.  ``lattice``: align_to's arguments."""
        if i == j:
            raise capi.TsdError("SlamFleet.align: a node's map against itself")
        held = []
        try:
            for k in sorted((i, j)):
                node = self.nodes[k]
                node.lib.tsd_node_grid_lock(node.h)
                held.append(node)
            # (through the class, on views without a lock of their own: both locks are held here)
            dst = GridView(self.nodes[i].lib.tsd_node_grid_ctx(self.nodes[i].h), None)
            src = GridView(self.nodes[j].lib.tsd_node_grid_ctx(self.nodes[j].h), None)
            return capi.TsdGridDevice.align_to(dst, src, **lattice)
        finally:
            for node in reversed(held):
                node.lib.tsd_node_grid_unlock(node.h)

    def set_transforms(self, Ts):
        """Places the nodes' maps by rigid transforms (``ThreadGridGroup::setTransforms``): ``Ts[i]`` (3x3) carries node i's grid
        coordinates into node 0's, ``Ts[0]`` is the identity --
        ``[np.eye(3)] + [fleet.align(0, j, ...)["T"] for j in range(1, n)]``.  The merged map published from then on is the
        occupancy-level merge under those transforms (rotations and fractions of a cell included); ``fuse_tsd`` raises unless every
        transform is a whole-cell shift."""
        Ts = list(Ts)
        if len(Ts) != len(self.nodes):
            raise capi.TsdError(f"SlamFleet.set_transforms: {len(Ts)} transforms for {len(self.nodes)} nodes")
        flat = np.ascontiguousarray([np.asarray(T, dtype=np.float64).reshape(9) for T in Ts], dtype=np.float64).reshape(-1)
        err = C.create_string_buffer(512)
        rc = self.lib.tsd_fleet_set_transforms(self.h, flat.ctypes.data_as(_dp), err, 512)
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_set_transforms refused ({rc}): {err.value.decode()}")

    def fused_image_msg(self) -> dict:
        """the colour image of the fused grid (after ``fuse_tsd``) as a sensor_msgs/Image: ``map_image_msg``'s fields"""
        info = np.zeros(5)
        text = C.create_string_buffer(256)
        rc = self.lib.tsd_fleet_fused_image_msg(self.h, None, info.ctypes.data_as(_dp), text, 256)
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_fused_image_msg failed ({rc}): no fused grid yet?")
        h, w, step = int(info[0]), int(info[1]), int(info[2])
        data = np.zeros(step * h, dtype=np.uint8)
        rc = self.lib.tsd_fleet_fused_image_msg(self.h, data.ctypes.data, info.ctypes.data_as(_dp), text, 256)
        if rc != 0:
            raise capi.TsdError(f"tsd_fleet_fused_image_msg failed ({rc})")
        enc, frame = text.value.decode().split("|")
        return {"height": h, "width": w, "step": step, "is_bigendian": int(info[3]), "stamp_ns": int(info[4]),
                "encoding": enc, "frame_id": frame, "data": data.reshape(h, w, 3)}


class _FusedLock:
    """what GridView asks of a node, for the fleet's fused grid: its mutex"""

    def __init__(self, fleet):
        self.h = fleet.h
        self.lib = _FusedLib(fleet.lib)


class _FusedLib:
    def __init__(self, lib):
        self.tsd_node_grid_lock = lib.tsd_fleet_fused_lock
        self.tsd_node_grid_unlock = lib.tsd_fleet_fused_unlock


class GridView(capi.TsdGridDevice):
    """Non-owning view of the facade's grid context (for dumps / profiling through the tsd_* ABI).  Every device call
    made through it takes the facade's grid mutex (obvious::TsdGrid::mutex()), like the facade's own classes do: the
    node's localise / mapping threads may be enqueueing on the same context."""

    _LOCKED = ("reset", "sync", "free_footprint", "push", "raycast", "icp", "localize", "icp_trace", "download_tile_state",
               "download_tiles", "upload_tiles", "digest", "occupancy", "occupancy_into", "calibrate_rmw", "profile", "store_text",
               "load_text", "color_image", "push_stats_total", "profile_reset", "profile_get", "profile_spread", "profile_samples", "tsdpdf_match",
               "relocalize", "debug_reloc_scores", "debug_reloc_peaks", "surface_extract", "surface_fetch", "surface_points",
               "surface_dev", "align_points", "debug_align_scores", "debug_align_peaks", "debug_align_sums",
               "clearance_of", "costmap_begin", "frontiers_of", "frontiers", "route_of", "route", "route_goals", "route_paths",
               "route_fields_of", "route_fields", "route_fields_goals", "route_fields_paths", "route_fields_waypoints")

    def __init__(self, ctx, node=None):  # noqa: D401 - does not call the base constructor on purpose
        self.lib = capi.load_library()
        self.h = ctx
        self._node = node
        self.cells = self.lib.tsd_cells(ctx)
        self.tiles = self.lib.tsd_tiles(ctx)
        self.cell_size = self.lib.tsd_cell_size(ctx)
        self.max_trunc = self.lib.tsd_max_truncation(ctx)
        self.min_x, self.max_x = self.lib.tsd_min_x(ctx), self.lib.tsd_max_x(ctx)
        self.min_y, self.max_y = self.lib.tsd_min_y(ctx), self.lib.tsd_max_y(ctx)

    # these also use the context's frontier scratch, which the node's ThreadGrid (and a fleet's group) use: the grid's frontierMutex
    # is taken first and held until the records and labels are fetched
    _FRONTIER = ("frontiers_of", "frontiers", "route_of", "route", "route_goals", "route_paths",      # (the goals read the frontier result)
                 "route_fields_of", "route_fields", "route_fields_goals", "route_fields_paths", "route_fields_waypoints")

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name in GridView._LOCKED and callable(attr):
            node = object.__getattribute__(self, "_node")
            if node is not None and getattr(node, "h", None):
                scratch = name in GridView._FRONTIER and hasattr(node.lib, "tsd_node_frontier_lock")

                def locked(*a, **k):
                    if scratch:
                        node.lib.tsd_node_frontier_lock(node.h)
                    node.lib.tsd_node_grid_lock(node.h)
                    try:
                        return attr(*a, **k)
                    finally:
                        node.lib.tsd_node_grid_unlock(node.h)
                        if scratch:
                            node.lib.tsd_node_frontier_unlock(node.h)
                return locked
        return attr

    def close(self):
        self.h = None


def node_params(gc, geo=None, **over) -> dict:
    """Parameter set of the measurement plan: single-laser.yaml values with
    registration_mode 0 and the benchmark's grid size."""
    p = {
        "robot_nbr": 1, "map_size": gc.map_size_log2, "cellsize": float(gc.cell_size),
        "truncation_radius": gc.truncation_radius, "x_offset": 0.0, "y_offset": 0.0,
        "dist_filter_max": 0.4, "dist_filter_min": 0.02, "icp_iterations": 30,
        "reg_trs_max": 1.0, "reg_sin_rot_max": 0.5, "laser_min_range": 0.26, "registration_mode": 0,
        "tsd_slam/local_offset_x": 0.37, "tsd_slam/local_offset_y": -0.21, "tsd_slam/local_offset_yaw": 0.1,
    }
    p.update(over)
    return p
