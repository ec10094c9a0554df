"""ctypes binding of the C ABI in ``include/tsd_hip.h`` (``lib/libtsd_hip.so``).

This is plumbing for the Python test / bench drivers; the product is the HIP library itself and the
C++ facade in ``csrc/host``.  There is no CPU fall-back: importing works without a GPU (so the ABI can
be checked), but every compute call needs a gfx950 device and raises :class:`TsdError` otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TSD_LIB_DIR: developer override used by tools/*_stamps*.sh, which build INSTRUMENTED variants of the kernels into
# lib/diag/ so that the product libraries under lib/ are never replaced by a build without parity checks
LIB_DIR = os.environ.get("TSD_LIB_DIR") or os.path.join(_HERE, "lib")
if os.environ.get("TSD_LIB_DIR"):
    import sys as _sys
    print(f"ohm_tsd_slam_amd: using the libraries under TSD_LIB_DIR={LIB_DIR} (diagnostic build)", file=_sys.stderr)
LIB_PATH = os.path.join(LIB_DIR, "libtsd_hip.so")
# the same library built with 32-bit fixed-point cell storage (-DTSD_STORAGE_Q32, csrc/tsd_device.hpp)
LIB_PATH_Q32 = os.path.join(LIB_DIR, "libtsd_hip_q32.so")

TILE_CELLS = 1089
MAX_BEAMS = 4096
MAX_ICP_POINTS = 2048

ICP_STATE = {1: "PROCESSING", 2: "NOTMATCHABLE", 3: "MAXITERATIONS", 5: "SUCCESS"}


class TsdError(RuntimeError):
    pass


class PushStats(C.Structure):
    _fields_ = [
        ("cells_updated", C.c_int64),
        ("cells_visited", C.c_int64),
        ("tiles_total", C.c_int32),
        ("tiles_range_pass", C.c_int32),
        ("tiles_update", C.c_int32),
        ("tiles_new", C.c_int32),
        ("tiles_new_from_empty", C.c_int32),
        ("tiles_emptied_init", C.c_int32),
        ("tiles_emptied_uninit", C.c_int32),
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class IcpParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("estimator", C.c_int),          # 0 ClosedFormEstimator2D (the node's), 1 PointToLine2DEstimator
        ("dist_filter_max", C.c_double),
        ("dist_filter_min", C.c_double),
        ("min_x", C.c_double),
        ("max_x", C.c_double),
        ("min_y", C.c_double),
        ("max_y", C.c_double),
        ("t_init", C.c_double * 9),      # Tinit of Icp::iterate (pre-registration result), used when use_t_init != 0
        ("use_t_init", C.c_int),
        ("reserved", C.c_int),
    ]


class TsdPdfParams(C.Structure):
    """tsd_tsdpdf_params"""
    _fields_ = [("trials", C.c_int), ("size_control_set", C.c_int), ("eps_thresh", C.c_double), ("zrand", C.c_double),
                ("phi_max", C.c_double), ("ang_res", C.c_double)]


class TsdPdfResult(C.Structure):
    """tsd_tsdpdf_result"""
    _fields_ = [("T", C.c_double * 9), ("probability", C.c_double), ("idx_model", C.c_int32), ("idx_scene", C.c_int32),
                ("candidates", C.c_int32), ("valid_model", C.c_int32), ("valid_scene", C.c_int32), ("control_points", C.c_int32),
                ("reserved", C.c_int32)]


class PdfMatchParams(C.Structure):
    """tsd_pdfmatch_params"""
    _fields_ = [("trials", C.c_int), ("size_control_set", C.c_int), ("eps_thresh", C.c_double), ("zhit", C.c_double),
                ("zphi", C.c_double), ("zshort", C.c_double), ("zmax", C.c_double), ("zrand", C.c_double),
                ("percentage_points_in_c", C.c_double), ("rangemax", C.c_double), ("sigphi", C.c_double), ("sighit", C.c_double),
                ("lamshort", C.c_double), ("max_angle_diff", C.c_double), ("max_angle_penalty", C.c_double), ("phi_max", C.c_double),
                ("ang_res", C.c_double)]


# the node's defaults for registration_mode 2 (ThreadLocalize.cpp:105-128): PdfMatchParams fields -> value
PDFMATCH_DEFAULTS = dict(trials=100, size_control_set=140, eps_thresh=0.15, zhit=0.45, zphi=0.0, zshort=0.25, zmax=0.05, zrand=0.25,
                         percentage_points_in_c=0.9, rangemax=20.0, sigphi=3.141592653589793 / 180.0 * 3, sighit=0.2,
                         lamshort=0.08, max_angle_diff=3.0, max_angle_penalty=0.5)


class RnMatchParams(C.Structure):
    """tsd_rnmatch_params"""
    _fields_ = [("trials", C.c_int), ("size_control_set", C.c_int), ("eps_thresh", C.c_double), ("phi_max", C.c_double),
                ("ang_res", C.c_double)]


class MapParams(C.Structure):
    """tsd_map_params"""
    _fields_ = [("inflate", C.c_int32), ("inflate_factor", C.c_int32)]


class MapWindow(C.Structure):
    """tsd_map_window"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]

    def as_tuple(self):
        return (int(self.x), int(self.y), int(self.width), int(self.height))


CLEARANCE_MAX_RADIUS = 255
DIST2_NONE = 0xFFFF      # the distance field's value where no obstacle lies within the radius


class CostmapParams(C.Structure):
    """tsd_costmap_params"""
    _fields_ = [("radius_cells", C.c_int32), ("want_dist2", C.c_int32), ("inscribed_radius_m", C.c_double),
                ("cost_scaling", C.c_double)]


FRONTIER_MAX_SEEDS = 16
FRONTIER_NONE = 0xFFFFFFFF   # the label image's value off the frontier cells


class Frontier(C.Structure):
    """tsd_frontier"""
    _fields_ = [("root_x", C.c_int32), ("root_y", C.c_int32), ("size", C.c_uint32), ("reachable", C.c_int32),
                ("sum_x", C.c_uint64), ("sum_y", C.c_uint64), ("min_x", C.c_int32), ("min_y", C.c_int32),
                ("max_x", C.c_int32), ("max_y", C.c_int32)]


FRONTIER_DTYPE = np.dtype([("root_x", "<i4"), ("root_y", "<i4"), ("size", "<u4"), ("reachable", "<i4"), ("sum_x", "<u8"),
                           ("sum_y", "<u8"), ("min_x", "<i4"), ("min_y", "<i4"), ("max_x", "<i4"), ("max_y", "<i4")])
assert FRONTIER_DTYPE.itemsize == C.sizeof(Frontier) == 48


class FrontierParams(C.Structure):
    """tsd_frontier_params"""
    _fields_ = [("free_max", C.c_int32), ("min_size", C.c_uint32), ("n_seeds", C.c_int32), ("reserved", C.c_int32),
                ("seeds_xy", C.POINTER(C.c_int32))]


ROUTE_NONE = 0xFFFFFFFF      # the key image's value where no path within the limit ends
ROUTE_MAX_DIST = 0x0FFFF000
ROUTE_SOURCES = {"map": 0, "costmap": 1}


class RouteParams(C.Structure):
    """tsd_route_params"""
    _fields_ = [("free_max", C.c_int32), ("n_seeds", C.c_int32), ("seeds_xy", C.POINTER(C.c_int32)),
                ("weights", C.POINTER(C.c_uint8)), ("limit", C.c_uint32), ("max_rounds", C.c_int32)]


class RouteInfo(C.Structure):
    """tsd_route_info"""
    _fields_ = [("seeds_used", C.c_int32), ("rounds", C.c_int32), ("converged", C.c_int32), ("reached", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RouteFieldsInfo(C.Structure):
    """tsd_route_fields_info"""
    _fields_ = [("layers", C.c_int32), ("rounds", C.c_int32), ("converged", C.c_int32), ("seeds_used", C.c_int32),
                ("used", C.c_uint8 * 16), ("reached", C.c_uint32 * 16)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in ("layers", "rounds", "converged", "seeds_used")}
        d["used"] = [int(v) for v in self.used]
        d["reached"] = [int(v) for v in self.reached]
        return d


class RouteGoal(C.Structure):
    """tsd_route_goal"""
    _fields_ = [("cell", C.c_uint32), ("dist", C.c_uint32), ("seed", C.c_int32), ("reserved", C.c_uint32)]


ROUTE_GOAL_DTYPE = np.dtype([("cell", "<u4"), ("dist", "<u4"), ("seed", "<i4"), ("reserved", "<u4")])
assert ROUTE_GOAL_DTYPE.itemsize == C.sizeof(RouteGoal) == 16


WAYPOINT_MAX_LOOKAHEAD = 1024
ROUTE_MAX_GOALS = 4096


class WaypointParams(C.Structure):
    """tsd_waypoint_params"""
    _fields_ = [("lookahead", C.c_int32), ("slack", C.c_uint32), ("max_len", C.c_int32), ("max_way", C.c_int32)]


class WaypointInfo(C.Structure):
    """tsd_waypoint_info"""
    _fields_ = [("len", C.c_int32), ("n_way", C.c_int32), ("cost", C.c_uint32), ("dist", C.c_uint32)]


WAYPOINT_INFO_DTYPE = np.dtype([("len", "<i4"), ("n_way", "<i4"), ("cost", "<u4"), ("dist", "<u4")])
assert WAYPOINT_INFO_DTYPE.itemsize == C.sizeof(WaypointInfo) == C.sizeof(WaypointParams) == 16


DRIVE_HEADINGS = 4096
DRIVE_MAX_STEPS = 256
DRIVE_MAX_SPEEDS = 64
DRIVE_MAX_TURNS = 129
DRIVE_MAX_BODY = 64
DRIVE_MAX_ROBOTS = 16
DRIVE_NONE = 0xFFFFFFFFFFFFFFFF   # the score of a refused sample, and of a choice without an admissible one


class DriveParams(C.Structure):
    _fields_ = [("steps", C.c_int32), ("n_speeds", C.c_int32), ("n_turns", C.c_int32), ("n_body", C.c_int32),
                ("step_q16", C.POINTER(C.c_int32)), ("turn", C.POINTER(C.c_int32)), ("body_q16", C.POINTER(C.c_int32)),
                ("a_end", C.c_int32), ("a_nose", C.c_int32), ("a_cost", C.c_int32), ("a_turn", C.c_int32),
                ("nose_q16", C.c_int32), ("nose_miss", C.c_uint32)]


class DrivePose(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("fx", C.c_int32), ("fy", C.c_int32), ("heading", C.c_int32), ("layer", C.c_int32)]


class DriveChoice(C.Structure):
    _fields_ = [("speed", C.c_int32), ("turn", C.c_int32), ("admissible", C.c_int32), ("end_cell", C.c_uint32), ("d_end", C.c_uint32),
                ("d_nose", C.c_uint32), ("cost", C.c_uint32), ("reserved", C.c_uint32), ("score", C.c_uint64)]


class DriveFleetParams(C.Structure):
    """tsd_drive_fleet_params"""
    _fields_ = [("order", C.POINTER(C.c_int32)), ("sep_q16", C.c_int32), ("reserved", C.c_int32)]


class DriveLiveParams(C.Structure):
    """tsd_drive_live_params"""
    _fields_ = [("radius", C.c_int32), ("n_skip", C.c_int32), ("skip", C.POINTER(C.c_int32))]


DRIVE_LIVE_MAX_POINTS = 32768     # tsd_drive_live_set's limits: points, skip discs, the radius in cells
DRIVE_LIVE_MAX_SKIP = 16
DRIVE_LIVE_MAX_RADIUS = 64
DRIVE_MAX_SEP = 128 * 65536       # tsd_drive_fleet_rollout's largest separation, Q16 cells
DRIVE_POSE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("fx", "<i4"), ("fy", "<i4"), ("heading", "<i4"), ("layer", "<i4")])
DRIVE_CHOICE_DTYPE = np.dtype([("speed", "<i4"), ("turn", "<i4"), ("admissible", "<i4"), ("end_cell", "<u4"), ("d_end", "<u4"),
                               ("d_nose", "<u4"), ("cost", "<u4"), ("reserved", "<u4"), ("score", "<u8")])


VIEW_MAX_RADIUS = 511
VIEW_MAX_CELLS = 4096


class ViewParams(C.Structure):
    """tsd_view_params"""
    _fields_ = [("free_max", C.c_int32), ("radius", C.c_int32), ("unknown_depth", C.c_int32), ("use_claims", C.c_int32)]


class ViewGain(C.Structure):
    """tsd_view_gain"""
    _fields_ = [("cell", C.c_uint32), ("gain", C.c_uint32), ("unknown", C.c_uint32), ("visible", C.c_uint32)]


VIEW_GAIN_DTYPE = np.dtype([("cell", "<u4"), ("gain", "<u4"), ("unknown", "<u4"), ("visible", "<u4")])
assert VIEW_GAIN_DTYPE.itemsize == C.sizeof(ViewGain) == C.sizeof(ViewParams) == 16


class FuseStats(C.Structure):
    """tsd_fuse_stats"""
    _fields_ = [("tiles_materialised", C.c_int64), ("tiles_empty", C.c_int64), ("cells_valid", C.c_int64),
                ("cells_one_source", C.c_int64), ("cells_many_sources", C.c_int64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RnMatchResult(C.Structure):
    """tsd_rnmatch_result"""
    _fields_ = [("T", C.c_double * 9), ("ratio", C.c_double), ("err_sum", C.c_double), ("cnt_match", C.c_int32),
                ("max_cnt_match", C.c_int32), ("idx_model", C.c_int32), ("idx_scene", C.c_int32), ("candidates", C.c_int32),
                ("valid_model", C.c_int32), ("valid_scene", C.c_int32), ("control_points", C.c_int32), ("reserved", C.c_int32 * 2)]


# the node's defaults for registration_mode 1 (ThreadLocalize.cpp:105-107, :183): RnMatchParams fields -> value
RNMATCH_DEFAULTS = dict(trials=100, size_control_set=140, eps_thresh=0.15)


class IcpResult(C.Structure):
    _fields_ = [
        ("T", C.c_double * 9),
        ("rms", C.c_double),
        ("pairs", C.c_int32),
        ("iterations", C.c_int32),
        ("state", C.c_int32),
        ("n_model", C.c_int32),
        ("n_scene", C.c_int32),
        ("reserved", C.c_int32),
    ]


class GridDigest(C.Structure):
    """tsd_grid_digest_t"""
    _fields_ = [("hash", C.c_uint64), ("cells_valid", C.c_int64), ("tiles_initialized", C.c_int32),
                ("reserved", C.c_int32), ("sum_tsd", C.c_double), ("sum_weight", C.c_double)]

    def as_dict(self):
        return dict(hash=int(self.hash), cells_valid=int(self.cells_valid), tiles_initialized=int(self.tiles_initialized),
                    sum_tsd=float(self.sum_tsd), sum_weight=float(self.sum_weight))


class GateParams(C.Structure):
    _fields_ = [("reg_trs_max", C.c_double), ("reg_sin_rot_max", C.c_double),
                ("trs_min", C.c_double), ("rot_min", C.c_double)]


class ScanResult(C.Structure):
    _fields_ = [("icp", IcpResult), ("pose", C.c_double * 9), ("reg_error", C.c_int32), ("pushed", C.c_int32),
                ("no_model", C.c_int32), ("reserved", C.c_int32)]


RELOC_MAX_PEAKS = 64
RELOC_MAX_CANDIDATES = 1 << 26


class RelocParams(C.Structure):
    """tsd_reloc_params"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("step_xy", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("ntheta", C.c_int32), ("theta_wraps", C.c_int32), ("cos_sin", C.POINTER(C.c_double)), ("theta0", C.c_double),
                ("dtheta", C.c_double), ("K", C.c_int32), ("min_pairs", C.c_int32)]


class RelocResult(C.Structure):
    """tsd_reloc_result"""
    _fields_ = [("found", C.c_int32), ("winner_idx", C.c_int32), ("pose33", C.c_double * 9), ("coarse_x", C.c_double),
                ("coarse_y", C.c_double), ("coarse_cos", C.c_double), ("coarse_sin", C.c_double), ("winner_score", C.c_uint32),
                ("n_peaks", C.c_int32), ("n_refined", C.c_int32), ("reserved", C.c_int32), ("icp", IcpResult),
                ("search_ms", C.c_double), ("refine_ms", C.c_double)]


ALIGN_MAX_POINTS = 1 << 20
ALIGN_MAXITER, ALIGN_CONVERGED, ALIGN_DEGENERATE = 0, 1, 2


class AlignParams(C.Structure):
    """tsd_align_params"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("step_xy", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("ntheta", C.c_int32), ("theta_wraps", C.c_int32), ("cos_sin", C.POINTER(C.c_double)), ("theta0", C.c_double),
                ("dtheta", C.c_double), ("K", C.c_int32), ("iterations", C.c_int32), ("pivot_x", C.c_double), ("pivot_y", C.c_double),
                ("v_cut", C.c_double), ("eps", C.c_double), ("lever", C.c_double), ("min_overlap", C.c_double), ("max_rms", C.c_double)]


class AlignPeak(C.Structure):
    """tsd_align_peak"""
    _fields_ = [("idx", C.c_int32), ("score", C.c_uint32), ("status", C.c_int32), ("iterations", C.c_int32), ("n_ok", C.c_int32),
                ("reserved", C.c_int32), ("m", C.c_double * 2), ("c", C.c_double), ("s", C.c_double), ("gain", C.c_double),
                ("sums", C.c_double * 11)]


class AlignResult(C.Structure):
    """tsd_align_result"""
    _fields_ = [("found", C.c_int32), ("winner_idx", C.c_int32), ("T33", C.c_double * 9), ("coarse_x", C.c_double),
                ("coarse_y", C.c_double), ("coarse_cos", C.c_double), ("coarse_sin", C.c_double), ("winner_score", C.c_uint32),
                ("n_peaks", C.c_int32), ("n_refined", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("n", C.c_int32), ("stride", C.c_int32), ("n_ok", C.c_int32), ("weight_sum", C.c_double), ("rms", C.c_double),
                ("overlap", C.c_double), ("info", C.c_double * 6), ("cell_off", C.c_int32 * 2), ("cell_error", C.c_double),
                ("search_ms", C.c_double), ("refine_ms", C.c_double)]


class SurfaceParams(C.Structure):
    """tsd_surface_params"""
    _fields_ = [("tx0", C.c_int32), ("ty0", C.c_int32), ("tx1", C.c_int32), ("ty1", C.c_int32), ("want_normals", C.c_int32),
                ("reserved", C.c_int32)]


# every symbol include/tsd_hip.h declares: name -> (restype, argtypes)
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_i8p = C.POINTER(C.c_int8)
_ip = C.POINTER(C.c_int)
ABI = {
    "tsd_device_count": (C.c_int, []),
    "tsd_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tsd_create": (C.c_void_p, [C.c_int, C.c_int, C.c_double, C.c_double]),
    "tsd_destroy": (None, [C.c_void_p]),
    "tsd_reset": (C.c_int, [C.c_void_p]),
    "tsd_set_max_truncation": (C.c_int, [C.c_void_p, C.c_double]),
    "tsd_sync": (C.c_int, [C.c_void_p]),
    "tsd_device": (C.c_int, [C.c_void_p]),
    "tsd_stream": (C.c_void_p, [C.c_void_p]),
    "tsd_last_error": (C.c_char_p, [C.c_void_p]),
    "tsd_cells": (C.c_int, [C.c_void_p]),
    "tsd_tiles": (C.c_int, [C.c_void_p]),
    "tsd_cell_size": (C.c_double, [C.c_void_p]),
    "tsd_max_truncation": (C.c_double, [C.c_void_p]),
    "tsd_min_x": (C.c_double, [C.c_void_p]),
    "tsd_max_x": (C.c_double, [C.c_void_p]),
    "tsd_min_y": (C.c_double, [C.c_void_p]),
    "tsd_max_y": (C.c_double, [C.c_void_p]),
    "tsd_free_footprint": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_double]),
    "tsd_push": (C.c_int, [C.c_void_p, _dp, _dp, _u8p, C.c_int, C.c_double, C.c_double, C.c_double,
                           C.c_double, C.c_double, C.POINTER(PushStats)]),
    "tsd_raycast": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_double, C.c_double, _dp, _dp, _u8p, _ip]),
    "tsd_icp": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, C.c_int, _dp, C.POINTER(IcpParams),
                          C.POINTER(IcpResult)]),
    "tsd_icp_normals": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _dp, C.c_int, _dp, C.POINTER(IcpParams),
                                  C.POINTER(IcpResult)]),
    "tsd_localize": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _u8p, C.c_int, C.c_double, C.c_double,
                               C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "tsd_sensor_create": (C.c_void_p, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "tsd_sensor_destroy": (None, [C.c_void_p]),
    "tsd_sensor_set_pose": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "tsd_scan": (C.c_int, [C.c_void_p, _dp, _u8p, _u8p, C.POINTER(IcpParams), C.POINTER(GateParams),
                           C.POINTER(ScanResult)]),
    "tsd_scan_submit": (C.c_int, [C.c_void_p, _dp, _u8p, _u8p, C.POINTER(IcpParams), C.POINTER(GateParams)]),
    "tsd_scan_stage": (C.c_int, [C.c_void_p, _dp, _u8p, _u8p]),
    "tsd_scan_collect": (C.c_int, [C.c_void_p, C.POINTER(ScanResult)]),
    "tsd_scan_begin": (C.c_int, [C.c_void_p, _dp, _u8p, _u8p, C.POINTER(IcpParams), C.POINTER(GateParams)]),
    "tsd_scan_wait": (C.c_int, [C.c_void_p]),
    "tsd_scan_finish": (C.c_int, [C.c_void_p, C.POINTER(ScanResult)]),
    "tsd_batch_create": (C.c_void_p, [C.c_void_p, C.c_int]),
    "tsd_batch_destroy": (None, [C.c_void_p]),
    "tsd_batch_capacity": (C.c_int, [C.c_void_p]),
    "tsd_batch_inflight": (C.c_int, [C.c_void_p]),
    "tsd_batch_begin": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(_dp), C.POINTER(_u8p), C.POINTER(_u8p),
                                  C.POINTER(IcpParams), C.POINTER(GateParams)]),
    "tsd_batch_push": (C.c_int, [C.c_void_p]),
    "tsd_batch_poll": (C.c_int, [C.c_void_p]),
    "tsd_batch_results": (C.c_int, [C.c_void_p, C.POINTER(ScanResult)]),
    "tsd_icp_trace": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "tsd_tsdpdf_match": (C.c_int, [C.c_void_p, _dp, _dp, _u8p, _dp, _u8p, C.c_int, C.POINTER(TsdPdfParams), _ip, _ip, _ip,
                                   C.POINTER(TsdPdfResult)]),
    "tsd_pdf_match": (C.c_int, [C.c_void_p, _dp, _u8p, _dp, _u8p, C.c_int, C.POINTER(PdfMatchParams), _ip, _ip, _ip,
                                C.POINTER(TsdPdfResult)]),
    "tsd_debug_pdf_match_scores": (C.c_int, [C.c_void_p, _dp, _ip, C.c_int]),
    "tsd_rn_match": (C.c_int, [C.c_void_p, _dp, _u8p, _dp, _u8p, C.c_int, C.POINTER(RnMatchParams), _ip, _ip, _ip,
                               C.POINTER(RnMatchResult)]),
    "tsd_debug_rn_match_scores": (C.c_int, [C.c_void_p, _ip, _ip, _dp, C.c_int]),
    "tsd_debug_rn_select": (C.c_int, [C.c_void_p, _ip, _ip, _dp, C.c_int, C.c_int, _ip]),
    "tsd_relocalize": (C.c_int, [C.c_void_p, C.POINTER(RelocParams), _dp, C.c_int, _dp, _dp, _u8p, C.c_int, C.c_double, C.c_double,
                                 C.POINTER(IcpParams), C.POINTER(RelocResult)]),
    "tsd_debug_reloc_scores": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "tsd_debug_reloc_peaks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _ip]),
    "tsd_align_points": (C.c_int, [C.c_void_p, C.POINTER(AlignParams), C.c_void_p, C.c_int, C.c_int, C.POINTER(AlignResult)]),
    "tsd_map_align": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AlignParams), C.POINTER(AlignResult)]),
    "tsd_debug_align_scores": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "tsd_debug_align_peaks": (C.c_int, [C.c_void_p, C.POINTER(AlignPeak), C.c_int]),
    "tsd_debug_align_sums": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, _ip]),
    "tsd_surface_extract": (C.c_int, [C.c_void_p, C.POINTER(SurfaceParams), _ip]),
    "tsd_surface_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _u8p]),
    "tsd_surface_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _ip]),
    "tsd_scan_preregister": (C.c_int, [C.c_void_p, C.POINTER(TsdPdfParams), _dp, _u8p, _ip, _ip, _ip]),
    "tsd_scan_preregistration_result": (C.c_int, [C.c_void_p, C.POINTER(TsdPdfResult)]),
    "tsd_sensor_set_async_mapping": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_debug_stall_push_stream": (C.c_int, [C.c_void_p, C.c_uint]),
    "tsd_debug_set_icp_helpers": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_debug_sensor_scan_path": (C.c_int, [C.c_void_p]),
    "tsd_debug_set_push_multi": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_color_image": (C.c_int, [C.c_void_p, _u8p, C.c_uint, C.c_uint]),
    "tsd_map_frame_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_map_frame_wait": (C.c_int, [C.c_void_p, _ip]),
    "tsd_map_update_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_map_update_wait": (C.c_int, [C.c_void_p, _ip]),
    "tsd_costmap_table": (C.c_int, [C.c_double, C.c_int, C.c_double, C.c_double, _i8p]),
    "tsd_clearance_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(MapWindow), C.c_int, _i8p,
                                    C.c_void_p, C.c_void_p]),
    "tsd_costmap_begin": (C.c_int, [C.c_void_p, C.POINTER(CostmapParams), C.c_void_p, C.c_void_p, C.POINTER(MapWindow),
                                    C.POINTER(MapWindow)]),
    "tsd_costmap_wait": (C.c_int, [C.c_void_p]),
    "tsd_debug_set_clearance_skip": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_frontiers_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FrontierParams), _ip, _ip]),
    "tsd_frontiers_frame": (C.c_int, [C.c_void_p, C.POINTER(FrontierParams), _ip, _ip]),
    "tsd_frontiers_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tsd_frontiers_dev_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _ip]),
    "tsd_frontiers_counts": (C.c_int, [C.c_void_p, _ip, _ip, _ip]),
    "tsd_route_weights": (C.c_int, [C.c_int, C.c_int, _u8p]),
    "tsd_route_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RouteParams), C.POINTER(RouteInfo)]),
    "tsd_route_frame": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RouteParams), C.POINTER(RouteInfo)]),
    "tsd_route_goals": (C.c_int, [C.c_void_p, _ip]),
    "tsd_route_goals_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tsd_route_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tsd_route_dev_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _ip, _ip]),
    "tsd_route_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _ip]),
    "tsd_debug_set_route_sweeps": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_route_waypoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(WaypointParams), C.c_void_p, C.c_void_p]),
    "tsd_route_fields_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RouteParams), C.POINTER(RouteFieldsInfo)]),
    "tsd_route_fields_frame": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RouteParams), C.POINTER(RouteFieldsInfo)]),
    "tsd_route_fields_goals": (C.c_int, [C.c_void_p, _ip]),
    "tsd_route_fields_goals_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tsd_route_fields_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tsd_route_fields_waypoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(WaypointParams), C.c_void_p, C.c_void_p]),
    "tsd_route_fields_dev_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _ip, _ip, _ip]),
    "tsd_route_fields_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _ip]),
    "tsd_drive_table": (C.c_int, [C.c_void_p]),
    "tsd_drive_advance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "tsd_drive_rollout": (C.c_int, [C.c_void_p, C.POINTER(DriveParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_drive_fields_rollout": (C.c_int, [C.c_void_p, C.POINTER(DriveParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_drive_fleet_rollout": (C.c_int, [C.c_void_p, C.POINTER(DriveParams), C.POINTER(DriveFleetParams), C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsd_drive_fields_togo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tsd_drive_dev_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong)]),
    "tsd_drive_live_set": (C.c_int, [C.c_void_p, C.POINTER(DriveLiveParams), C.c_void_p, C.c_int, C.c_int, C.c_int, _ip]),
    "tsd_drive_live_clear": (C.c_int, [C.c_void_p]),
    "tsd_drive_live_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, _ip, _ip, _ip]),
    "tsd_drive_live_dev_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _ip, _ip, _ip]),
    "tsd_view_assign_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ViewParams), C.c_void_p, C.c_int, C.c_int,
                                         C.c_uint32, C.c_void_p, C.c_void_p, _ip]),
    "tsd_view_gains": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ViewParams), C.c_void_p, C.c_int, C.c_void_p]),
    "tsd_view_claim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ViewParams), C.c_void_p, C.c_int]),
    "tsd_view_claims_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "tsd_view_claims_dev_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _ip, _ip]),
    "tsd_view_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ViewParams), C.c_void_p, C.c_int, C.c_int,
                                  C.c_uint32, C.c_void_p, C.c_void_p, _ip]),
    "tsd_dev_alloc": (C.c_void_p, [C.c_void_p, C.c_uint64]),
    "tsd_dev_free": (None, [C.c_void_p, C.c_void_p]),
    "tsd_dev_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "tsd_host_alloc": (C.c_void_p, [C.c_uint64]),
    "tsd_host_free": (None, [C.c_void_p]),
    "tsd_store_grid_text": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tsd_load_grid_text": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tsd_download_tiles": (C.c_int, [C.c_void_p, _u8p, _dp, _dp, _dp]),
    "tsd_upload_tiles": (C.c_int, [C.c_void_p, _u8p, _dp, _dp, _dp]),
    "tsd_download_tile_state": (C.c_int, [C.c_void_p, _u8p, _dp]),
    "tsd_grid_digest": (C.c_int, [C.c_void_p, C.POINTER(GridDigest)]),
    "tsd_storage_bits": (C.c_int, []),
    "tsd_abi_sizeof": (C.c_int, [C.c_char_p]),
    "tsd_occupancy": (C.c_int, [C.c_void_p, _i8p, C.c_int, C.c_int, _ip]),
    "tsd_occupancy_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "tsd_occupancy_dev_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "tsd_group_create": (C.c_void_p, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "tsd_group_create_rigid": (C.c_void_p, [C.c_int, C.POINTER(C.c_void_p), _dp, C.c_int, C.c_int]),
    "tsd_group_member_transform": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "tsd_group_cell_offsets": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "tsd_group_destroy": (None, [C.c_void_p]),
    "tsd_group_size": (C.c_int, [C.c_void_p]),
    "tsd_group_width": (C.c_int, [C.c_void_p]),
    "tsd_group_height": (C.c_int, [C.c_void_p]),
    "tsd_group_corner": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsd_group_last_error": (C.c_char_p, [C.c_void_p]),
    "tsd_group_merge_begin": (C.c_int, [C.c_void_p, C.POINTER(MapParams), C.c_void_p]),
    "tsd_group_extract_begin": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(MapParams)]),
    "tsd_group_merge_maps_begin": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "tsd_group_member_map_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "tsd_group_merge_wait": (C.c_int, [C.c_void_p, _ip]),
    "tsd_group_map_dev": (C.c_void_p, [C.c_void_p]),
    "tsd_group_member_map_dev": (C.c_void_p, [C.c_void_p, C.c_int]),
    "tsd_group_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_group_merge_times": (C.c_int, [C.c_void_p, _dp, _dp, _ip]),
    "tsd_fuse_begin": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "tsd_fuse_wait": (C.c_int, [C.c_void_p, C.POINTER(FuseStats)]),
    "tsd_fuse": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(FuseStats)]),
    "tsd_icp_pairs": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, C.c_int, _dp, C.POINTER(IcpParams), C.c_int, _ip, _ip, _ip]),
    "tsd_calibrate_rmw": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "tsd_measure_stream": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _dp, _dp]),
    "tsd_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_profile_select": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tsd_profile_reset": (C.c_int, [C.c_void_p]),
    "tsd_push_stats_total": (C.c_int, [C.c_void_p, C.POINTER(PushStats), C.POINTER(C.c_int64), C.c_int]),
    "tsd_profile_get": (C.c_int, [C.c_void_p, C.c_char_p, _dp, _ip]),
    "tsd_profile_get_spread": (C.c_int, [C.c_void_p, C.c_char_p, _dp, _dp, _dp]),
    "tsd_profile_get_samples": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int]),
}

_lib = None


def load_library(path: str | None = None):
    """Load ``libtsd_hip.so`` and bind every ABI symbol.  Raises if the library is missing: the HIP
    extension is the only implementation."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise TsdError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fall-back")
    lib = C.CDLL(p)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)     # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    # the ctypes mirrors of the public structs must have the library's layout
    for cname, mirror in (("tsd_push_stats", PushStats), ("tsd_icp_params", IcpParams), ("tsd_icp_result", IcpResult),
                          ("tsd_gate_params", GateParams), ("tsd_scan_result", ScanResult), ("tsd_grid_digest_t", GridDigest),
                          ("tsd_tsdpdf_params", TsdPdfParams), ("tsd_tsdpdf_result", TsdPdfResult),
                          ("tsd_pdfmatch_params", PdfMatchParams), ("tsd_rnmatch_params", RnMatchParams),
                          ("tsd_rnmatch_result", RnMatchResult), ("tsd_map_params", MapParams),
                          ("tsd_fuse_stats", FuseStats), ("tsd_map_window", MapWindow), ("tsd_reloc_params", RelocParams),
                          ("tsd_reloc_result", RelocResult), ("tsd_surface_params", SurfaceParams),
                          ("tsd_align_params", AlignParams), ("tsd_align_peak", AlignPeak), ("tsd_align_result", AlignResult),
                          ("tsd_costmap_params", CostmapParams), ("tsd_frontier", Frontier),
                          ("tsd_frontier_params", FrontierParams), ("tsd_route_params", RouteParams),
                          ("tsd_route_info", RouteInfo), ("tsd_route_goal", RouteGoal), ("tsd_route_fields_info", RouteFieldsInfo),
                          ("tsd_view_params", ViewParams), ("tsd_view_gain", ViewGain),
                          ("tsd_waypoint_params", WaypointParams), ("tsd_waypoint_info", WaypointInfo),
                          ("tsd_drive_params", DriveParams), ("tsd_drive_pose", DrivePose), ("tsd_drive_choice", DriveChoice),
                          ("tsd_drive_fleet_params", DriveFleetParams), ("tsd_drive_live_params", DriveLiveParams)):
        if lib.tsd_abi_sizeof(cname.encode()) != C.sizeof(mirror):
            raise TsdError(f"ABI mismatch: sizeof({cname}) = {lib.tsd_abi_sizeof(cname.encode())} in {p}, {C.sizeof(mirror)} in capi.py")
    if path is None:
        _lib = lib
    return lib


def device_memory(device: int = 0):
    """(free, total) bytes of `device` as the product's own HIP runtime reports them (tsd_device_memory)."""
    lib = load_library()
    f, t = C.c_uint64(0), C.c_uint64(0)
    rc = lib.tsd_device_memory(device, C.byref(f), C.byref(t))
    if rc != 0:
        raise TsdError(f"tsd_device_memory({device}) failed ({rc})")
    return f.value, t.value


def route_weights(free_max=0, max_weight=1) -> np.ndarray:
    """tsd_route_weights: the uint8 table W[0 .. free_max] = 1 + v * (max_weight - 1) / 98 of the routes (host code: no GPU)"""
    lib = load_library()
    tab = np.zeros(max(int(free_max), 0) + 1, dtype=np.uint8)
    rc = lib.tsd_route_weights(int(free_max), int(max_weight), tab.ctypes.data_as(_u8p))
    if rc != 0:
        raise TsdError(f"tsd_route_weights refused (rc {rc}): free_max {free_max}, max_weight {max_weight}")
    return tab


def drive_table() -> np.ndarray:
    """tsd_drive_table: the direction table int32 (DRIVE_HEADINGS, 2), row h = (cx, cy) in Q16 (host code: no GPU)"""
    lib = load_library()
    tab = np.zeros((DRIVE_HEADINGS, 2), dtype=np.int32)
    if lib.tsd_drive_table(tab.ctypes.data) != 0:
        raise TsdError("tsd_drive_table refused")
    return tab


def drive_poses(poses) -> np.ndarray:
    """poses as a DRIVE_POSE_DTYPE array: a structured array, or rows (x, y, fx, fy, heading[, layer])"""
    if isinstance(poses, np.ndarray) and poses.dtype == DRIVE_POSE_DTYPE:
        return np.ascontiguousarray(poses).ravel()
    rows = np.asarray(list(poses), dtype=np.int64).reshape(len(poses), -1)
    out = np.zeros(rows.shape[0], dtype=DRIVE_POSE_DTYPE)
    for k, name in enumerate(DRIVE_POSE_DTYPE.names[:rows.shape[1]]):
        out[name] = rows[:, k]
    return out


def drive_advance(pose, step_q16: int, turn: int, n_steps: int = 1) -> np.ndarray:
    """tsd_drive_advance: the pose (one DRIVE_POSE_DTYPE record) after ``n_steps`` steps of the rule's trajectory (host code: no GPU)"""
    lib = load_library()
    p = drive_poses([pose] if not isinstance(pose, np.ndarray) else pose)
    assert p.size == 1
    out = np.zeros(1, dtype=DRIVE_POSE_DTYPE)
    rc = lib.tsd_drive_advance(p.ctypes.data, int(step_q16), int(turn), int(n_steps), out.ctypes.data)
    if rc != 0:
        raise TsdError(f"tsd_drive_advance refused (rc {rc}): pose {p[0]}, step {step_q16}, turn {turn}, n_steps {n_steps}")
    return out[0]


def costmap_table(cell_size, radius, inscribed_radius_m=0.25, cost_scaling=10.0) -> np.ndarray:
    """tsd_costmap_table: the int8 table [radius^2 + 1] of nav2's inflation layer on the OccupancyGrid scale (host code: no GPU)"""
    lib = load_library()
    tab = np.zeros(max(int(radius), 0) ** 2 + 1, dtype=np.int8)
    rc = lib.tsd_costmap_table(float(cell_size), int(radius), float(inscribed_radius_m), float(cost_scaling), tab.ctypes.data_as(_i8p))
    if rc != 0:
        raise TsdError(f"tsd_costmap_table refused (rc {rc}): radius {radius}, cell size {cell_size}")
    return tab


class DeviceBuffer:
    """``nbytes`` of plain device memory on a grid's device (tsd_dev_alloc / _free / _copy, through the library's own HIP runtime),
    for maps handed to ``clearance_of`` and for its outputs.  Free it before the grid is closed."""

    def __init__(self, grid, nbytes: int):
        self.grid, self.nbytes = grid, int(nbytes)
        self.ptr = grid.lib.tsd_dev_alloc(grid.h, max(self.nbytes, 1))
        if not self.ptr:
            raise TsdError(f"tsd_dev_alloc({nbytes}) failed")

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        self.grid._check(self.grid.lib.tsd_dev_copy(self.grid.h, self.ptr + offset, a.ctypes.data, a.nbytes, 1), "tsd_dev_copy")

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.zeros(count, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        self.grid._check(self.grid.lib.tsd_dev_copy(self.grid.h, out.ctypes.data, self.ptr + offset, out.nbytes, 0), "tsd_dev_copy")
        return out

    def free(self):
        if getattr(self, "ptr", None) and getattr(self.grid, "h", None):
            self.grid.lib.tsd_dev_free(self.grid.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _d(a):
    return a.ctypes.data_as(_dp)


def _u8(a):
    return a.ctypes.data_as(_u8p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


@dataclass
class IcpOut:
    T: np.ndarray
    rms: float
    pairs: int
    iterations: int
    state: int
    n_model: int = 0
    n_scene: int = 0
    seeded: int = 0         # tsd_icp_result.reserved: scene points whose step-0 search came from the helper workgroups


class TsdGridDevice:
    """One TSD grid resident in the HBM of one GPU (``obvious::TsdGrid`` as constructed by
    ``SlamNode::initialize``, SlamNode.cpp:77-78)."""

    def __init__(self, map_size_log2: int, cell_size: float, max_trunc: float, device: int = 0, storage: str = "f64"):
        """storage: "f64" (the reference's cells, lib/libtsd_hip.so) or "q32" (8 bytes per cell, lib/libtsd_hip_q32.so)"""
        self.lib = load_library() if storage == "f64" else load_library(LIB_PATH_Q32)
        assert self.lib.tsd_storage_bits() == (64 if storage == "f64" else 32)
        if self.lib.tsd_device_count() <= 0:
            raise TsdError("no HIP device visible: the TSD hot path only exists as gfx950 kernels")
        self.h = self.lib.tsd_create(device, map_size_log2, cell_size, max_trunc)
        if not self.h:
            raise TsdError("tsd_create failed")
        self.cells = self.lib.tsd_cells(self.h)
        self.tiles = self.lib.tsd_tiles(self.h)
        self.cell_size = self.lib.tsd_cell_size(self.h)
        self.max_trunc = self.lib.tsd_max_truncation(self.h)
        self.min_x, self.max_x = self.lib.tsd_min_x(self.h), self.lib.tsd_max_x(self.h)
        self.min_y, self.max_y = self.lib.tsd_min_y(self.h), self.lib.tsd_max_y(self.h)

    def close(self):
        for buf in getattr(self, "_dev_bufs", {}).values():
            buf.free()
        self._dev_bufs = {}
        if getattr(self, "h", None):
            self.lib.tsd_destroy(self.h)
            self.h = None
        for ptr in getattr(self, "_frame_bufs", {}).values():
            self.lib.tsd_host_free(ptr)
        self._frame_bufs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise TsdError(f"{what} failed ({rc}): {self.lib.tsd_last_error(self.h).decode()}")

    def reset(self):
        self._check(self.lib.tsd_reset(self.h), "tsd_reset")

    def sync(self):
        self._check(self.lib.tsd_sync(self.h), "tsd_sync")

    def set_max_truncation(self, val) -> float:
        """TsdGrid::setMaxTruncation on the live grid (tsd_set_max_truncation): the truncation the context reports afterwards."""
        self._check(self.lib.tsd_set_max_truncation(self.h, float(val)), "tsd_set_max_truncation")
        self.max_trunc = self.lib.tsd_max_truncation(self.h)
        return self.max_trunc

    def free_footprint(self, center, width, height) -> bool:
        c = _f64(center)
        rc = self.lib.tsd_free_footprint(self.h, _d(c), float(width), float(height))
        if rc == -4:
            return False
        self._check(rc, "tsd_free_footprint")
        return True

    def push(self, pose, ranges, mask, ang_res, phi_min, max_range, min_range, low_refl, want_stats=True):
        pose = _f64(pose).reshape(9)
        ranges = _f64(ranges)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        st = PushStats()
        rc = self.lib.tsd_push(self.h, _d(pose), _d(ranges), _u8(mask), ranges.size, ang_res, phi_min,
                               max_range, min_range, low_refl, C.byref(st) if want_stats else None)
        self._check(rc, "tsd_push")
        return st.as_dict() if want_stats else None

    def raycast(self, pose, rays_world, min_range, max_range):
        pose = _f64(pose).reshape(9)
        rays = _f64(rays_world)
        beams = rays.size // 2
        coords = np.zeros(2 * beams)
        normals = np.zeros(2 * beams)
        mask = np.zeros(beams, dtype=np.uint8)
        n = C.c_int(0)
        rc = self.lib.tsd_raycast(self.h, _d(pose), _d(rays), beams, min_range, max_range, _d(coords),
                                  _d(normals), _u8(mask), C.byref(n))
        self._check(rc, "tsd_raycast")
        return coords, normals, mask, n.value

    def icp_params(self, iterations, dist_max, dist_min, estimator: int = 0, t_init=None) -> IcpParams:
        p = IcpParams(iterations, estimator, dist_max, dist_min, self.min_x, self.max_x, self.min_y, self.max_y)
        if t_init is not None:
            p.t_init = (C.c_double * 9)(*_f64(t_init).reshape(9))
            p.use_t_init = 1
        return p

    def _match(self, fn, lead, model_xy, mask_m, scene_xy, mask_s, prm, result, draws_sub, draws_ctrl, draws_trials) -> dict:
        """the marshalling the three pre-registration calls share; the common record's fields of `result` as a dict"""
        M, S = _f64(model_xy).reshape(-1), _f64(scene_xy).reshape(-1)
        n = M.size // 2
        mM, mS = np.ascontiguousarray(mask_m, dtype=np.uint8), np.ascontiguousarray(mask_s, dtype=np.uint8)
        ds, dc, dt = (np.ascontiguousarray(x, dtype=np.int32) for x in (draws_sub, draws_ctrl, draws_trials))
        assert ds.size >= n and dc.size >= prm.size_control_set and dt.size >= prm.trials
        rc = getattr(self.lib, fn)(self.h, *lead, _d(M), _u8(mM), _d(S), _u8(mS), n, C.byref(prm), ds.ctypes.data_as(_ip),
                                   dc.ctypes.data_as(_ip), dt.ctypes.data_as(_ip), C.byref(result))
        self._check(rc, fn)
        return dict(T=np.array(result.T[:]).reshape(3, 3), idx=result.idx_model, i=result.idx_scene, candidates=result.candidates,
                    valid_model=result.valid_model, valid_scene=result.valid_scene, control=result.control_points)

    def tsdpdf_match(self, pose, model_xy, mask_m, scene_xy, mask_s, trials, size_control_set, zrand, phi_max, ang_res,
                     draws_sub, draws_ctrl, draws_trials, eps_thresh=0.15) -> dict:
        """obvious::TSD_PDFMatching::match with the rand() draws as inputs (tsd_tsdpdf_match)"""
        r = TsdPdfResult()
        return dict(self._match("tsd_tsdpdf_match", (_d(_f64(pose).reshape(9)),), model_xy, mask_m, scene_xy, mask_s,
                                TsdPdfParams(trials, size_control_set, eps_thresh, zrand, phi_max, ang_res), r,
                                draws_sub, draws_ctrl, draws_trials), prob=r.probability)

    def pdf_match(self, model_xy, mask_m, scene_xy, mask_s, phi_max, ang_res, draws_sub, draws_ctrl, draws_trials, **kw) -> dict:
        """obvious::PDFMatching::match with the rand() draws as inputs (tsd_pdf_match); `kw` overrides PDFMATCH_DEFAULTS"""
        r = TsdPdfResult()
        return dict(self._match("tsd_pdf_match", (), model_xy, mask_m, scene_xy, mask_s,
                                PdfMatchParams(phi_max=phi_max, ang_res=ang_res, **dict(PDFMATCH_DEFAULTS, **kw)), r,
                                draws_sub, draws_ctrl, draws_trials), prob=r.probability)

    def debug_pdf_match_scores(self):
        """TEST HOOK: the last pdf_match's ungated products and field-of-view counts, in candidate order"""
        n = self.lib.tsd_debug_pdf_match_scores(self.h, None, None, 0)
        self._check(min(n, 0), "tsd_debug_pdf_match_scores")
        p, f = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32)
        self.lib.tsd_debug_pdf_match_scores(self.h, _d(p), f.ctypes.data_as(_ip), n)
        return p[:n], f[:n]

    def rn_match(self, model_xy, mask_m, scene_xy, mask_s, phi_max, ang_res, draws_sub, draws_ctrl, draws_trials, **kw) -> dict:
        """obvious::RandomNormalMatching::match with the rand() draws as inputs (tsd_rn_match); `kw` overrides RNMATCH_DEFAULTS"""
        r = RnMatchResult()
        return dict(self._match("tsd_rn_match", (), model_xy, mask_m, scene_xy, mask_s,
                                RnMatchParams(phi_max=phi_max, ang_res=ang_res, **dict(RNMATCH_DEFAULTS, **kw)), r,
                                draws_sub, draws_ctrl, draws_trials),
                    ratio=r.ratio, err_sum=r.err_sum, cnt=r.cnt_match, max_cnt=r.max_cnt_match)

    def debug_rn_match_scores(self):
        """TEST HOOK: the last rn_match's cntMatch, maxCntMatch and errSum per candidate, in candidate order"""
        n = self.lib.tsd_debug_rn_match_scores(self.h, None, None, None, 0)
        self._check(min(n, 0), "tsd_debug_rn_match_scores")
        c, m, e = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1))
        self.lib.tsd_debug_rn_match_scores(self.h, c.ctypes.data_as(_ip), m.ctypes.data_as(_ip), _d(e), n)
        return c[:n], m[:n], e[:n]

    def debug_rn_select(self, cnt, max_cnt, err_sum, thresh) -> int:
        """TEST HOOK: the device selection of rn_match (Kuehn's rating in serial order) on given arrays: the winner's index or -1"""
        c, m = np.ascontiguousarray(cnt, dtype=np.int32), np.ascontiguousarray(max_cnt, dtype=np.int32)
        e = _f64(err_sum).reshape(-1)
        assert c.size == m.size == e.size
        w = C.c_int(-2)
        rc = self.lib.tsd_debug_rn_select(self.h, c.ctypes.data_as(_ip), m.ctypes.data_as(_ip), _d(e), int(c.size), int(thresh),
                                          C.byref(w))
        self._check(rc, "tsd_debug_rn_select")
        return w.value

    def icp(self, model_xy, scene_xy, pose, params: IcpParams, model_normals_xy=None) -> IcpOut:
        m = _f64(model_xy).reshape(-1)
        s = _f64(scene_xy).reshape(-1)
        pose = _f64(pose).reshape(9)
        r = IcpResult()
        if model_normals_xy is None:
            rc = self.lib.tsd_icp(self.h, _d(m), m.size // 2, _d(s), s.size // 2, _d(pose), C.byref(params), C.byref(r))
        else:
            nrm = _f64(model_normals_xy).reshape(-1)
            assert nrm.size == m.size
            rc = self.lib.tsd_icp_normals(self.h, _d(m), _d(nrm), m.size // 2, _d(s), s.size // 2, _d(pose),
                                          C.byref(params), C.byref(r))
        self._check(rc, "tsd_icp")
        return IcpOut(np.array(r.T[:]).reshape(3, 3), r.rms, r.pairs, r.iterations, r.state, seeded=r.reserved)

    def localize(self, pose, rays_world, rays_local, ranges, mask, min_range, max_range, params: IcpParams) -> IcpOut:
        pose = _f64(pose).reshape(9)
        rw, rl, rg = _f64(rays_world), _f64(rays_local), _f64(ranges)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        r = IcpResult()
        rc = self.lib.tsd_localize(self.h, _d(pose), _d(rw), _d(rl), _d(rg), _u8(mk), rg.size, min_range,
                                   max_range, C.byref(params), C.byref(r))
        self._check(rc, "tsd_localize")
        return IcpOut(np.array(r.T[:]).reshape(3, 3), r.rms, r.pairs, r.iterations, r.state, r.n_model, r.n_scene, seeded=r.reserved)

    def relocalize(self, points_xy, rays_local, ranges, mask, min_range, max_range, params: IcpParams, x0, y0, step_xy, nx, ny,
                   ntheta, theta0=0.0, dtheta=0.0, cos_sin=None, theta_wraps=False, K=16, min_pairs=0) -> dict:
        """tsd_relocalize: search the pose lattice (x0 + ix * step_xy, y0 + iy * step_xy, rotation k of ``cos_sin`` -- (ntheta, 2)
        cos / sin -- or of theta0 + k * dtheta) for the scan whose valid points in the sensor frame are ``points_xy`` (P, 2), refine the
        K best peaks with the registration of ``localize`` and keep the one with the most pairs.  Raises TsdError with the C code in
        ``.args`` text on a refused call."""
        pts, rl, rg = _f64(points_xy).reshape(-1), _f64(rays_local), _f64(ranges)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        tab = None if cos_sin is None else _f64(cos_sin).reshape(-1)
        assert tab is None or tab.size == 2 * ntheta
        prm = RelocParams(float(x0), float(y0), float(step_xy), int(nx), int(ny), int(ntheta), int(bool(theta_wraps)),
                          None if tab is None else _d(tab), float(theta0), float(dtheta), int(K), int(min_pairs))
        r = RelocResult()
        rc = self.lib.tsd_relocalize(self.h, C.byref(prm), _d(pts), pts.size // 2, _d(rl), _d(rg), _u8(mk), rg.size, min_range,
                                     max_range, C.byref(params), C.byref(r))
        self.last_rc = rc
        self._check(rc, "tsd_relocalize")
        i = r.icp
        return dict(found=bool(r.found), pose=np.array(r.pose33[:]).reshape(3, 3), idx=int(r.winner_idx), score=int(r.winner_score),
                    coarse=(r.coarse_x, r.coarse_y, r.coarse_cos, r.coarse_sin), n_peaks=int(r.n_peaks), n_refined=int(r.n_refined),
                    icp=IcpOut(np.array(i.T[:]).reshape(3, 3), i.rms, i.pairs, i.iterations, i.state, i.n_model, i.n_scene,
                               seeded=i.reserved),
                    search_ms=r.search_ms, refine_ms=r.refine_ms)

    def debug_reloc_scores(self) -> np.ndarray:
        """TEST HOOK: the score volume of the last relocalize, uint32 [nx * ny * ntheta] in candidate order (empty before the first search and
        after one of more than 2^23 candidates, whose volume the context does not keep)"""
        n = self.lib.tsd_debug_reloc_scores(self.h, None, 0)
        self._check(min(n, 0), "tsd_debug_reloc_scores")
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(min(self.lib.tsd_debug_reloc_scores(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n), 0), "tsd_debug_reloc_scores")
        return out[:n]

    def debug_reloc_peaks(self, scores, shape, wraps, K):
        """TEST HOOK: the device's peak selection on a volume ``scores`` of ``shape`` = (ntheta, ny, nx): (idx, score) of the K best
        peaks, score descending then idx ascending"""
        nt, ny, nx = (int(v) for v in shape)
        vol = np.ascontiguousarray(scores, dtype=np.uint32).reshape(-1)
        assert vol.size == nt * ny * nx
        idx, sc, n = np.zeros(RELOC_MAX_PEAKS, dtype=np.int32), np.zeros(RELOC_MAX_PEAKS, dtype=np.uint32), C.c_int(0)
        rc = self.lib.tsd_debug_reloc_peaks(self.h, vol.ctypes.data_as(C.POINTER(C.c_uint32)), nx, ny, nt, int(bool(wraps)), int(K),
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n))
        self._check(rc, "tsd_debug_reloc_peaks")
        return idx[:n.value].copy(), sc[:n.value].copy()

    @staticmethod
    def _align_params(x0, y0, step_xy, nx, ny, ntheta, theta0, dtheta, cos_sin, theta_wraps, K, iterations, pivot, v_cut, eps, lever,
                      min_overlap, max_rms):
        tab = None if cos_sin is None else _f64(cos_sin).reshape(-1)
        assert tab is None or tab.size == 2 * ntheta
        pv = (float("nan"), float("nan")) if pivot is None else (float(pivot[0]), float(pivot[1]))
        prm = AlignParams(float(x0), float(y0), float(step_xy), int(nx), int(ny), int(ntheta), int(bool(theta_wraps)),
                          None if tab is None else _d(tab), float(theta0), float(dtheta), int(K), int(iterations), pv[0], pv[1],
                          float(v_cut), float(eps), float(lever), float(min_overlap), float(max_rms))
        return prm, tab                # (the table must outlive the call)

    @staticmethod
    def _align_dict(r: AlignResult) -> dict:
        return dict(found=bool(r.found), T=np.array(r.T33[:]).reshape(3, 3), idx=int(r.winner_idx), score=int(r.winner_score),
                    coarse=(r.coarse_x, r.coarse_y, r.coarse_cos, r.coarse_sin), n_peaks=int(r.n_peaks), n_refined=int(r.n_refined),
                    iterations=int(r.iterations), converged=bool(r.converged), n=int(r.n), stride=int(r.stride), n_ok=int(r.n_ok),
                    weight_sum=r.weight_sum, rms=r.rms, overlap=r.overlap, info=np.array(r.info[:]),
                    cell_off=(int(r.cell_off[0]), int(r.cell_off[1])), cell_error=r.cell_error, search_ms=r.search_ms,
                    refine_ms=r.refine_ms, raw=bytes(r))

    def align_points(self, points_xy, x0, y0, step_xy, nx, ny, ntheta, pivot, theta0=0.0, dtheta=0.0, cos_sin=None,
                     theta_wraps=False, K=16, iterations=40, v_cut=0.75, eps=1e-6, lever=0.0, min_overlap=0.0, max_rms=0.0,
                     device_ptr=None, n=None) -> dict:
        """tsd_align_points: the rigid transform that carries ``points_xy`` (n, 2; field coordinates) into this grid: lattice search
        (a node is where ``pivot`` lands, the rotations turn about it), then the Gauss-Newton refinement of the K best peaks on the
        device.  ``device_ptr`` / ``n``: a list that lies on this grid's device instead.  Returns the result's fields as a dict (T:
        3 x 3, points -> grid)."""
        prm, tab = self._align_params(x0, y0, step_xy, nx, ny, ntheta, theta0, dtheta, cos_sin, theta_wraps, K, iterations, pivot,
                                      v_cut, eps, lever, min_overlap, max_rms)
        r = AlignResult()
        if device_ptr is None:
            pts = _f64(points_xy).reshape(-1)
            rc = self.lib.tsd_align_points(self.h, C.byref(prm), pts.ctypes.data, pts.size // 2, 0, C.byref(r))
        else:
            rc = self.lib.tsd_align_points(self.h, C.byref(prm), C.c_void_p(device_ptr), int(n), 1, C.byref(r))
        self.last_rc = rc
        self._check(rc, "tsd_align_points")
        return self._align_dict(r)

    def align_to(self, src, x0, y0, step_xy, nx, ny, ntheta, pivot=None, theta0=0.0, dtheta=0.0, cos_sin=None, theta_wraps=False,
                 K=16, iterations=40, v_cut=0.75, eps=1e-6, lever=0.0, min_overlap=0.0, max_rms=0.0) -> dict:
        """tsd_map_align(self, src): the transform T that carries ``src``'s map coordinates into this grid's (src's surface list,
        replaced by the call, against this grid's TSD).  pivot None: the centre of src's grid.  ``cell_off`` / ``cell_error`` say
        whether a whole-cell shift describes T: ``fuse_begin([.., src], offsets=[.., cell_off])``."""
        prm, tab = self._align_params(x0, y0, step_xy, nx, ny, ntheta, theta0, dtheta, cos_sin, theta_wraps, K, iterations, pivot,
                                      v_cut, eps, lever, min_overlap, max_rms)
        r = AlignResult()
        rc = self.lib.tsd_map_align(self.h, src.h if src is not None else None, C.byref(prm), C.byref(r))
        self.last_rc = rc
        self._check(rc, "tsd_map_align")
        return self._align_dict(r)

    def debug_align_scores(self) -> np.ndarray:
        """TEST HOOK: the score volume of the last alignment, uint32 [nx * ny * ntheta] in candidate order"""
        n = self.lib.tsd_debug_align_scores(self.h, None, 0)
        self._check(min(n, 0), "tsd_debug_align_scores")
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(min(self.lib.tsd_debug_align_scores(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n), 0), "tsd_debug_align_scores")
        return out[:n]

    def debug_align_peaks(self) -> list:
        """TEST HOOK: the per-peak records of the last alignment, in the peaks' order, as dicts (``raw``: the record's bytes)"""
        recs = (AlignPeak * RELOC_MAX_PEAKS)()
        n = self.lib.tsd_debug_align_peaks(self.h, recs, RELOC_MAX_PEAKS)
        self._check(min(n, 0), "tsd_debug_align_peaks")
        return [dict(idx=int(p.idx), score=int(p.score), status=int(p.status), iterations=int(p.iterations), n_ok=int(p.n_ok),
                     m=(p.m[0], p.m[1]), c=p.c, s=p.s, gain=p.gain, sums=np.array(p.sums[:]), raw=bytes(p)) for p in recs[:n]]

    def debug_align_sums(self, points_xy, pivot, m, c, s, v_cut=0.75):
        """TEST HOOK: one accumulation of the refinement kernel at the state (m, c, s): (sums[11], n_ok)"""
        pts = _f64(points_xy).reshape(-1)
        pv, mm, sums, nok = _f64(pivot).reshape(2), _f64(m).reshape(2), np.zeros(11), C.c_int(0)
        rc = self.lib.tsd_debug_align_sums(self.h, _d(pts), pts.size // 2, _d(pv), _d(mm), float(c), float(s), float(v_cut), _d(sums),
                                           C.byref(nok))
        self.last_rc = rc
        self._check(rc, "tsd_debug_align_sums")
        return sums, nok.value

    def set_icp_helpers(self, on: bool):
        """test hook: off = every registration does its first step's searches itself (same results, tsd_debug_set_icp_helpers)"""
        self._check(self.lib.tsd_debug_set_icp_helpers(self.h, 1 if on else 0), "tsd_debug_set_icp_helpers")

    def set_push_multi(self, on: bool):
        """test hook: off = tsd_batch_push enqueues one push per robot instead of one pass per tile (same grid, tsd_debug_set_push_multi)"""
        self._check(self.lib.tsd_debug_set_push_multi(self.h, 1 if on else 0), "tsd_debug_set_push_multi")

    def icp_pairs(self, model_xy, scene_xy, pose, params: IcpParams, calls: int):
        """tsd_icp_pairs: [(model_idx, scene_idx)] of each of the first ``calls`` determinePairs calls on the static scene"""
        m, sc, ps = _f64(model_xy).reshape(-1), _f64(scene_xy).reshape(-1), _f64(pose).reshape(9)
        nm, ns = len(m) // 2, len(sc) // 2
        n = np.zeros(calls, dtype=np.int32)
        mi, si = np.zeros(calls * ns, dtype=np.int32), np.zeros(calls * ns, dtype=np.int32)
        rc = self.lib.tsd_icp_pairs(self.h, _d(m), nm, _d(sc), ns, _d(ps), C.byref(params), calls, n.ctypes.data_as(_ip),
                                    mi.ctypes.data_as(_ip), si.ctypes.data_as(_ip))
        self._check(rc, "tsd_icp_pairs")
        return [(mi[k * ns:k * ns + n[k]].copy(), si[k * ns:k * ns + n[k]].copy()) for k in range(calls)]

    def icp_trace(self, iterations):
        """per iteration: pairs, rms, DistanceFilter threshold before the step, state, Tlast as (c, s, tx, ty)"""
        tr = np.zeros((max(iterations, 1), 8))
        self._check(self.lib.tsd_icp_trace(self.h, _d(tr), iterations), "tsd_icp_trace")
        return tr[:iterations]

    def download_tile_state(self):
        init = np.zeros(self.tiles, dtype=np.uint8)
        iw = np.zeros(self.tiles)
        self._check(self.lib.tsd_download_tile_state(self.h, _u8(init), _d(iw)), "tsd_download_tile_state")
        return init, iw

    def download_tiles(self):
        init = np.zeros(self.tiles, dtype=np.uint8)
        iw = np.zeros(self.tiles)
        tsd = np.zeros((self.tiles, TILE_CELLS))
        w = np.zeros((self.tiles, TILE_CELLS))
        self._check(self.lib.tsd_download_tiles(self.h, _u8(init), _d(iw), _d(tsd), _d(w)), "tsd_download_tiles")
        return init, iw, tsd, w

    def upload_tiles(self, init, iw, tsd, w):
        init = np.ascontiguousarray(init, dtype=np.uint8)
        iw, tsd, w = _f64(iw), _f64(tsd), _f64(w)
        self._check(self.lib.tsd_upload_tiles(self.h, _u8(init), _d(iw), _d(tsd), _d(w)), "tsd_upload_tiles")

    def digest(self) -> dict:
        d = GridDigest()
        self._check(self.lib.tsd_grid_digest(self.h, C.byref(d)), "tsd_grid_digest")
        return d.as_dict()

    def occupancy(self, inflate=False, inflate_factor=2):
        occ = np.zeros(self.cells * self.cells, dtype=np.int8)
        n = C.c_int(0)
        rc = self.lib.tsd_occupancy(self.h, occ.ctypes.data_as(_i8p), int(inflate), inflate_factor, C.byref(n))
        self._check(rc, "tsd_occupancy")
        return occ.reshape(self.cells, self.cells), n.value

    def surface_extract(self, window=None, normals=True) -> int:
        """tsd_surface_extract: builds the surface list on the device and returns its length.  window: (tx0, ty0, tx1, ty1) in tiles,
        half open, clipped to the processed ring; None: the whole grid (with the C call's NULL parameters when normals are wanted)."""
        n = C.c_int(0)
        prm = None
        if window is not None or not normals:
            tx0, ty0, tx1, ty1 = window if window is not None else (0, 0, self.cells // 32, self.cells // 32)
            prm = C.byref(SurfaceParams(int(tx0), int(ty0), int(tx1), int(ty1), 1 if normals else 0, 0))
        self._check(self.lib.tsd_surface_extract(self.h, prm, C.byref(n)), "tsd_surface_extract")
        return n.value

    def surface_fetch(self, first: int, count: int, normals=True):
        """tsd_surface_fetch: points [first, first + count) of the last list as (xy[count, 2], normals[count, 2] or None,
        ok[count] or None)"""
        xy = np.zeros((max(count, 0), 2))
        nr = np.zeros((max(count, 0), 2)) if normals else None
        ok = np.zeros(max(count, 0), dtype=np.uint8) if normals else None
        rc = self.lib.tsd_surface_fetch(self.h, int(first), int(count), _d(xy), _d(nr) if normals else None, _u8(ok) if normals else None)
        self._check(rc, "tsd_surface_fetch")
        return xy, nr, ok

    def surface_points(self, window=None, normals=True):
        """The map's surface as an ordered point list (RayCastAxisAligned2D::calcCoords' coords, tsd_surface_extract + _fetch):
        (xy[n, 2], normals[n, 2] or None, ok[n] or None), the normals being TsdGrid::interpolateNormal at each point and ok[i] = 0
        where it fails (normal (0, 0))."""
        # (through the class: a GridView takes the node's lock once, around this whole method)
        n = TsdGridDevice.surface_extract(self, window, normals)
        return TsdGridDevice.surface_fetch(self, 0, n, normals)

    def surface_dev(self):
        """tsd_surface_dev: (xy, normals, ok) device addresses (0 where there is none) and the length of the last list"""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.lib.tsd_surface_dev(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "tsd_surface_dev")
        return a.value or 0, b.value or 0, c.value or 0, n.value

    def occupancy_into(self, dev_ptr: int, inflate=False, inflate_factor=2):
        self._check(self.lib.tsd_occupancy_dev(self.h, C.c_void_p(dev_ptr), int(inflate), inflate_factor),
                    "tsd_occupancy_dev")

    def measure_stream(self, n_doubles: int, reps: int = 5):
        """(best, mean) GB/s of the RMW stream kernel over two arrays of ``n_doubles`` (tsd_measure_stream)"""
        best, mean = C.c_double(), C.c_double()
        self._check(self.lib.tsd_measure_stream(self.h, n_doubles, reps, C.byref(best), C.byref(mean)), "tsd_measure_stream")
        return best.value, mean.value

    def calibrate_rmw(self, n_doubles: int, reps: int = 3):
        self._check(self.lib.tsd_calibrate_rmw(self.h, n_doubles, reps), "tsd_calibrate_rmw")

    def profile(self, on=True, kernels="all"):
        self.lib.tsd_profile_select(self.h, kernels.encode())
        self.lib.tsd_profile_enable(self.h, int(on))

    def store_text(self, path):
        """TsdGrid::storeGrid: the reference's text format."""
        self._check(self.lib.tsd_store_grid_text(self.h, str(path).encode()), "tsd_store_grid_text")

    def load_text(self, path):
        """TsdGrid(file): replaces the grid's content by a stored file of the same layout."""
        self._check(self.lib.tsd_load_grid_text(self.h, str(path).encode()), "tsd_load_grid_text")

    def color_image(self, width=None, height=None):
        """TsdGrid::grid2ColorImage: (height, width, 3) uint8."""
        width = self.cells if width is None else width
        height = self.cells if height is None else height
        img = np.zeros((height, width, 3), dtype=np.uint8)
        self._check(self.lib.tsd_color_image(self.h, img.ctypes.data_as(_u8p), width, height), "tsd_color_image")
        return img

    def fuse_begin(self, members, offsets=None):
        """tsd_fuse_begin: this grid becomes the TSD-level fusion of ``members`` (grids on the same GPU), member i shifted by
        ``offsets[i]`` = (ox, oy) whole cells (None: all 0).  Returns once the fusion is enqueued."""
        n = len(members)
        hs = (C.c_void_p * max(n, 1))(*[m.h if m is not None else None for m in members])
        off = None
        if offsets is not None:
            flat = [int(v) for o in offsets for v in o]
            assert len(flat) == 2 * n
            off = (C.c_int32 * max(2 * n, 1))(*flat)
        self._check(self.lib.tsd_fuse_begin(self.h, n, hs, off), "tsd_fuse_begin")

    def fuse_wait(self) -> dict:
        """tsd_fuse_wait: blocks until the fusion begun last is done; its counters (tsd_fuse_stats)"""
        st = FuseStats()
        self._check(self.lib.tsd_fuse_wait(self.h, C.byref(st)), "tsd_fuse_wait")
        return st.as_dict()

    def fuse_from(self, members, offsets=None) -> dict:
        """tsd_fuse: fuse_begin + fuse_wait"""
        self.fuse_begin(members, offsets)
        return self.fuse_wait()

    def _pinned(self, name, nbytes):
        """a page-locked host buffer kept by the wrapper (tsd_host_alloc), as a numpy view"""
        bufs = self.__dict__.setdefault("_frame_bufs", {})
        if name not in bufs:
            ptr = self.lib.tsd_host_alloc(nbytes)
            if not ptr:
                raise TsdError(f"tsd_host_alloc({nbytes}) failed")
            bufs[name] = ptr
        return np.ctypeslib.as_array(C.cast(bufs[name], _u8p), shape=(nbytes,))

    def map_frame_begin(self, inflate=False, factor=2, image=True):
        """tsd_map_frame_begin into the wrapper's pinned buffers: returns once the frame is enqueued"""
        n = self.cells * self.cells
        prm = MapParams(int(bool(inflate)), int(factor))
        occ = self._pinned("occ", n)
        rgb = self._pinned("rgb", 3 * n) if image else None
        self._check(self.lib.tsd_map_frame_begin(self.h, C.byref(prm), occ.ctypes.data, None if rgb is None else rgb.ctypes.data),
                    "tsd_map_frame_begin")
        self._frame_image = bool(image)          # (only once begun: a refused begin leaves the frame in flight as it was)

    def map_frame_wait(self):
        """tsd_map_frame_wait: (occ (cells, cells) int8, rgb (cells, cells, 3) uint8 or None, n_surface), copied out of the pinned buffers"""
        ns = C.c_int(0)
        self._check(self.lib.tsd_map_frame_wait(self.h, C.byref(ns)), "tsd_map_frame_wait")
        n = self.cells * self.cells
        occ = self._pinned("occ", n).view(np.int8).reshape(self.cells, self.cells).copy()
        rgb = self._pinned("rgb", 3 * n).reshape(self.cells, self.cells, 3).copy() if self._frame_image else None
        return occ, rgb, ns.value

    def map_frame(self, inflate=False, factor=2, image=True):
        """ThreadGrid's publication in one frame (tsd_map_frame_begin + _wait): (occ, rgb or None, n_surface)"""
        self.map_frame_begin(inflate, factor, image)
        return self.map_frame_wait()

    def map_update_begin(self, inflate=False, factor=2, image=True, occ=None, rgb=None):
        """tsd_map_update_begin: the windowed form of map_frame_begin.  Returns the window (x, y, width, height) in cells once the
        update is enqueued; width 0: nothing changed.  The window's rows and columns are written into the wrapper's pinned buffers --
        the ones map_frame uses, so they always hold the full current frame -- or into ``occ`` (cells, cells) int8 / ``rgb``
        (cells, cells, 3) uint8 where the caller hands in full C-contiguous buffers of its own (which must live until the wait)."""
        n = self.cells * self.cells
        prm = MapParams(int(bool(inflate)), int(factor))
        if occ is None:
            occ = self._pinned("occ", n)
            rgb = self._pinned("rgb", 3 * n) if image else None
        else:
            assert occ.dtype == np.int8 and occ.size == n and occ.flags.c_contiguous
            assert not image or (rgb is not None and rgb.dtype == np.uint8 and rgb.size == 3 * n and rgb.flags.c_contiguous)
            rgb = rgb if image else None
        win = MapWindow()
        self._check(self.lib.tsd_map_update_begin(self.h, C.byref(prm), occ.ctypes.data, None if rgb is None else rgb.ctypes.data,
                                                  C.byref(win)), "tsd_map_update_begin")
        self._update_bufs = (occ, rgb)           # (kept alive until the wait)
        return win.as_tuple()

    def map_update_wait(self):
        """tsd_map_update_wait: (occ, rgb or None, n_surface) -- copies of the full buffers the update was written into, n_surface
        the marks made by the update's tiles"""
        ns = C.c_int(0)
        self._check(self.lib.tsd_map_update_wait(self.h, C.byref(ns)), "tsd_map_update_wait")
        occ, rgb = self._update_bufs
        self._update_bufs = None
        occ = occ.view(np.int8).reshape(self.cells, self.cells).copy()
        rgb = None if rgb is None else rgb.reshape(self.cells, self.cells, 3).copy()
        return occ, rgb, ns.value

    def map_update(self, inflate=False, factor=2, image=True, occ=None, rgb=None):
        """tsd_map_update_begin + _wait: (window, occ, rgb or None, n_surface)"""
        win = self.map_update_begin(inflate, factor, image, occ, rgb)
        o, r, ns = self.map_update_wait()
        return win, o, r, ns

    # ---- clearance field and cost map (tsd_costmap_table, tsd_clearance_dev, tsd_costmap_begin / _wait)
    def costmap_table(self, radius, inscribed_radius_m=0.25, cost_scaling=10.0) -> np.ndarray:
        """tsd_costmap_table at this grid's cell size: int8 [radius^2 + 1]"""
        return costmap_table(self.cell_size, radius, inscribed_radius_m, cost_scaling)

    def set_clearance_skip(self, on: bool):
        """test hook: off = every workgroup of the column pass walks its rows (same bytes, tsd_debug_set_clearance_skip)"""
        self._check(self.lib.tsd_debug_set_clearance_skip(self.h, 1 if on else 0), "tsd_debug_set_clearance_skip")

    def _dev_out(self, name, nbytes):
        """a device buffer kept by the wrapper for clearance_of's outputs (replaced when a larger one is asked for)"""
        bufs = self.__dict__.setdefault("_dev_bufs", {})
        if name not in bufs or bufs[name].nbytes < nbytes:
            if name in bufs:
                bufs[name].free()
            bufs[name] = DeviceBuffer(self, nbytes)
        return bufs[name]

    def clearance_of(self, dev_ptr: int, width: int, height: int, stride: int, radius: int, window=None, table=None, prefill=None):
        """tsd_clearance_dev on a device map (``dev_ptr``: int8, ``height`` rows of ``stride`` bytes): (dist2 (height, width)
        uint16, cost (height, width) int8 or None without a ``table``), copied to the host.  window: (x, y, width, height), None: the
        whole map; only its cells are written.  prefill: (uint16, int8) values the outputs hold before the call (default 0)."""
        n = int(width) * int(height)
        d_d2 = self._dev_out("dist2", 2 * n)
        d_cost = self._dev_out("cost", n) if table is not None else None
        p2, pc = prefill if prefill is not None else (0, 0)
        d_d2.upload(np.full(n, p2, dtype=np.uint16))
        if d_cost is not None:
            d_cost.upload(np.full(n, pc, dtype=np.int8))
        tab = None if table is None else np.ascontiguousarray(table, dtype=np.int8)
        assert tab is None or tab.size == int(radius) * int(radius) + 1
        win = None if window is None else C.byref(MapWindow(*[int(v) for v in window]))
        rc = self.lib.tsd_clearance_dev(self.h, C.c_void_p(dev_ptr), int(width), int(height), int(stride), win, int(radius),
                                        None if tab is None else tab.ctypes.data_as(_i8p), C.c_void_p(d_d2.ptr),
                                        None if d_cost is None else C.c_void_p(d_cost.ptr))
        self.last_rc = rc
        self._check(rc, "tsd_clearance_dev")
        d2 = d_d2.download(np.uint16, n).reshape(height, width)
        cost = None if d_cost is None else d_cost.download(np.int8, n).reshape(height, width)
        return d2, cost

    def costmap_begin(self, radius, inscribed_radius_m=0.25, cost_scaling=10.0, map_win=None, want_dist2=False, cost=None, dist2=None):
        """tsd_costmap_begin: the cost map of the frame or update taken last, recomputed in ``map_win`` (x, y, width, height; None:
        the whole map) grown by ``radius`` and clipped -- the window returned.  Written into the wrapper's pinned buffers, which always
        hold the full current cost map, or into ``cost`` (cells, cells) int8 / ``dist2`` (cells, cells) uint16 where the caller hands
        in full C-contiguous buffers of its own (which must live until the wait)."""
        n = self.cells * self.cells
        if cost is None:
            cost = self._pinned("cost", n)
            dist2 = self._pinned("dist2", 2 * n) if want_dist2 else None
        else:
            assert cost.dtype == np.int8 and cost.size == n and cost.flags.c_contiguous
            assert not want_dist2 or (dist2 is not None and dist2.dtype == np.uint16 and dist2.size == n and dist2.flags.c_contiguous)
            dist2 = dist2 if want_dist2 else None
        prm = CostmapParams(int(radius), int(bool(want_dist2)), float(inscribed_radius_m), float(cost_scaling))
        mw = None if map_win is None else C.byref(MapWindow(*[int(v) for v in map_win]))
        out = MapWindow()
        rc = self.lib.tsd_costmap_begin(self.h, C.byref(prm), cost.ctypes.data, None if dist2 is None else dist2.ctypes.data, mw,
                                        C.byref(out))
        self.last_rc = rc
        self._check(rc, "tsd_costmap_begin")
        self._costmap_bufs = (cost, dist2)       # (kept alive until the wait)
        return out.as_tuple()

    def costmap_wait(self):
        """tsd_costmap_wait: (cost (cells, cells) int8, dist2 (cells, cells) uint16 or None) -- copies of the full buffers"""
        self._check(self.lib.tsd_costmap_wait(self.h), "tsd_costmap_wait")
        cost, dist2 = self._costmap_bufs
        self._costmap_bufs = None
        cost = cost.view(np.int8).reshape(self.cells, self.cells).copy()
        dist2 = None if dist2 is None else dist2.view(np.uint16).reshape(self.cells, self.cells).copy()
        return cost, dist2

    def costmap(self, radius, inscribed_radius_m=0.25, cost_scaling=10.0, map_win=None, want_dist2=False, cost=None, dist2=None):
        """tsd_costmap_begin + _wait: (window, cost, dist2 or None)"""
        win = self.costmap_begin(radius, inscribed_radius_m, cost_scaling, map_win, want_dist2, cost, dist2)
        c, d = self.costmap_wait()
        return win, c, d

    def clearance(self, radius) -> np.ndarray:
        """Distance of every cell of the frame taken last to the nearest occupied cell, metres as float32 (cells, cells):
        sqrt(d2) * cell_size, inf beyond ``radius`` cells"""
        _, _, d2 = self.costmap(radius, want_dist2=True)
        out = (np.sqrt(d2.astype(np.float64)) * self.cell_size).astype(np.float32)
        out[d2 == DIST2_NONE] = np.inf
        return out

    # ---- frontiers (tsd_frontiers_dev / _frame / _fetch / _dev_ptrs)
    @staticmethod
    def _frontier_params(free_max, min_size, seeds):
        """(tsd_frontier_params, the seed array it points into -- to be kept alive over the call)"""
        xy = np.ascontiguousarray(np.asarray(list(seeds), dtype=np.int32).reshape(-1, 2))
        prm = FrontierParams(int(free_max), int(min_size), int(xy.shape[0]), 0,
                             xy.ctypes.data_as(C.POINTER(C.c_int32)) if xy.shape[0] else None)
        return prm, xy

    def _frontier_result(self, n, width, height):
        rec = np.zeros(n, dtype=FRONTIER_DTYPE)
        self._check(self.lib.tsd_frontiers_fetch(self.h, 0, n, rec.ctypes.data), "tsd_frontiers_fetch")
        _, labels_dev, n2 = self.frontiers_dev_ptrs()
        assert n2 == n
        labels = np.zeros((int(height), int(width)), dtype=np.uint32)
        self._check(self.lib.tsd_dev_copy(self.h, labels.ctypes.data, labels_dev, labels.nbytes, 0), "tsd_dev_copy")
        return rec, labels

    def frontiers_dev_ptrs(self):
        """tsd_frontiers_dev_ptrs: (records_dev, labels_dev, n) of the last frontier call, valid until the next one"""
        r, l, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.lib.tsd_frontiers_dev_ptrs(self.h, C.byref(r), C.byref(l), C.byref(n)), "tsd_frontiers_dev_ptrs")
        return r.value, l.value, n.value

    def frontiers_counts(self):
        """tsd_frontiers_counts: (frontiers before min_size, seam unions of the frontiers' labels, of the regions' labels)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.tsd_frontiers_counts(self.h, C.byref(a), C.byref(b), C.byref(c)), "tsd_frontiers_counts")
        return a.value, b.value, c.value

    def frontiers_of(self, dev_ptr: int, width: int, height: int, stride: int, free_max=0, min_size=1, seeds=()):
        """tsd_frontiers_dev on a device map (``dev_ptr``: int8, ``height`` rows of ``stride`` bytes): (records as a structured
        array of FRONTIER_DTYPE in ascending root index, labels (height, width) uint32, seeds_used).  seeds: (x, y) cells."""
        prm, xy = self._frontier_params(free_max, min_size, seeds)
        n, used = C.c_int(0), C.c_int(0)
        rc = self.lib.tsd_frontiers_dev(self.h, C.c_void_p(dev_ptr), int(width), int(height), int(stride), C.byref(prm),
                                        C.byref(n), C.byref(used))
        self.last_rc = rc
        self._check(rc, "tsd_frontiers_dev")
        rec, labels = self._frontier_result(n.value, width, height)
        return rec, labels, used.value

    def frontiers(self, free_max=0, min_size=1, seeds=()):
        """tsd_frontiers_frame: the same for the map of the frame or update taken last (cells x cells)"""
        prm, xy = self._frontier_params(free_max, min_size, seeds)
        n, used = C.c_int(0), C.c_int(0)
        rc = self.lib.tsd_frontiers_frame(self.h, C.byref(prm), C.byref(n), C.byref(used))
        self.last_rc = rc
        self._check(rc, "tsd_frontiers_frame")
        rec, labels = self._frontier_result(n.value, self.cells, self.cells)
        return rec, labels, used.value

    # ---- routes (tsd_route_dev / _frame / _goals / _trace / _dev_ptrs)
    @staticmethod
    def route_weights(free_max=0, max_weight=1) -> np.ndarray:
        """tsd_route_weights: uint8 W[0 .. free_max]"""
        return route_weights(free_max, max_weight)

    @staticmethod
    def _route_params(seeds, free_max, weights, limit, max_rounds):
        """(tsd_route_params, the arrays it points into -- to be kept alive over the call)"""
        xy = np.ascontiguousarray(np.asarray(list(seeds), dtype=np.int32).reshape(-1, 2))
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint8)
        assert w is None or w.size == int(free_max) + 1
        prm = RouteParams(int(free_max), int(xy.shape[0]), xy.ctypes.data_as(C.POINTER(C.c_int32)) if xy.shape[0] else None,
                          None if w is None else w.ctypes.data_as(_u8p), int(limit), int(max_rounds))
        return prm, (xy, w)

    def set_route_sweeps(self, n: int):
        """test hook: the sweeps a tile makes per launch (tsd_debug_set_route_sweeps; 0: the default; same bytes at any value)"""
        self._check(self.lib.tsd_debug_set_route_sweeps(self.h, int(n)), "tsd_debug_set_route_sweeps")

    def route_dev_ptrs(self):
        """tsd_route_dev_ptrs: (keys_dev, width, height) of the last route call, valid until the next one"""
        k, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
        self._check(self.lib.tsd_route_dev_ptrs(self.h, C.byref(k), C.byref(w), C.byref(h)), "tsd_route_dev_ptrs")
        return k.value, w.value, h.value

    def route_counts(self):
        """tsd_route_counts: (workgroups that found their tile active over all rounds, host waits) of the last route call"""
        v, w = C.c_longlong(0), C.c_int(0)
        self._check(self.lib.tsd_route_counts(self.h, C.byref(v), C.byref(w)), "tsd_route_counts")
        return v.value, w.value

    def route_keys(self) -> np.ndarray:
        """the key image of the last route call, (height, width) uint32, copied to the host"""
        keys_dev, w, h = self.route_dev_ptrs()
        keys = np.zeros((h, w), dtype=np.uint32)
        self._check(self.lib.tsd_dev_copy(self.h, keys.ctypes.data, keys_dev, keys.nbytes, 0), "tsd_dev_copy")
        return keys

    def route_of(self, dev_ptr: int, width: int, height: int, stride: int, seeds, free_max=0, weights=None, limit=0, max_rounds=0):
        """tsd_route_dev on a device map (``dev_ptr``: int8, ``height`` rows of ``stride`` bytes): (keys (height, width) uint32 --
        (d << 4) | seed index, ROUTE_NONE without a path within the limit --, info as a dict).  seeds: (x, y) cells."""
        prm, keep = self._route_params(seeds, free_max, weights, limit, max_rounds)
        info = RouteInfo()
        rc = self.lib.tsd_route_dev(self.h, C.c_void_p(dev_ptr), int(width), int(height), int(stride), C.byref(prm), C.byref(info))
        self.last_rc = rc
        self._check(rc, "tsd_route_dev")
        return self.route_keys(), info.as_dict()

    def route(self, source="map", seeds=(), free_max=0, weights=None, limit=0, max_rounds=0):
        """tsd_route_frame: the same for the map ("map") of the frame or update taken last or for the cost map ("costmap") made of
        it last (cells x cells)"""
        prm, keep = self._route_params(seeds, free_max, weights, limit, max_rounds)
        info = RouteInfo()
        rc = self.lib.tsd_route_frame(self.h, ROUTE_SOURCES[source], C.byref(prm), C.byref(info))
        self.last_rc = rc
        self._check(rc, "tsd_route_frame")
        return self.route_keys(), info.as_dict()

    def route_goals(self) -> np.ndarray:
        """tsd_route_goals + _fetch: for every record of the frontier call made last the cheapest cell to reach on the key image of
        the route call made last, as a structured array of ROUTE_GOAL_DTYPE (cell, dist, seed)"""
        n = C.c_int(0)
        rc = self.lib.tsd_route_goals(self.h, C.byref(n))
        self.last_rc = rc
        self._check(rc, "tsd_route_goals")
        out = np.zeros(n.value, dtype=ROUTE_GOAL_DTYPE)
        self._check(self.lib.tsd_route_goals_fetch(self.h, 0, n.value, out.ctypes.data), "tsd_route_goals_fetch")
        return out

    def route_paths(self, cells, max_len=4096):
        """tsd_route_trace: (paths -- one uint32 array of linear cell indices per goal cell, goal first and seed last, cut at
        ``max_len`` --, lengths int32: the full length, 0 without a key, -1 where the image did not converge)"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        paths = np.zeros((cells.size, int(max_len)), dtype=np.uint32)
        lens = np.zeros(cells.size, dtype=np.int32)
        rc = self.lib.tsd_route_trace(self.h, cells.ctypes.data, int(cells.size), int(max_len), paths.ctypes.data, lens.ctypes.data)
        self.last_rc = rc
        self._check(rc, "tsd_route_trace")
        return [paths[g, :min(max(int(n), 0), int(max_len))].copy() for g, n in enumerate(lens)], lens

    def route_waypoints(self, cells, lookahead=128, slack=0, max_len=4096, max_way=256):
        """tsd_route_waypoints: (waypoints -- one uint32 array of linear cell indices per goal cell, SEED FIRST and goal last (the
        opposite of route_paths), consecutive cells joined by a straight drivable segment that spans at most ``lookahead`` path cells
        and costs at most the field's difference plus ``slack``, cut at ``max_way`` --, info as a structured array of
        WAYPOINT_INFO_DTYPE: len as route_paths gives it, n_way the full count (0 where the path is longer than ``max_len``), the
        segments' cost, the goal's dist)"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        way = np.zeros((cells.size, max(int(max_way), 1)), dtype=np.uint32)
        info = np.zeros(cells.size, dtype=WAYPOINT_INFO_DTYPE)
        prm = WaypointParams(int(lookahead), int(slack), int(max_len), int(max_way))
        rc = self.lib.tsd_route_waypoints(self.h, cells.ctypes.data, int(cells.size), C.byref(prm), way.ctypes.data, info.ctypes.data)
        self.last_rc = rc
        self._check(rc, "tsd_route_waypoints")
        return [way[g, :min(max(int(n), 0), int(max_way))].copy() for g, n in enumerate(info["n_way"])], info

    # ---- drive (tsd_drive_*): the next step's velocity from arcs rolled out on a route or fields result
    @staticmethod
    def drive_table() -> np.ndarray:
        """tsd_drive_table: int32 (DRIVE_HEADINGS, 2)"""
        return drive_table()

    @staticmethod
    def drive_advance(pose, step_q16: int, turn: int, n_steps: int = 1) -> np.ndarray:
        """tsd_drive_advance: the pose after ``n_steps`` steps"""
        return drive_advance(pose, step_q16, turn, n_steps)

    def drive_dev_ptrs(self):
        """tsd_drive_dev_ptrs: (the drive block on the device, its capacity in 32-bit words); the table is its first 8192 words"""
        b, n = C.c_void_p(), C.c_ulonglong(0)
        self._check(self.lib.tsd_drive_dev_ptrs(self.h, C.byref(b), C.byref(n)), "tsd_drive_dev_ptrs")
        return b.value, n.value

    @staticmethod
    def _drive_params(steps, step_q16, turn, body, weights, nose_q16, nose_miss):
        """(tsd_drive_params, the arrays it points into -- to be kept alive over the call)"""
        s = np.ascontiguousarray(step_q16, dtype=np.int32).ravel()
        t = np.ascontiguousarray(turn, dtype=np.int32).ravel()
        b = np.zeros((0, 2), dtype=np.int32) if body is None else np.ascontiguousarray(body, dtype=np.int32).reshape(-1, 2)
        p32 = C.POINTER(C.c_int32)
        prm = DriveParams(int(steps), int(s.size), int(t.size), int(b.shape[0]), s.ctypes.data_as(p32), t.ctypes.data_as(p32),
                          b.ctypes.data_as(p32) if b.shape[0] else None, *[int(w) for w in weights], int(nose_q16), int(nose_miss))
        return prm, (s, t, b)

    def _drive(self, fn, name, poses, steps, step_q16, turn, body, weights, nose_q16, nose_miss, want_scores):
        prm, keep = self._drive_params(steps, step_q16, turn, body, weights, nose_q16, nose_miss)
        p = drive_poses(poses)
        n = prm.n_speeds * prm.n_turns
        choice = np.zeros(p.size, dtype=DRIVE_CHOICE_DTYPE)
        scores = np.zeros((p.size, prm.n_speeds, prm.n_turns), dtype=np.uint64) if want_scores else None
        why = np.zeros((p.size, prm.n_speeds, prm.n_turns), dtype=np.uint16) if want_scores else None
        rc = fn(self.h, C.byref(prm), p.ctypes.data, int(p.size), choice.ctypes.data, scores.ctypes.data if want_scores else None,
                why.ctypes.data if want_scores else None)
        self.last_rc = rc
        self._check(rc, name)
        return (choice, scores, why) if want_scores else choice

    def drive_rollout(self, poses, steps, step_q16, turn, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0, want_scores=False):
        """tsd_drive_rollout on the route result the context holds: per pose (x, y, fx, fy, heading) the best of the
        len(step_q16) x len(turn) arcs of ``steps`` steps, as a structured array of DRIVE_CHOICE_DTYPE (speed and turn: indices into
        the lists, -1 without an admissible arc).  weights: (a_end, a_nose, a_cost, a_turn); body: (bx, by) pairs in Q16 cells.
        want_scores: (choice, scores uint64 (n, V, Wn) -- DRIVE_NONE where refused --, why uint16 (n, V, Wn))."""
        return self._drive(self.lib.tsd_drive_rollout, "tsd_drive_rollout", poses, steps, step_q16, turn, body, weights, nose_q16, nose_miss,
                           want_scores)

    def drive_fields_rollout(self, poses, steps, step_q16, turn, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0,
                             want_scores=False):
        """tsd_drive_fields_rollout: the same on the fields result, pose r (x, y, fx, fy, heading, layer) on its layer's keys"""
        return self._drive(self.lib.tsd_drive_fields_rollout, "tsd_drive_fields_rollout", poses, steps, step_q16, turn, body, weights,
                           nose_q16, nose_miss, want_scores)

    def drive_fleet_rollout(self, poses, steps, step_q16, turn, order, sep_q16, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0,
                            want_scores=False, want_tracks=False):
        """tsd_drive_fleet_rollout: tsd_drive_fields_rollout with the robots deciding in the order ``order`` (a permutation of their
        indices, order[0] first), each against the arcs chosen before it: an arc that comes within ``sep_q16`` (Q16 cells, centre to
        centre) of one of them without moving away from it is refused by reason 6.  A pose with layer -1 is a parked robot.  Returns
        the choices, then (scores, why) with want_scores, then tracks int64 (n, steps + 1, 2) -- the absolute Q16 positions of each
        robot's chosen arc, its pose in every slot without one -- with want_tracks."""
        prm, keep = self._drive_params(steps, step_q16, turn, body, weights, nose_q16, nose_miss)
        p = drive_poses(poses)
        o = np.ascontiguousarray(order, dtype=np.int32).ravel()
        if o.size != p.size:
            raise TsdError(f"tsd_drive_fleet_rollout: {o.size} ranks for {p.size} robots")
        fleet = DriveFleetParams(o.ctypes.data_as(C.POINTER(C.c_int32)), int(sep_q16), 0)
        choice = np.zeros(p.size, dtype=DRIVE_CHOICE_DTYPE)
        scores = np.zeros((p.size, prm.n_speeds, prm.n_turns), dtype=np.uint64) if want_scores else None
        why = np.zeros((p.size, prm.n_speeds, prm.n_turns), dtype=np.uint16) if want_scores else None
        tracks = np.zeros((p.size, int(steps) + 1, 2), dtype=np.int64) if want_tracks else None
        rc = self.lib.tsd_drive_fleet_rollout(self.h, C.byref(prm), C.byref(fleet), p.ctypes.data, int(p.size), choice.ctypes.data,
                                              scores.ctypes.data if want_scores else None, why.ctypes.data if want_scores else None,
                                              tracks.ctypes.data if want_tracks else None)
        self.last_rc = rc
        self._check(rc, "tsd_drive_fleet_rollout")
        out = (choice,) + ((scores, why) if want_scores else ()) + ((tracks,) if want_tracks else ())
        return out if len(out) > 1 else choice

    def drive_fields_togo(self, poses) -> np.ndarray:
        """tsd_drive_fields_togo: uint32 per pose, the key of its layer of the fields result at its cell (ROUTE_NONE without one and
        for a parked robot, layer -1) -- what a priority by cost-to-go sorts by"""
        p = drive_poses(poses)
        togo = np.zeros(p.size, dtype=np.uint32)
        self._check(self.lib.tsd_drive_fields_togo(self.h, p.ctypes.data, int(p.size), togo.ctypes.data), "tsd_drive_fields_togo")
        return togo

    # ---- the live layer (tsd_drive_live_*): the current scans' end points, kept off the arcs of the three rollouts
    def drive_live_set(self, points_cells, radius: int, skip=None, size=None) -> int:
        """tsd_drive_live_set: the layer of the int32 (n, 2) map cells ``points_cells`` (they may lie outside the map), each a disc of
        ``radius`` cells; ``skip``: up to 16 discs (ox, oy, ro) whose points are dropped -- the robots themselves; ``size``: (width,
        height), by default the image of the route result, else of the fields result.  Returns the number of points not dropped.
        While the layer is set the rollouts refuse every arc that enters it (reason 7)."""
        pts = np.ascontiguousarray(points_cells if points_cells is not None else [], dtype=np.int32).reshape(-1, 2)
        sk = np.ascontiguousarray(skip if skip is not None else [], dtype=np.int32).reshape(-1, 3)
        if size is None:
            k, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
            if self.lib.tsd_route_dev_ptrs(self.h, C.byref(k), C.byref(w), C.byref(h)) != 0:
                w, h = (C.c_int(v) for v in self.route_fields_dev_ptrs()[1:3])
            size = (w.value, h.value)
        prm = DriveLiveParams(int(radius), int(sk.shape[0]), sk.ctypes.data_as(C.POINTER(C.c_int32)) if sk.shape[0] else None)
        kept = C.c_int(-1)
        rc = self.lib.tsd_drive_live_set(self.h, C.byref(prm), pts.ctypes.data if pts.shape[0] else None, int(pts.shape[0]), int(size[0]),
                                         int(size[1]), C.byref(kept))
        self.last_rc = rc
        self._check(rc, "tsd_drive_live_set")
        return kept.value

    def drive_live_clear(self) -> None:
        """tsd_drive_live_clear: no layer -- the rollouts are those without one again"""
        self._check(self.lib.tsd_drive_live_clear(self.h), "tsd_drive_live_clear")

    def drive_live(self):
        """the layer as a bool (height, width) image (tsd_drive_live_fetch, unpacked), None where none is set"""
        w, h, s = C.c_int(0), C.c_int(0), C.c_int(0)
        if self.lib.tsd_drive_live_dev_ptr(self.h, None, C.byref(w), C.byref(h), C.byref(s)) != 0:
            return None
        words = np.zeros((h.value, s.value), dtype="<u4")
        self._check(self.lib.tsd_drive_live_fetch(self.h, words.ctypes.data, words.size, None, None, None), "tsd_drive_live_fetch")
        return np.unpackbits(words.view(np.uint8).reshape(h.value, -1), axis=1, bitorder="little")[:, :w.value].astype(bool)

    # ---- fields (tsd_route_fields_*): one key image per seed
    def route_fields_dev_ptrs(self):
        """tsd_route_fields_dev_ptrs: (keys_dev, width, height, layers) of the last fields call, valid until the next one; layer r
        lies at keys_dev + 4 * r * width * height"""
        k, w, h, l = C.c_void_p(), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.tsd_route_fields_dev_ptrs(self.h, C.byref(k), C.byref(w), C.byref(h), C.byref(l)), "tsd_route_fields_dev_ptrs")
        return k.value, w.value, h.value, l.value

    def route_fields_counts(self):
        """tsd_route_fields_counts: (workgroups that found their tile active over all rounds and layers, host waits)"""
        v, w = C.c_longlong(0), C.c_int(0)
        self._check(self.lib.tsd_route_fields_counts(self.h, C.byref(v), C.byref(w)), "tsd_route_fields_counts")
        return v.value, w.value

    def route_fields_keys(self) -> np.ndarray:
        """the key images of the last fields call, (layers, height, width) uint32, copied to the host"""
        keys_dev, w, h, l = self.route_fields_dev_ptrs()
        keys = np.zeros((l, h, w), dtype=np.uint32)
        self._check(self.lib.tsd_dev_copy(self.h, keys.ctypes.data, keys_dev, keys.nbytes, 0), "tsd_dev_copy")
        return keys

    def route_fields_of(self, dev_ptr: int, width: int, height: int, stride: int, seeds, free_max=0, weights=None, limit=0, max_rounds=0):
        """tsd_route_fields_dev on a device map: (keys (L, height, width) uint32 -- layer r the field of seed r alone, its index in
        the low four bits --, info as a dict with used[] and reached[] per layer).  seeds: (x, y) cells, L of them."""
        prm, keep = self._route_params(seeds, free_max, weights, limit, max_rounds)
        info = RouteFieldsInfo()
        rc = self.lib.tsd_route_fields_dev(self.h, C.c_void_p(dev_ptr), int(width), int(height), int(stride), C.byref(prm), C.byref(info))
        self.last_rc = rc
        self._check(rc, "tsd_route_fields_dev")
        return self.route_fields_keys(), info.as_dict()

    def route_fields(self, source="map", seeds=(), free_max=0, weights=None, limit=0, max_rounds=0):
        """tsd_route_fields_frame: the same for the map ("map") of the frame or update taken last or for the cost map ("costmap")"""
        prm, keep = self._route_params(seeds, free_max, weights, limit, max_rounds)
        info = RouteFieldsInfo()
        rc = self.lib.tsd_route_fields_frame(self.h, ROUTE_SOURCES[source], C.byref(prm), C.byref(info))
        self.last_rc = rc
        self._check(rc, "tsd_route_fields_frame")
        return self.route_fields_keys(), info.as_dict()

    def route_fields_goals(self) -> np.ndarray:
        """tsd_route_fields_goals + _fetch: the goal matrix (L, n) of ROUTE_GOAL_DTYPE -- row r: for every record of the frontier
        call made last robot r's cheapest cell of it on layer r of the fields call made last"""
        n = C.c_int(0)
        rc = self.lib.tsd_route_fields_goals(self.h, C.byref(n))
        self.last_rc = rc
        self._check(rc, "tsd_route_fields_goals")
        layers = self.route_fields_dev_ptrs()[3]
        out = np.zeros((layers, n.value), dtype=ROUTE_GOAL_DTYPE)
        for r in range(layers):
            self._check(self.lib.tsd_route_fields_goals_fetch(self.h, r, 0, n.value, out[r].ctypes.data), "tsd_route_fields_goals_fetch")
        return out

    def route_fields_paths(self, cells, layers, max_len=4096):
        """tsd_route_fields_trace: route_paths with a layer per goal cell"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        layers = np.ascontiguousarray(layers, dtype=np.uint8).ravel()
        assert layers.size == cells.size
        paths = np.zeros((cells.size, int(max_len)), dtype=np.uint32)
        lens = np.zeros(cells.size, dtype=np.int32)
        rc = self.lib.tsd_route_fields_trace(self.h, cells.ctypes.data, layers.ctypes.data, int(cells.size), int(max_len), paths.ctypes.data,
                                             lens.ctypes.data)
        self.last_rc = rc
        self._check(rc, "tsd_route_fields_trace")
        return [paths[g, :min(max(int(n), 0), int(max_len))].copy() for g, n in enumerate(lens)], lens

    def route_fields_waypoints(self, cells, layers, lookahead=128, slack=0, max_len=4096, max_way=256):
        """tsd_route_fields_waypoints: route_waypoints with a layer per goal cell"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        layers = np.ascontiguousarray(layers, dtype=np.uint8).ravel()
        assert layers.size == cells.size
        way = np.zeros((cells.size, max(int(max_way), 1)), dtype=np.uint32)
        info = np.zeros(cells.size, dtype=WAYPOINT_INFO_DTYPE)
        prm = WaypointParams(int(lookahead), int(slack), int(max_len), int(max_way))
        rc = self.lib.tsd_route_fields_waypoints(self.h, cells.ctypes.data, layers.ctypes.data, int(cells.size), C.byref(prm), way.ctypes.data,
                                                 info.ctypes.data)
        self.last_rc = rc
        self._check(rc, "tsd_route_fields_waypoints")
        return [way[g, :min(max(int(n), 0), int(max_way))].copy() for g, n in enumerate(info["n_way"])], info

    # ---- views (tsd_view_gains / _claim / _claims_reset / _claims_dev_ptr / _assign / _assign_fields)
    def view_gains_of(self, dev_ptr, width: int, height: int, stride: int, cells, radius: int, free_max=0, unknown_depth=0,
                      use_claims=False) -> np.ndarray:
        """tsd_view_gains on a device map (``dev_ptr``: int8, ``height`` rows of ``stride`` bytes; None: the staged map of the frame
        or update taken last): for every candidate cell (linear index) what a scanner there would see within ``radius`` cells, as a
        structured array of VIEW_GAIN_DTYPE (cell, gain, unknown, visible)"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        out = np.zeros(cells.size, dtype=VIEW_GAIN_DTYPE)
        prm = ViewParams(int(free_max), int(radius), int(unknown_depth), int(bool(use_claims)))
        rc = self.lib.tsd_view_gains(self.h, None if dev_ptr is None else C.c_void_p(dev_ptr), int(width), int(height), int(stride),
                                     C.byref(prm), cells.ctypes.data, int(cells.size), out.ctypes.data)
        self.last_rc = rc
        self._check(rc, "tsd_view_gains")
        return out

    def view_gains(self, cells, radius: int, free_max=0, unknown_depth=0, use_claims=False) -> np.ndarray:
        """the same for the map of the frame or update taken last (cells x cells)"""
        return self.view_gains_of(None, 0, 0, 0, cells, radius, free_max, unknown_depth, use_claims)

    def view_claim_of(self, dev_ptr, width: int, height: int, stride: int, cells, radius: int, free_max=0, unknown_depth=0):
        """tsd_view_claim: marks the unknown cells every candidate would see in the context's claims image (view_claims_reset first)"""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
        prm = ViewParams(int(free_max), int(radius), int(unknown_depth), 0)
        rc = self.lib.tsd_view_claim(self.h, None if dev_ptr is None else C.c_void_p(dev_ptr), int(width), int(height), int(stride),
                                     C.byref(prm), cells.ctypes.data, int(cells.size))
        self.last_rc = rc
        self._check(rc, "tsd_view_claim")

    def view_claim(self, cells, radius: int, free_max=0, unknown_depth=0):
        """the same for the map of the frame or update taken last"""
        self.view_claim_of(None, 0, 0, 0, cells, radius, free_max, unknown_depth)

    def view_claims_reset(self, width: int, height: int):
        """tsd_view_claims_reset: the claims image at width x height, all 0"""
        rc = self.lib.tsd_view_claims_reset(self.h, int(width), int(height))
        self.last_rc = rc
        self._check(rc, "tsd_view_claims_reset")

    def view_claims_dev_ptr(self):
        """tsd_view_claims_dev_ptr: (claims_dev, width, height)"""
        p, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
        self._check(self.lib.tsd_view_claims_dev_ptr(self.h, C.byref(p), C.byref(w), C.byref(h)), "tsd_view_claims_dev_ptr")
        return p.value, w.value, h.value

    def view_claims(self) -> np.ndarray:
        """the claims image, (height, width) uint8, copied to the host"""
        p, w, h = self.view_claims_dev_ptr()
        img = np.zeros((h, w), dtype=np.uint8)
        self._check(self.lib.tsd_dev_copy(self.h, img.ctypes.data, p, img.nbytes, 0), "tsd_dev_copy")
        return img

    def view_assign_of(self, dev_ptr, width: int, height: int, stride: int, goals, n_robots: int, radius: int, gain_weight: int,
                       free_max=0, unknown_depth=0):
        """tsd_view_assign on the goals of a route plan (ROUTE_GOAL_DTYPE): (goal_of_robot int32[n_robots] -- the index of the goal
        each robot is given, -1 for none --, the picked goals' records as their rounds saw them, the rounds)"""
        goals = np.ascontiguousarray(goals, dtype=ROUTE_GOAL_DTYPE).ravel()
        goal_of = np.full(int(n_robots), -7, dtype=np.int32)
        picked = np.zeros(int(n_robots), dtype=VIEW_GAIN_DTYPE)
        rounds = C.c_int(-1)
        prm = ViewParams(int(free_max), int(radius), int(unknown_depth), 0)
        rc = self.lib.tsd_view_assign(self.h, None if dev_ptr is None else C.c_void_p(dev_ptr), int(width), int(height), int(stride),
                                      C.byref(prm), goals.ctypes.data if goals.size else None, int(goals.size), int(n_robots),
                                      int(gain_weight), goal_of.ctypes.data, picked.ctypes.data, C.byref(rounds))
        self.last_rc = rc
        self._check(rc, "tsd_view_assign")
        return goal_of, picked, rounds.value

    def view_assign(self, goals, n_robots: int, radius: int, gain_weight: int, free_max=0, unknown_depth=0):
        """the same for the map of the frame or update taken last"""
        return self.view_assign_of(None, 0, 0, 0, goals, n_robots, radius, gain_weight, free_max, unknown_depth)

    def view_assign_fields_of(self, dev_ptr, width: int, height: int, stride: int, goals, radius: int, gain_weight: int, free_max=0,
                              unknown_depth=0):
        """tsd_view_assign_fields on the goal matrix of a fields plan (ROUTE_GOAL_DTYPE, shape (n_robots, n_frontiers)):
        (goal_of_robot int32[n_robots] -- the frontier index each robot is given, -1 for none --, the picked cells' records as their
        rounds saw them, the rounds)"""
        goals = np.ascontiguousarray(goals, dtype=ROUTE_GOAL_DTYPE)
        assert goals.ndim == 2
        n_robots, n_frontiers = goals.shape
        goal_of = np.full(n_robots, -7, dtype=np.int32)
        picked = np.zeros(n_robots, dtype=VIEW_GAIN_DTYPE)
        rounds = C.c_int(-1)
        prm = ViewParams(int(free_max), int(radius), int(unknown_depth), 0)
        rc = self.lib.tsd_view_assign_fields(self.h, None if dev_ptr is None else C.c_void_p(dev_ptr), int(width), int(height), int(stride),
                                             C.byref(prm), goals.ctypes.data if goals.size else None, int(n_frontiers), int(n_robots),
                                             int(gain_weight), goal_of.ctypes.data, picked.ctypes.data, C.byref(rounds))
        self.last_rc = rc
        self._check(rc, "tsd_view_assign_fields")
        return goal_of, picked, rounds.value

    def view_assign_fields(self, goals, radius: int, gain_weight: int, free_max=0, unknown_depth=0):
        """the same for the map of the frame or update taken last"""
        return self.view_assign_fields_of(None, 0, 0, 0, goals, radius, gain_weight, free_max, unknown_depth)

    def push_stats_total(self, reset=False):
        st = PushStats()
        n = C.c_int64(0)
        self._check(self.lib.tsd_push_stats_total(self.h, C.byref(st), C.byref(n), int(reset)), "tsd_push_stats_total")
        return st.as_dict(), n.value

    def profile_reset(self):
        self.lib.tsd_profile_reset(self.h)

    def profile_spread(self, kernel: str):
        """(min, max, std) in ms of the timed dispatches of one kernel since the last reset"""
        mn, mx, sd = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self.lib.tsd_profile_get_spread(self.h, kernel.encode(), C.byref(mn), C.byref(mx), C.byref(sd))
        return mn.value, mx.value, sd.value

    def profile_samples(self, kernel: str, cap: int = 65536) -> np.ndarray:
        """the timed dispatches of one kernel since the last reset, in launch order (ms)"""
        buf = np.zeros(cap, dtype=np.float32)
        n = self.lib.tsd_profile_get_samples(self.h, kernel.encode(), buf.ctypes.data_as(C.POINTER(C.c_float)), cap)
        self._check(min(n, 0), "tsd_profile_get_samples")
        return buf[: min(n, cap)].copy()

    def profile_get(self, kernel: str):
        ms = C.c_double(0.0)
        n = C.c_int(0)
        self.lib.tsd_profile_get(self.h, kernel.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value


class TsdSensorDevice:
    """Device-resident ``SensorPolar2D`` + pose bookkeeping of one robot on a grid (fused scan path)."""

    def __init__(self, grid: TsdGridDevice, beams, ang_res, phi_min, max_range, min_range, low_refl):
        self.grid = grid
        self.lib = grid.lib
        self.h = self.lib.tsd_sensor_create(grid.h, beams, ang_res, phi_min, max_range, min_range, low_refl)
        if not self.h:
            raise TsdError("tsd_sensor_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_sensor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pose(self, pose, rays_world, rays_local):
        pose, rw, rl = _f64(pose).reshape(9), _f64(rays_world), _f64(rays_local)
        self.grid._check(self.lib.tsd_sensor_set_pose(self.h, _d(pose), _d(rw), _d(rl)), "tsd_sensor_set_pose")

    def scan_ahead(self, ranges, mask, mask_push, params: IcpParams, gates: GateParams, nxt=None, nxt_pre=None) -> ScanResult:
        """tsd_scan_submit (``ranges`` None: the scan staged by the previous call) + tsd_scan_stage of ``nxt`` = (ranges, mask,
        mask_push) while the registration runs (+ tsd_scan_preregister(*nxt_pre) for that staged scan, also ahead of the collect)
        + tsd_scan_collect"""
        if ranges is None:
            rc = self.lib.tsd_scan_submit(self.h, None, None, None, C.byref(params), C.byref(gates))
        else:
            rg, mk = _f64(ranges), np.ascontiguousarray(mask, dtype=np.uint8)
            mp = np.ascontiguousarray(mask_push, dtype=np.uint8) if mask_push is not None else None
            rc = self.lib.tsd_scan_submit(self.h, _d(rg), _u8(mk), _u8(mp) if mp is not None else None, C.byref(params), C.byref(gates))
        self.grid._check(rc, "tsd_scan_submit")
        if nxt is not None:
            rg, mk = _f64(nxt[0]), np.ascontiguousarray(nxt[1], dtype=np.uint8)
            mp = np.ascontiguousarray(nxt[2], dtype=np.uint8) if nxt[2] is not None else None
            self.grid._check(self.lib.tsd_scan_stage(self.h, _d(rg), _u8(mk), _u8(mp) if mp is not None else None), "tsd_scan_stage")
        if nxt_pre is not None:
            self.preregister(*nxt_pre)
        r = ScanResult()
        self.grid._check(self.lib.tsd_scan_collect(self.h, C.byref(r)), "tsd_scan_collect")
        return r

    def preregister(self, scene_xy, mask_s, trials, size_control_set, zrand, phi_max, ang_res, draws_sub, draws_ctrl, draws_trials):
        """tsd_scan_preregister: registration_mode 3's TSD_PDF pre-registration for the NEXT scan of this sensor, on the device
        between its ray cast and its registration"""
        prm = TsdPdfParams(int(trials), int(size_control_set), 0.0, float(zrand), float(phi_max), float(ang_res))
        S, mS = _f64(scene_xy).reshape(-1), np.ascontiguousarray(mask_s, dtype=np.uint8)
        ds, dc, dt = (np.ascontiguousarray(x, dtype=np.int32) for x in (draws_sub, draws_ctrl, draws_trials))
        rc = self.lib.tsd_scan_preregister(self.h, C.byref(prm), _d(S), _u8(mS), ds.ctypes.data_as(_ip), dc.ctypes.data_as(_ip),
                                           dt.ctypes.data_as(_ip))
        self.grid._check(rc, "tsd_scan_preregister")

    def set_async_mapping(self, on=True):
        """tsd_sensor_set_async_mapping: the fused scan's push beside the next registration (the next ray cast one push behind)."""
        self.grid._check(self.lib.tsd_sensor_set_async_mapping(self.h, 1 if on else 0), "tsd_sensor_set_async_mapping")

    def preregistration_result(self) -> dict:
        r = TsdPdfResult()
        self.grid._check(self.lib.tsd_scan_preregistration_result(self.h, C.byref(r)), "tsd_scan_preregistration_result")
        return {"T": np.array(r.T[:]).reshape(3, 3), "prob": r.probability, "idx": r.idx_model, "i": r.idx_scene,
                "candidates": r.candidates, "valid_model": r.valid_model, "valid_scene": r.valid_scene, "control_points": r.control_points}

    def scan(self, ranges, mask, mask_push, params: IcpParams, gates: GateParams) -> ScanResult:
        rg = _f64(ranges)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        mp = np.ascontiguousarray(mask_push, dtype=np.uint8) if mask_push is not None else None
        r = ScanResult()
        rc = self.lib.tsd_scan(self.h, _d(rg), _u8(mk), _u8(mp) if mp is not None else None, C.byref(params),
                               C.byref(gates), C.byref(r))
        self.grid._check(rc, "tsd_scan")
        return r


class TsdBatch:
    """One batch slot of the multi-robot path (``tsd_batch_*``): the scans of several sensors on one grid registered by one
    launch of each kernel, their pushes applied in the order of the batch."""

    def __init__(self, grid: TsdGridDevice, max_scans: int):
        self.grid = grid
        self.lib = grid.lib
        self.h = self.lib.tsd_batch_create(grid.h, max_scans)
        if not self.h:
            raise TsdError("tsd_batch_create failed")
        self._keep = None
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self, sensors, ranges, masks, masks_push, params, gates):
        """``params`` / ``gates``: one IcpParams / GateParams for all scans, or a list with one per scan."""
        n = len(sensors)
        rg = [_f64(r) for r in ranges]
        mk = [np.ascontiguousarray(m, dtype=np.uint8) for m in masks]
        mp = [np.ascontiguousarray(m, dtype=np.uint8) if m is not None else None for m in (masks_push or [None] * n)]
        hs = (C.c_void_p * n)(*[s.h for s in sensors])
        rp = (_dp * n)(*[_d(r) for r in rg])
        mkp = (_u8p * n)(*[_u8(m) for m in mk])
        mpp = (_u8p * n)(*[_u8(m) if m is not None else C.cast(None, _u8p) for m in mp])
        pl = params if isinstance(params, (list, tuple)) else [params] * n
        gl = gates if isinstance(gates, (list, tuple)) else [gates] * n
        pa = (IcpParams * n)(*pl)
        ga = (GateParams * n)(*gl)
        self._keep = (rg, mk, mp)
        self.grid._check(self.lib.tsd_batch_begin(self.h, n, hs, rp, mkp, mpp, pa, ga), "tsd_batch_begin")
        self.n = n

    def push(self):
        self.grid._check(self.lib.tsd_batch_push(self.h), "tsd_batch_push")

    def poll(self) -> bool:
        return self.lib.tsd_batch_poll(self.h) == 1

    def results(self):
        out = (ScanResult * self.n)()
        self.grid._check(self.lib.tsd_batch_results(self.h, out), "tsd_batch_results")
        self._keep = None
        return list(out)
