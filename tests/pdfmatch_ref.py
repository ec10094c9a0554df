"""The plain-C restatement of PDFMatching::match (tests/pdfmatch_restate.c) built into a temporary directory and bound with
ctypes, plus the scene set-up the registration_mode-2 tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from ohm_tsd_slam_amd import capi, synth
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_ip = C.POINTER(C.c_int)


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libpdfmatch_restate.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-std=gnu99", "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "pdfmatch_restate.c"), "-o", out, "-lm"], check=True, capture_output=True, text=True)
    lib = C.CDLL(out)
    lib.pdfr_prob.restype = C.c_double
    lib.pdfr_prob.argtypes = [C.POINTER(capi.PdfMatchParams), C.c_double, C.c_double]
    lib.pdfr_nearest.restype = C.c_int
    lib.pdfr_nearest.argtypes = [_dp, C.c_int, C.c_double, _dp]
    lib.pdfr_match.restype = C.c_int
    lib.pdfr_match.argtypes = [_dp, _u8p, _dp, _u8p, C.c_int, C.POINTER(capi.PdfMatchParams), _ip, _ip, _ip, _dp, _dp, _ip, _dp, _ip, C.c_int]
    return lib


def params(phi_max=0.0, ang_res=0.0, **kw):
    return capi.PdfMatchParams(phi_max=phi_max, ang_res=ang_res, **dict(capi.PDFMATCH_DEFAULTS, **kw))


class Restatement:
    def __init__(self, lib):
        self.lib = lib

    def prob(self, prm, m, s):
        return self.lib.pdfr_prob(C.byref(prm), m, s)

    def nearest(self, A, q):
        A = np.ascontiguousarray(A, dtype=np.float64)
        best = C.c_double(0.0)
        k = self.lib.pdfr_nearest(A.ctypes.data_as(_dp), A.size, q, C.byref(best))
        return k, best.value

    def match(self, M, mask_m, S, mask_s, phi_max, ang_res, ds, dc, dt, **kw):
        """the restatement's result in the keys of capi.TsdGridDevice.pdf_match, plus rc and the per-candidate values"""
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1)
        mM, mS = np.ascontiguousarray(mask_m, dtype=np.uint8), np.ascontiguousarray(mask_s, dtype=np.uint8)
        ds, dc, dt = (np.ascontiguousarray(x, dtype=np.int32) for x in (ds, dc, dt))
        prm = params(phi_max, ang_res, **kw)
        n = M.size // 2
        cap = max(1, prm.trials * n)
        T, prob, cnt = np.zeros(9), C.c_double(0.0), np.zeros(6, dtype=np.int32)
        ung, fov = np.zeros(cap), np.zeros(cap, dtype=np.int32)
        rc = self.lib.pdfr_match(M.ctypes.data_as(_dp), mM.ctypes.data_as(_u8p), S.ctypes.data_as(_dp), mS.ctypes.data_as(_u8p), n,
                                 C.byref(prm), ds.ctypes.data_as(_ip), dc.ctypes.data_as(_ip), dt.ctypes.data_as(_ip),
                                 T.ctypes.data_as(_dp), C.byref(prob), cnt.ctypes.data_as(_ip), ung.ctypes.data_as(_dp),
                                 fov.ctypes.data_as(_ip), cap)
        nc = int(cnt[0])
        return dict(rc=rc, T=T.reshape(3, 3), prob=prob.value, candidates=nc, valid_model=int(cnt[1]), valid_scene=int(cnt[2]),
                    control=int(cnt[3]), idx=int(cnt[4]), i=int(cnt[5]), ungated=ung[:min(nc, cap)].copy(), fov=fov[:min(nc, cap)].copy())


def oracle_scene(oracle, cfg, k_pose=3, k_scan=8, dyaw=0.05, pushes=4, scene=None):
    """a grid built by the oracle from `pushes` scans, its ray-cast model at pose k_pose and the scene of the scan taken at
    k_scan (yaw + dyaw): what ThreadLocalize hands a pre-registration.  CPU only."""
    gc, geo, scene0 = synth.CONFIGS[cfg]
    world = synth.World(scene or scene0, gc)
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for k in range(pushes):
        pose, (x, y, yaw) = H.sensor_pose(world, k)
        data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), H.MAX_RANGE, geo.angle_increment)
        og.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
    pose, _ = H.sensor_pose(world, k_pose)
    _, (x, y, yaw) = H.sensor_pose(world, k_scan)
    rl, rw = H.world_rays(oracle, geo, pose, gc.cell_size)
    co, no, mo, cnt = og.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw + dyaw, geo), H.MAX_RANGE, geo.angle_increment)
    sc, ms, ns = oracle.scene_from_scan(rl, data, mask)
    Ttrue = np.linalg.inv(pose) @ synth.pose_matrix(x, y, yaw + dyaw)
    return dict(gc=gc, geo=geo, grid=og, pose=pose, M=co, mask_m=mo, S=sc, mask_s=ms, Ttrue=Ttrue, rays_world=rw, rays_local=rl,
                data=data, mask=mask)

