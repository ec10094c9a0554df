"""The plain-C restatement of RandomNormalMatching::match (tests/rnmatch_restate.c) built into a temporary directory and bound with
ctypes, and a Python transcription of its selection rule.  The scene set-up is registration_mode 2's (pdfmatch_ref.oracle_scene)."""
import ctypes as C
import os
import subprocess

import numpy as np

from ohm_tsd_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_ip = C.POINTER(C.c_int)


def build(tmpdir):
    out = os.path.join(str(tmpdir), "librnmatch_restate.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-std=gnu99", "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "rnmatch_restate.c"), "-o", out, "-lm"], check=True, capture_output=True, text=True)
    lib = C.CDLL(out)
    lib.rnr_select.restype = C.c_int
    lib.rnr_select.argtypes = [_ip, _ip, _dp, C.c_int, C.c_int]
    lib.rnr_match.restype = C.c_int
    lib.rnr_match.argtypes = [_dp, _u8p, _dp, _u8p, C.c_int, C.POINTER(capi.RnMatchParams), _ip, _ip, _ip, _dp, _dp, _ip, _ip, _ip,
                              _dp, _u8p, C.c_int]
    return lib


def params(phi_max=0.0, ang_res=0.0, **kw):
    return capi.RnMatchParams(phi_max=phi_max, ang_res=ang_res, **dict(capi.RNMATCH_DEFAULTS, **kw))


def py_select(cnt, max_cnt, err, thresh):
    """Kuehn's rating (RandomNormalMatching.cpp:338-359) transcribed statement for statement: the winner's index or -1.
    `abs(float(x < 1e-5))` is the reference's fabs() of a bool."""
    bestRatio, bestCnt, bestErr, win = 0.0, 0, 1e12, -1
    for c in range(len(cnt)):
        cntMatch, maxCntMatch, errSum = int(cnt[c]) & 0xFFFFFFFF, int(max_cnt[c]) & 0xFFFFFFFF, float(err[c])
        if cntMatch <= (int(thresh) & 0xFFFFFFFF):
            continue
        ratio = float(np.float64(cntMatch) / np.float64(maxCntMatch))
        equalThres = 1e-5
        rateCondition = ((ratio - bestRatio) > equalThres) and (cntMatch > bestCnt)
        similarityCondition = abs(float((ratio - bestRatio) < equalThres)) != 0.0 and (cntMatch == bestCnt) and errSum < bestErr
        if rateCondition or similarityCondition:
            bestRatio, bestCnt, bestErr, win = ratio, cntMatch, errSum, c
    return win


class Restatement:
    def __init__(self, lib):
        self.lib = lib

    def select(self, cnt, max_cnt, err, thresh):
        c, m = np.ascontiguousarray(cnt, dtype=np.int32), np.ascontiguousarray(max_cnt, dtype=np.int32)
        e = np.ascontiguousarray(err, dtype=np.float64)
        return self.lib.rnr_select(c.ctypes.data_as(_ip), m.ctypes.data_as(_ip), e.ctypes.data_as(_dp), int(c.size), int(thresh))

    def match(self, M, mask_m, S, mask_s, phi_max, ang_res, ds, dc, dt, **kw):
        """the restatement's result in the keys of capi.TsdGridDevice.rn_match, plus rc, the winner's candidate index and the
        per-candidate values (cnt, max_cnt, err_sum, near: an in-view err within 1e-12 of 1.0)"""
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1)
        mM, mS = np.ascontiguousarray(mask_m, dtype=np.uint8), np.ascontiguousarray(mask_s, dtype=np.uint8)
        ds, dc, dt = (np.ascontiguousarray(x, dtype=np.int32) for x in (ds, dc, dt))
        prm = params(phi_max, ang_res, **kw)
        n = M.size // 2
        cap = max(1, prm.trials * n)
        T, best, cnt = np.zeros(9), np.zeros(2), np.zeros(8, dtype=np.int32)
        cm, mx, es, near = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap, dtype=np.uint8)
        rc = self.lib.rnr_match(M.ctypes.data_as(_dp), mM.ctypes.data_as(_u8p), S.ctypes.data_as(_dp), mS.ctypes.data_as(_u8p), n,
                                C.byref(prm), ds.ctypes.data_as(_ip), dc.ctypes.data_as(_ip), dt.ctypes.data_as(_ip),
                                T.ctypes.data_as(_dp), best.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip), cm.ctypes.data_as(_ip),
                                mx.ctypes.data_as(_ip), es.ctypes.data_as(_dp), near.ctypes.data_as(_u8p), cap)
        nc = int(cnt[0])
        k = min(nc, cap)
        return dict(rc=rc, T=T.reshape(3, 3), ratio=float(best[0]), err_sum=float(best[1]), candidates=nc, valid_model=int(cnt[1]),
                    valid_scene=int(cnt[2]), control=int(cnt[3]), idx=int(cnt[4]), i=int(cnt[5]), winner=int(cnt[6]),
                    cnt=cm[:k].copy(), max_cnt=mx[:k].copy(), errs=es[:k].copy(), near=near[:k].astype(bool))
