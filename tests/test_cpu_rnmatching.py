"""CPU checks of registration_mode 1 (RandomNormalMatching pre-registration; RandomNormalMatching.cpp:67-395): the restatement's
selection rule against a Python transcription (the fabs-of-a-bool quirk included), its front end against the oracle's mode-3 one,
its winner on a synthetic scene, and the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import pdfmatch_ref as P
from tests import rnmatch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSD_E_ARG = -1                                           # include/tsd_hip.h


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return R.Restatement(R.build(tmp_path_factory.mktemp("rnr")))


def selection_cases():
    """(cnt, max_cnt, err, thresh) arrays: random ones and the adversarial orders the device fold must also survive"""
    rng = np.random.default_rng(11)
    cases = []
    for n in (1, 5, 63, 64, 65, 130, 1000):
        mx = rng.integers(40, 141, n)
        cnt = np.minimum(mx, rng.integers(0, 141, n))
        err = rng.uniform(10.0, 200.0, n)
        cases.append((cnt, mx, err, 46))
    # few distinct values: many equal counts, ratios and errors
    n = 300
    mx = rng.choice([100, 120, 140], n)
    cnt = rng.choice([50, 60, 100], n)
    cnt = np.minimum(cnt, mx)
    err = rng.choice([20.0, 20.0 + 1e-13, 30.0], n)
    cases.append((cnt, mx, err, 46))
    # ratio differences of exactly 1e-5 (and a hair either side): 1e5 - 1 of 1e5 against 1e5 of 1e5, etc.
    cases.append((np.array([99999, 100000, 99999, 99998]), np.array([100000] * 4), np.array([5.0, 6.0, 4.0, 3.0]), 10))
    cases.append((np.array([50, 50, 51, 51]), np.array([100000, 100000, 100000, 99999]), np.array([9.0, 8.0, 9.0, 1.0]), 10))
    # ties in errSum at equal counts: the first keeps it
    cases.append((np.array([60, 60, 60]), np.array([100, 100, 100]), np.array([7.0, 7.0, 7.0]), 46))
    # nothing above the threshold
    cases.append((np.array([10, 46, 46]), np.array([100, 100, 100]), np.array([1.0, 2.0, 3.0]), 46))
    return cases


def test_selection_rule_matches_a_python_transcription(restate):
    for cnt, mx, err, th in selection_cases():
        assert restate.select(cnt, mx, err, th) == R.py_select(cnt, mx, err, th), (cnt[:8], mx[:8], err[:8], th)
    assert restate.select(np.array([10, 46]), np.array([100, 100]), np.array([1.0, 2.0]), 46) == -1


def test_selection_keeps_the_fabs_of_a_bool_quirk(restate):
    """fabs((ratio - bestRatio) < equalThres) is fabs() of a bool: a LOWER ratio with the same count and a smaller error replaces
    the best.  With fabs(ratio - bestRatio) < equalThres, candidate 0 would stay."""
    cnt, mx, err = np.array([60, 60]), np.array([60, 120]), np.array([9.0, 8.0])
    assert R.py_select(cnt, mx, err, 46) == 1
    assert restate.select(cnt, mx, err, 46) == 1
    # the same without the lower error: 0 stays
    assert restate.select(cnt, mx, np.array([9.0, 9.5]), 46) == 0
    # a higher count at a lower ratio does not pass rateCondition, and the counts differ: 0 stays
    assert restate.select(np.array([60, 61]), np.array([60, 122]), np.array([9.0, 1.0]), 46) == 0


@pytest.mark.parametrize("cfg,seed,trials,phi_deg", [("cfg1", 1, 100, 30.0), ("cfg2", 2, 100, 30.0), ("cfg2", 5, 600, 90.0)])
def test_restatement_front_end_equals_the_oracles(oracle, restate, cfg, seed, trials, phi_deg):
    """RandomNormalMatching::match shares its front end with PDFMatching / TSD_PDFMatching (:79-262): for the same draws the
    restatement rates exactly as many (trial, i) candidates as the oracle's mode-3 restatement, with the same counts"""
    sc = P.oracle_scene(oracle, cfg)
    geo = sc["geo"]
    rng = np.random.default_rng(seed)
    ds, dc, dt = (rng.integers(0, 2 ** 31 - 1, n) for n in (geo.beams, 140, trials))
    phi = math.radians(phi_deg)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, geo.angle_increment, ds, dc, dt, trials=trials)
    ro = oracle.tsdpdf_match(sc["grid"], sc["pose"], sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], trials, 140, 0.25, phi,
                             geo.angle_increment, ds, dc, dt)
    assert rr["rc"] == 0 and ro["rc"] == 0
    assert rr["candidates"] == ro["candidates"] > 100
    assert rr["control"] == 140 and len(rr["cnt"]) == rr["candidates"]
    assert np.all(rr["cnt"] <= rr["max_cnt"]) and np.all(rr["max_cnt"] <= 140)
    # the winner is the serial fold over the per-candidate values
    assert rr["winner"] == R.py_select(rr["cnt"], rr["max_cnt"], rr["errs"], 140 // 3)


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2"])
def test_restatement_winner_is_near_the_true_motion(oracle, restate, cfg):
    sc = P.oracle_scene(oracle, cfg)
    geo = sc["geo"]
    rng = np.random.default_rng(7)
    ds, dc, dt = (rng.integers(0, 2 ** 31 - 1, n) for n in (geo.beams, 140, 100))
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], math.radians(30.0), geo.angle_increment, ds, dc, dt)
    assert rr["rc"] == 0 and rr["idx"] >= 0 and rr["winner"] >= 0
    d = np.hypot(*(rr["T"][:2, 2] - sc["Ttrue"][:2, 2]))
    a = abs(math.atan2(rr["T"][1, 0], rr["T"][0, 0]) - math.atan2(sc["Ttrue"][1, 0], sc["Ttrue"][0, 0]))
    assert d < 0.3 and a < 0.1, (d, a)
    assert rr["cnt"][rr["winner"]] > 140 // 3 and 0.0 < rr["ratio"] <= 1.0


def test_abi_symbols_and_sizes(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "tsd_hip.h")).read()
    assert re.search(r"int tsd_rn_match\(tsd_ctx\* ctx,", hdr)
    assert "tsd_debug_rn_match_scores(" in hdr and "tsd_debug_rn_select(" in hdr
    for name in ("tsd_rn_match", "tsd_debug_rn_match_scores", "tsd_debug_rn_select"):
        assert name in capi.ABI and hasattr(hip_lib, name)
    assert C.sizeof(capi.RnMatchParams) == 8 + 3 * 8
    assert capi.RnMatchParams.eps_thresh.offset == 8 and capi.RnMatchParams.ang_res.offset == 8 + 2 * 8
    assert C.sizeof(capi.RnMatchResult) == 11 * 8 + 10 * 4
    assert capi.RnMatchResult.cnt_match.offset == 88 and capi.RnMatchResult.control_points.offset == 88 + 7 * 4
    assert hip_lib.tsd_abi_sizeof(b"tsd_rnmatch_params") == C.sizeof(capi.RnMatchParams)
    assert hip_lib.tsd_abi_sizeof(b"tsd_rnmatch_result") == C.sizeof(capi.RnMatchResult)
    assert capi.RNMATCH_DEFAULTS == dict(trials=100, size_control_set=140, eps_thresh=0.15)
    # the existing records are untouched
    assert hip_lib.tsd_abi_sizeof(b"tsd_pdfmatch_params") == C.sizeof(capi.PdfMatchParams) == 8 + 15 * 8
    assert hip_lib.tsd_abi_sizeof(b"tsd_tsdpdf_result") == C.sizeof(capi.TsdPdfResult)


def test_rn_match_without_context_is_an_argument_error(hip_lib):
    n = 8
    M = np.zeros(2 * n)
    m = np.ones(n, dtype=np.uint8)
    d = np.zeros(n, dtype=np.int32)
    prm = R.params(0.5, 0.01)
    res = capi.RnMatchResult()
    _dp, _u8p, _ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    args = (M.ctypes.data_as(_dp), m.ctypes.data_as(_u8p), M.ctypes.data_as(_dp), m.ctypes.data_as(_u8p), n, C.byref(prm),
            d.ctypes.data_as(_ip), d.ctypes.data_as(_ip), d.ctypes.data_as(_ip), C.byref(res))
    assert hip_lib.tsd_rn_match(None, *args) == TSD_E_ARG
    assert hip_lib.tsd_debug_rn_match_scores(None, None, None, None, 0) == TSD_E_ARG
    w = C.c_int(0)
    assert hip_lib.tsd_debug_rn_select(None, d.ctypes.data_as(_ip), d.ctypes.data_as(_ip), M.ctypes.data_as(_dp), 1, 0,
                                       C.byref(w)) == TSD_E_ARG
