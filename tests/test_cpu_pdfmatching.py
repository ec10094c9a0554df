"""CPU checks of registration_mode 2 (PDFMatching pre-registration; PDFMatching.cpp:47-487): the restatement's beam model and
nearest-angle rule against independent Python statements, its front end against the oracle's mode-3 one, and the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import pdfmatch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSD_E_ARG = -1                                           # include/tsd_hip.h


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return R.Restatement(R.build(tmp_path_factory.mktemp("pdfr")))


def _py_prob(p, m, s):
    """probabilityOfTwoSingleScans in Python, math.pow(math.e, .) where the reference has pow(M_E, .)"""
    e = math.e
    sigphit = 1.0 / (math.sqrt(2.0 * math.pi) * p.sighit)
    phit = pphi = pshort = pmax = prand = 0.0
    if s < p.rangemax:
        phit = sigphit * math.pow(e, ((-0.5 * math.pow((m - s), 2)) / (p.sighit * p.sighit)))
    pphi = p.sigphi * math.pow(e, ((-0.5 * s * s) / (p.sigphi * p.sigphi)))
    if s < m:
        n = 1.0 / (1.0 - math.pow(e, (-p.lamshort * m)))
        pshort = n * p.lamshort * math.pow(e, (-p.lamshort * s))
    if s >= p.rangemax:
        pmax = 1.0
    if s < p.rangemax:
        prand = 1.0 / p.rangemax
    return p.zhit * phit + p.zshort * pshort + p.zmax * pmax + p.zrand * prand + p.zphi * pphi


@pytest.mark.parametrize("zphi", [0.0, 0.1])
def test_probability_of_two_single_scans(restate, zphi):
    p = R.params(zphi=zphi)
    cases = [(3.0, 25.0), (21.0, 20.0), (5.0, 20.0),         # s >= rangemax
             (4.0, 3.9), (10.0, 2.0), (0.5, 0.01),           # s < m
             (2.0, 2.0), (2.0, 2.05), (1.0, 7.5)]            # s >= m
    for m, s in cases:
        a, b = restate.prob(p, m, s), _py_prob(p, m, s)
        assert a == b, (m, s, a, b)
        assert a > 0.0
    # the terms switch where the reference's conditions say: past rangemax only zmax (and zphi pphi) remain
    assert restate.prob(R.params(zphi=0.0), 3.0, 25.0) == capi.PDFMATCH_DEFAULTS["zmax"] * 1.0


def _first_argmin(A, q):
    d = np.abs(q - np.asarray(A, dtype=np.float64))
    k = int(np.argmin(d))                                    # numpy: the first of equal minima
    return (k, float(d[k])) if d[k] < 2 * math.pi else (0, 2 * math.pi)


def test_nearest_angle_rule(restate):
    rng = np.random.default_rng(3)
    arrays = [np.sort(rng.uniform(-math.pi, math.pi, 300)),                                        # sorted
              np.repeat(np.linspace(-1.0, 1.0, 40), 3),                                             # ties (equal angles)
              np.concatenate([np.linspace(2.0, math.pi, 50), np.linspace(-math.pi, -2.0, 50)]),    # a 360-degree scan wrapping at +-pi
              np.array([-math.pi, math.pi])]                                                        # both ends
    for A in arrays:
        qs = np.concatenate([rng.uniform(-math.pi, math.pi, 200), A[:20], (A[:-1] + A[1:])[:20] / 2, [-math.pi, math.pi, 0.0]])
        for q in qs:
            assert restate.nearest(A, float(q)) == _first_argmin(A, float(q)), (A[:5], q)
    # no difference below 2 pi: idx 0 and 2 pi
    assert restate.nearest(np.array([-math.pi]), math.pi) == (0, 2 * math.pi)


@pytest.mark.parametrize("cfg,seed,trials,phi_deg", [("cfg1", 1, 100, 30.0), ("cfg2", 2, 100, 30.0), ("cfg2", 5, 600, 90.0)])
def test_restatement_front_end_equals_the_oracles(oracle, restate, cfg, seed, trials, phi_deg):
    """the two matchers share their front end (PDFMatching.cpp:45-220 = TSD_PDFMatching.cpp:31-205): for the same draws the
    restatement scores exactly as many (trial, i) candidates as the oracle's mode-3 restatement"""
    sc = R.oracle_scene(oracle, cfg)
    geo = sc["geo"]
    rng = np.random.default_rng(seed)
    ds, dc, dt = (rng.integers(0, 2 ** 31 - 1, n) for n in (geo.beams, 140, trials))
    phi = math.radians(phi_deg)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, geo.angle_increment, ds, dc, dt, trials=trials)
    ro = oracle.tsdpdf_match(sc["grid"], sc["pose"], sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], trials, 140, 0.25, phi,
                             geo.angle_increment, ds, dc, dt)
    assert rr["rc"] == 0 and ro["rc"] == 0
    assert rr["candidates"] == ro["candidates"] > 100
    assert rr["control"] == 140 and len(rr["fov"]) == rr["candidates"]
    # a sensible pre-registration too: the winner is near the true motion
    d, a = (np.hypot(*(rr["T"][:2, 2] - sc["Ttrue"][:2, 2])),
            abs(math.atan2(rr["T"][1, 0], rr["T"][0, 0]) - math.atan2(sc["Ttrue"][1, 0], sc["Ttrue"][0, 0])))
    assert rr["idx"] >= 0 and d < 0.3 and a < 0.1, (d, a)


def test_abi_symbols_and_sizes(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "tsd_hip.h")).read()
    assert re.search(r"int tsd_pdf_match\(tsd_ctx\* ctx,", hdr) and "tsd_debug_pdf_match_scores(" in hdr
    for name in ("tsd_pdf_match", "tsd_debug_pdf_match_scores"):
        assert name in capi.ABI and hasattr(hip_lib, name)
    assert C.sizeof(capi.PdfMatchParams) == 8 + 15 * 8
    assert capi.PdfMatchParams.eps_thresh.offset == 8 and capi.PdfMatchParams.ang_res.offset == 8 + 14 * 8
    assert hip_lib.tsd_abi_sizeof(b"tsd_pdfmatch_params") == C.sizeof(capi.PdfMatchParams)
    # the existing records are untouched
    assert hip_lib.tsd_abi_sizeof(b"tsd_tsdpdf_params") == C.sizeof(capi.TsdPdfParams) == 2 * 4 + 4 * 8
    assert hip_lib.tsd_abi_sizeof(b"tsd_tsdpdf_result") == C.sizeof(capi.TsdPdfResult)


def test_pdf_match_without_context_is_an_argument_error(hip_lib):
    n = 8
    M = np.zeros(2 * n)
    m = np.ones(n, dtype=np.uint8)
    d = np.zeros(n, dtype=np.int32)
    prm = R.params(0.5, 0.01)
    res = capi.TsdPdfResult()
    _dp, _u8p, _ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    args = (M.ctypes.data_as(_dp), m.ctypes.data_as(_u8p), M.ctypes.data_as(_dp), m.ctypes.data_as(_u8p), n, C.byref(prm),
            d.ctypes.data_as(_ip), d.ctypes.data_as(_ip), d.ctypes.data_as(_ip), C.byref(res))
    assert hip_lib.tsd_pdf_match(None, *args) == TSD_E_ARG
    assert hip_lib.tsd_debug_pdf_match_scores(None, None, None, 0) == TSD_E_ARG
