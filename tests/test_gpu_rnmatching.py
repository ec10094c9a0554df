"""GPU tests of registration_mode 1: the RandomNormalMatching pre-registration (RandomNormalMatching.cpp:67-395) on the device
(tsd_rn_match) against the plain-C restatement tests/rnmatch_restate.c for identical rand() draws, the device selection against the
serial rule, and ThreadLocalize in mode 1 (ray cast -> RandomNormalMatching::match -> Icp::iterate with its result as Tinit,
ThreadLocalize.cpp:537-545) against a test-side loop of the oracle's primitives.  Counts exact (cntMatch unless an err lies within
1e-12 of 1.0), errSum to 1e-12 relative, winners exact unless the restatement's fold has a near-tie."""
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import helpers as H
from tests import pdfmatch_ref as P
from tests import rnmatch_ref as R
from tests.slam_driver import slam_kwargs
from tests.test_cpu_rnmatching import selection_cases
from tests.test_gpu_pdfmatching import _libc_draws, _Mode2Loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return R.Restatement(R.build(tmp_path_factory.mktemp("rnr")))


_SCENES = {}


def _scene(oracle, cfg):
    if cfg not in _SCENES:
        _SCENES[cfg] = P.oracle_scene(oracle, cfg)
    return _SCENES[cfg]


def _context():
    gc = synth.CONFIGS["cfg1"][0]                    # (mode 1 reads no grid: the smallest context)
    return capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)


def _draws(seed, beams, ctrl, trials):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 2 ** 31 - 1, n) for n in (beams, ctrl, trials))


def _compare(dg, rr, rh):
    """device == restatement: counts and maxCntMatch exact, cntMatch exact except where the restatement has an err within 1e-12 of
    1.0, errSum to 1e-12 relative; the device's selection is the serial rule on its own values, and its winner is the restatement's
    unless the fold has a near-tie there (then the test checks that it is one).  True if the winners agree."""
    for k in ("candidates", "valid_model", "valid_scene", "control"):
        assert rh[k] == rr[k], (k, rh[k], rr[k])
    cnt, mx, err = dg.debug_rn_match_scores()
    assert len(cnt) == rr["candidates"]
    assert np.array_equal(mx, rr["max_cnt"]), np.nonzero(mx != rr["max_cnt"])[0][:10]
    diff = cnt != rr["cnt"]
    assert not np.any(diff & ~rr["near"]), np.nonzero(diff & ~rr["near"])[0][:10]
    rel = np.abs(err - rr["errs"]) / np.maximum(np.abs(rr["errs"]), 1e-300)
    assert np.all((rel <= 1e-12) | ((err == 0.0) & (rr["errs"] == 0.0))), (np.count_nonzero(rel > 1e-12), rel.max())
    thresh = rr["control"] // 3
    wd = R.py_select(cnt, mx, err, thresh)
    assert (wd >= 0) == (rh["idx"] >= 0)
    if wd >= 0:
        assert rh["cnt"] == cnt[wd] and rh["max_cnt"] == mx[wd] and rh["err_sum"] == err[wd]
    if wd != rr["winner"]:
        # a near-tie: a count moved by a near-boundary err, or the two winners' errSums (equal counts) within rounding
        wr = rr["winner"]
        moved = bool(np.any(diff))
        close = (wr >= 0 and wd >= 0 and cnt[wd] == rr["cnt"][wr] and
                 abs(rr["errs"][wd] - rr["errs"][wr]) <= 1e-12 * rr["errs"][wr])
        assert moved or close, ("different winner without a near-tie", wd, wr, rh, rr["idx"], rr["i"])
        return False
    assert (rh["idx"], rh["i"]) == (rr["idx"], rr["i"])
    if wd >= 0:
        assert rh["ratio"] == rr["ratio"] and rh["cnt"] == rr["cnt"][wd]
    else:
        assert rh["ratio"] == 0.0 and rh["err_sum"] == 1e12
    assert np.max(np.abs(rh["T"] - rr["T"])) <= 1e-12
    return True


# >= 20 seeds over the cfg 1 (360 degrees, 1 degree beams) and cfg 2 (270 degrees, 0.25 degree beams) geometries, trials 30 / 100 /
# 600 and phiMax 30 / 90 degrees
_CASES = ([("cfg1", t, p, s) for (t, p) in ((30, 30.0), (100, 30.0), (100, 90.0), (600, 90.0)) for s in (1, 2, 3)] +
          [("cfg2", t, p, s) for (t, p) in ((30, 30.0), (100, 30.0), (100, 90.0)) for s in (4, 5, 6)] + [("cfg2", 600, 30.0, 7)])


@pytest.mark.parametrize("cfg,trials,phi_deg,seed", _CASES)
def test_rn_match_matches_restatement(oracle, restate, cfg, trials, phi_deg, seed):
    sc = _scene(oracle, cfg)
    geo = sc["geo"]
    ds, dc, dt = _draws(seed, geo.beams, 140, trials)
    args = (sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], math.radians(phi_deg), geo.angle_increment, ds, dc, dt)
    rr = restate.match(*args, trials=trials)
    dg = _context()
    rh = dg.rn_match(*args, trials=trials)
    assert rr["rc"] == 0 and rr["candidates"] > 100
    _compare(dg, rr, rh)
    assert rh["idx"] >= 0 and rh["ratio"] > 0.0


def test_rn_select_matches_the_serial_rule():
    dg = _context()
    rng = np.random.default_rng(5)
    cases = list(selection_cases())
    # the fabs-of-a-bool quirk: a lower ratio, the same count and a smaller error win
    cases.append((np.array([60, 60]), np.array([60, 120]), np.array([9.0, 8.0]), 46))
    # many acceptances inside one 64-block and across blocks: rising counts, falling errors
    n = 200
    cases.append((np.arange(50, 50 + n), np.full(n, 400), np.linspace(100.0, 1.0, n), 46))
    cases.append((np.full(n, 80), np.full(n, 100), np.linspace(100.0, 1.0, n), 46))
    # equal errSums everywhere, one count per block rising; n = 1 above and below the threshold; n = 0
    cases.append((np.repeat(np.arange(60, 64), 64)[:250], np.full(250, 100), np.full(250, 3.0), 46))
    cases += [(np.array([47]), np.array([100]), np.array([1.0]), 46), (np.array([46]), np.array([100]), np.array([1.0]), 46),
              (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 46)]
    for _ in range(20):
        n = int(rng.integers(1, 700))
        mx = rng.integers(40, 141, n)
        cases.append((np.minimum(mx, rng.integers(30, 141, n)), mx, np.round(rng.uniform(5.0, 50.0, n), 1), 46))
    for cnt, mx, err, th in cases:
        assert dg.debug_rn_select(cnt, mx, err, th) == R.py_select(cnt, mx, err, th), (len(cnt), cnt[:8], mx[:8], err[:8], th)


def test_rn_select_quirk_on_the_device():
    dg = _context()
    assert dg.debug_rn_select([60, 60], [60, 120], [9.0, 8.0], 46) == 1      # fabs((ratio - bestRatio) < 1e-5): any smaller ratio
    assert dg.debug_rn_select([60, 60], [60, 120], [9.0, 9.5], 46) == 0
    assert dg.debug_rn_select([10, 46], [100, 100], [1.0, 2.0], 46) == -1    # nothing above cntMatchThresh


def test_rn_match_degenerate_inputs(oracle, restate):
    sc = _scene(oracle, "cfg1")
    geo = sc["geo"]
    ds, dc, dt = _draws(9, geo.beams, 140, 100)
    dg = _context()
    phi, res = math.radians(30.0), geo.angle_increment
    # n < 3 (:88-92)
    rh = dg.rn_match(sc["M"][:4], sc["mask_m"][:2], sc["S"][:4], sc["mask_s"][:2], phi, res, ds, dc, dt)
    rr = restate.match(sc["M"][:4], sc["mask_m"][:2], sc["S"][:4], sc["mask_s"][:2], phi, res, ds, dc, dt)
    assert rr["rc"] == 1 and np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1 and rh["candidates"] == 0
    # fewer than 3 valid points in scene / model (:165-175)
    z = np.zeros_like(sc["mask_m"])
    for mm, ms in ((sc["mask_m"], z), (z, sc["mask_s"])):
        rh = dg.rn_match(sc["M"], mm, sc["S"], ms, phi, res, ds, dc, dt)
        rr = restate.match(sc["M"], mm, sc["S"], ms, phi, res, ds, dc, dt)
        assert rr["rc"] == 1 and np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1
        assert (rh["valid_model"], rh["valid_scene"], rh["control"]) == (rr["valid_model"], rr["valid_scene"], rr["control"])
    # resolution not set (:192-201): identity, no error
    rh = dg.rn_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, 0.0, ds, dc, dt)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, 0.0, ds, dc, dt)
    assert rr["rc"] == 2 and np.array_equal(rh["T"], np.eye(3)) and rh["candidates"] == 0
    assert (rh["valid_model"], rh["valid_scene"]) == (rr["valid_model"], rr["valid_scene"]) and rh["valid_model"] >= 3
    # no candidates: phiMax 0 lets no normal difference through
    rh = dg.rn_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], 0.0, res, ds, dc, dt)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], 0.0, res, ds, dc, dt)
    assert rr["candidates"] == rh["candidates"] == 0 and np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1
    # an empty control set: nothing is in view, nothing passes cntMatch > 0
    rh = dg.rn_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=0)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=0)
    assert rr["candidates"] > 0 and rh["control"] == 0
    _compare(dg, rr, rh)
    assert np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1 and rh["ratio"] == 0.0
    # and a tiny control set still matches
    rh = dg.rn_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=3, trials=5)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=3, trials=5)
    _compare(dg, rr, rh)


@pytest.mark.parametrize("cfg,n", [("cfg1", 12), ("cfg2", 10)])
def test_facade_registration_mode_1_matches_the_test_loop(oracle, restate, cfg, n):
    """ThreadLocalize with registration_mode 1 (before this mode existed on the device the node fell back to plain ICP and had no
    pre-registration to report): the whole closed loop against the test-side loop, both fed the same rand() draws"""
    gc, geo, scene = synth.CONFIGS[cfg]
    world = synth.World(scene, gc)
    poses = synth.trajectory(world, n)
    scans = synth.scans_for(world, geo, poses)
    geo_msg = synth.ScanGeometry(geo.beams, float(np.float32(geo.angle_min)), float(np.float32(geo.angle_increment)))
    trials, ctrl, eps, phimax, seed = 100, 140, 0.15, 30.0, 4242
    kw = slam_kwargs(gc, geo_msg, ransac_phi_max=phimax)
    loop = _Mode2Loop(oracle, restate, kw, dict(trials=trials, size_control_set=ctrl, eps_thresh=eps))
    params = facade.node_params(gc, geo)
    params.update({"registration_mode": 1, "trials": trials, "sizeControlSet": ctrl, "epsThresh": eps, "ransac_phi_max": phimax,
                   "tsdpdf_seed": seed})
    node = facade.SlamNode(params, synchronous=True)
    pushes, won = 0, 0
    for k in range(n):
        if k > 0:
            loop.draws = _libc_draws(seed + (k - 1), geo.beams, ctrl, trials)
        ro = loop.process_scan(scans[k])
        node.laser(scans[k], geo.angle_min, geo.angle_increment)
        rh = node.report()
        d, a = H.pose_delta(ro["pose"], rh["pose"])
        assert d <= 1e-4 and a <= 1e-4, f"scan {k}: {d} m {a} rad"
        if k > 0:
            assert (ro["pairs"], ro["iterations"], ro["icp_state"]) == (rh["pairs"], rh["iterations"], rh["icp_state"]), f"scan {k}"
            assert (ro["valid_model"], ro["valid_scene"]) == (rh["valid_model"], rh["valid_scene"])
            assert bool(ro["pushed"]) == bool(rh["pushed"]) and bool(ro["reg_error"]) == bool(rh["reg_error"])
            pr = node.preregistration()
            assert pr is not None and pr["candidates"] == ro["pre"]["candidates"] > 0, (pr, k)
            assert (pr["valid_model"], pr["valid_scene"], pr["control"]) == (ro["pre"]["valid_model"], ro["pre"]["valid_scene"],
                                                                          ro["pre"]["control"])
            if pr["idx"] >= 0:
                assert 0.0 < pr["prob"] <= 1.0                     # bestRatio in the probability slot
            won += pr["idx"] >= 0
        pushes += rh["pushed"]
    assert pushes >= n // 2 and won > 0
    H.assert_grids_equal(loop.g.dump(), node.grid().download_tiles(), 1e-5)
    e = math.hypot(rh["pose"][0, 2] - poses[-1, 0], rh["pose"][1, 2] - poses[-1, 1])
    assert e < 0.1, f"tracking error {e} m"
    node.close()
