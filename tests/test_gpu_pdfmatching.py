"""GPU tests of registration_mode 2: the PDFMatching pre-registration (PDFMatching.cpp:47-487) on the device (tsd_pdf_match)
against the plain-C restatement tests/pdfmatch_restate.c for identical rand() draws, and ThreadLocalize in mode 2 (ray cast ->
PDFMatching::match -> Icp::iterate with its result as Tinit, ThreadLocalize.cpp:545-553) against a test-side loop of the
oracle's primitives.  Counts, winners and field-of-view counts exact; T / products to rounding (the device's atan2, pow and
cos / sin differ from libm's in the last bits)."""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import helpers as H
from tests import pdfmatch_ref as R
from tests.slam_driver import slam_kwargs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return R.Restatement(R.build(tmp_path_factory.mktemp("pdfr")))


_SCENES = {}


def _scene(oracle, cfg):
    if cfg not in _SCENES:
        _SCENES[cfg] = R.oracle_scene(oracle, cfg)
    return _SCENES[cfg]


def _context():
    gc = synth.CONFIGS["cfg1"][0]                    # (mode 2 reads no grid: the smallest context)
    return capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)


def _draws(seed, beams, ctrl, trials):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 2 ** 31 - 1, n) for n in (beams, ctrl, trials))


def _model_angles_sorted(M, mask):
    xy = np.asarray(M).reshape(-1, 2)[np.asarray(mask).astype(bool)]
    return bool(np.all(np.diff(np.arctan2(xy[:, 1], xy[:, 0])) >= 0.0))


def _gated(rr, pct):
    return np.where(rr["fov"].astype(np.float64) > float(rr["control"]) * pct, rr["ungated"], 0.0)


def _compare(dg, rr, rh, pct=capi.PDFMATCH_DEFAULTS["percentage_points_in_c"]):
    """device == restatement: counts and field-of-view counts exact, products to 1e-12 relative, the winner exact unless the
    restatement's two best gated products are a near-tie (then either may win, and the test checks that it is one)"""
    for k in ("candidates", "valid_model", "valid_scene", "control"):
        assert rh[k] == rr[k], (k, rh[k], rr[k])
    u, f = dg.debug_pdf_match_scores()
    assert len(u) == rr["candidates"] and np.array_equal(f, rr["fov"]), np.nonzero(f != rr["fov"])[0][:10]
    ru = rr["ungated"]
    rel = np.abs(u - ru) / np.maximum(np.abs(ru), 1e-300)
    assert np.all((rel <= 1e-12) | ((ru == 0.0) & (u == 0.0))), (np.count_nonzero(rel > 1e-12), rel.max())
    if (rh["idx"], rh["i"]) != (rr["idx"], rr["i"]):
        g = _gated(rr, pct)
        top = g.max()
        assert top > 0.0 and np.count_nonzero(g >= top * (1.0 - 1e-12)) >= 2, ("different winner without a tie", rh, rr)
        assert abs(rh["prob"] - top) <= 1e-12 * top
        return False
    assert abs(rh["prob"] - rr["prob"]) <= 1e-9 * rr["prob"]
    assert np.max(np.abs(rh["T"] - rr["T"])) <= 1e-12
    return True


# >= 20 seeds over the cfg 1 (360 degrees, 1 degree beams) and cfg 2 (270 degrees, 0.25 degree beams) geometries, trials 30 / 100 /
# 600 and phiMax 30 / 90 degrees
_CASES = ([("cfg1", t, p, s) for (t, p) in ((30, 30.0), (100, 30.0), (100, 90.0), (600, 90.0)) for s in (1, 2, 3)] +
          [("cfg2", t, p, s) for (t, p) in ((30, 30.0), (100, 30.0), (100, 90.0)) for s in (4, 5, 6)] + [("cfg2", 600, 30.0, 7)])


@pytest.mark.parametrize("cfg,trials,phi_deg,seed", _CASES)
def test_pdf_match_matches_restatement(oracle, restate, cfg, trials, phi_deg, seed):
    sc = _scene(oracle, cfg)
    geo = sc["geo"]
    # cfg 2's model angles rise with the beam index (the device bisects); cfg 1's 360-degree model wraps at +-pi (the linear scan)
    assert _model_angles_sorted(sc["M"], sc["mask_m"]) == (cfg == "cfg2")
    ds, dc, dt = _draws(seed, geo.beams, 140, trials)
    phi = math.radians(phi_deg)
    args = (sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, geo.angle_increment, ds, dc, dt)
    rr = restate.match(*args, trials=trials)
    dg = _context()
    rh = dg.pdf_match(*args, trials=trials)
    assert rr["rc"] == 0 and rr["candidates"] > 100
    _compare(dg, rr, rh)
    assert rh["idx"] >= 0 and rh["prob"] > 0.0


def test_pdf_match_winner_decided_by_the_gate(oracle, restate):
    """percentagePointsInC set so that the largest product does NOT see enough of the control set: the gated winner is another
    candidate (PDFMatching.cpp:373), on the device as in the restatement"""
    sc = _scene(oracle, "cfg1")
    geo = sc["geo"]
    ds, dc, dt = _draws(11, geo.beams, 140, 100)
    args = (sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], math.radians(30.0), geo.angle_increment, ds, dc, dt)
    mad = 0.5                                                   # maxAngleDiff (degrees): the counts differ between candidates
    r0 = restate.match(*args, percentage_points_in_c=0.0, max_angle_diff=mad)
    top = int(np.argmax(r0["ungated"]))
    f_top = int(r0["fov"][top])
    assert np.any(r0["fov"] > f_top), "no candidate sees more of the control set than the best product"
    pct = (f_top + 0.5) / r0["control"]
    rr = restate.match(*args, percentage_points_in_c=pct, max_angle_diff=mad)
    g = _gated(rr, pct)
    assert rr["prob"] > 0.0 and rr["prob"] < r0["ungated"][top] and g[top] == 0.0
    dg = _context()
    rh = dg.pdf_match(*args, percentage_points_in_c=pct, max_angle_diff=mad)
    assert _compare(dg, rr, rh, pct)
    assert rh["prob"] < r0["ungated"][top]


@pytest.mark.parametrize("seed", [21, 22])
def test_pdf_match_non_monotone_model_takes_the_linear_scan(oracle, restate, seed):
    """the whole scene turned by 100 degrees: the model's polar angles wrap at +-pi inside the list (a 360-degree scanner), so the
    device cannot bisect and has to scan all model angles like the reference"""
    sc = _scene(oracle, "cfg1")
    geo = sc["geo"]
    c, s = math.cos(math.radians(100.0)), math.sin(math.radians(100.0))
    rot = lambda P: (np.asarray(P).reshape(-1, 2) @ np.array([[c, s], [-s, c]])).reshape(-1)
    M, S = rot(sc["M"]), rot(sc["S"])
    assert not _model_angles_sorted(M, sc["mask_m"])
    ds, dc, dt = _draws(seed, geo.beams, 140, 100)
    args = (M, sc["mask_m"], S, sc["mask_s"], math.radians(30.0), geo.angle_increment, ds, dc, dt)
    rr = restate.match(*args)
    dg = _context()
    rh = dg.pdf_match(*args)
    assert rr["candidates"] > 100
    _compare(dg, rr, rh)


def test_pdf_match_degenerate_inputs(oracle, restate):
    sc = _scene(oracle, "cfg1")
    geo = sc["geo"]
    ds, dc, dt = _draws(9, geo.beams, 140, 100)
    dg = _context()
    phi, res = math.radians(30.0), geo.angle_increment
    # n < 3 (:61-65)
    rh = dg.pdf_match(sc["M"][:4], sc["mask_m"][:2], sc["S"][:4], sc["mask_s"][:2], phi, res, ds, dc, dt)
    rr = restate.match(sc["M"][:4], sc["mask_m"][:2], sc["S"][:4], sc["mask_s"][:2], phi, res, ds, dc, dt)
    assert rr["rc"] == 1 and np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1 and rh["candidates"] == 0
    # fewer than 3 valid points in scene / model (:134-144)
    z = np.zeros_like(sc["mask_m"])
    for mm, ms in ((sc["mask_m"], z), (z, sc["mask_s"])):
        rh = dg.pdf_match(sc["M"], mm, sc["S"], ms, phi, res, ds, dc, dt)
        rr = restate.match(sc["M"], mm, sc["S"], ms, phi, res, ds, dc, dt)
        assert rr["rc"] == 1 and np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1
        assert (rh["valid_model"], rh["valid_scene"], rh["control"]) == (rr["valid_model"], rr["valid_scene"], rr["control"])
    # resolution not set (:161-171): identity, no error
    rh = dg.pdf_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, 0.0, ds, dc, dt)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, 0.0, ds, dc, dt)
    assert rr["rc"] == 2 and np.array_equal(rh["T"], np.eye(3)) and rh["candidates"] == 0
    assert (rh["valid_model"], rh["valid_scene"]) == (rr["valid_model"], rr["valid_scene"]) and rh["valid_model"] >= 3
    # an empty control set: every product is 0 (probOfAllScans.size() == 0, :359-363), nothing wins
    rh = dg.pdf_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=0)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=0)
    assert rr["candidates"] > 0 and rh["control"] == 0
    _compare(dg, rr, rh)
    assert np.array_equal(rh["T"], np.eye(3)) and rh["idx"] == -1 and rh["prob"] == 0.0
    # and a tiny control set still matches
    rh = dg.pdf_match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=3, trials=5)
    rr = restate.match(sc["M"], sc["mask_m"], sc["S"], sc["mask_s"], phi, res, ds, dc, dt, size_control_set=3, trials=5)
    _compare(dg, rr, rh)


def _libc_draws(seed, n_sub, n_ctrl, n_trials):
    """what the facade's PDFMatching::match draws for `tsdpdf_seed` >= 0: srand(seed + call), then rand()"""
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    return ([libc.rand() for _ in range(n_sub)], [libc.rand() for _ in range(n_ctrl)], [libc.rand() for _ in range(n_trials)])


class _Mode2Loop:
    """ThreadLocalize::init + eventLoop body in registration_mode 2 on the oracle's primitives (ray cast, scene points, Icp::iterate
    with Tinit, gates, push) with the restatement as PDFMatching::match"""

    def __init__(self, oracle, restate, kw, mode2):
        self.o, self.r, self.kw, self.m2 = oracle, restate, kw, mode2
        self.g = oracle.Grid(kw["map_size_log2"], kw["cell_size"], kw["truncation_radius"] * kw["cell_size"])
        self.initialized = False
        self.draws = None

    def process_scan(self, ranges_f32):
        o, kw, g = self.o, self.kw, self.g
        r = np.array(ranges_f32, dtype=np.float32)
        r[r < kw["laser_min_range"]] = 0.0
        B, res, phi_min = kw["beams"], kw["angle_increment"], kw["angle_min"]
        out = dict(pushed=0, reg_error=0, pairs=0, iterations=0, icp_state=0, valid_model=0, valid_scene=0, pre=None)
        if not self.initialized:
            W = (1 << kw["map_size_log2"]) * kw["cell_size"]
            phi = kw["local_offset_yaw"]
            sx = W * 0.5 + kw["x_offset"] + kw["local_offset_x"]
            sy = W * 0.5 + kw["y_offset"] + kw["local_offset_y"]
            Tinit = np.array([[math.cos(phi), -math.sin(phi), sx], [math.sin(phi), math.cos(phi), sy], [0, 0, 1.0]])
            self.rays_local = o.rays_local(B, phi_min, res)
            self.rays = o.rays_transform(Tinit, self.rays_local)
            self.ray_norm = 1.0
            self.pose = o.mat3_mul(np.eye(3), Tinit)
            self.data, self.mask = o.ingest_f32(r, kw["max_range"], res)
            g.free_footprint([sx + kw["footprint_x_offset"], sy], kw["footprint_width"], kw["footprint_height"])
            g.push(self.pose, self.data, self.mask, res, phi_min, kw["max_range"], kw["min_range"], kw["low_refl_range"])
            self.initialized = True
            self.last_pose = None
            out.update(pose=self.pose.copy(), pushed=1)
            return out
        self.data, self.mask = o.ingest_f32(r, kw["max_range"], res)
        if self.last_pose is None:
            self.last_pose = self.pose.copy()
        self.rays = o.rays_rescale(self.rays, kw["cell_size"], self.ray_norm)
        self.ray_norm = kw["cell_size"]
        co, no, mo, cnt = g.raycast(self.pose, self.rays, kw["min_range"], kw["max_range"])
        out["valid_model"] = cnt
        if cnt == 0:
            out.update(pose=self.pose.copy(), no_model=1)
            return out
        scene, ms, ns = o.scene_from_scan(self.rays_local, self.data, self.mask)
        out["valid_scene"] = ns
        pre = self.r.match(co, mo, scene, ms, kw["ransac_phi_max"] * math.pi / 180.0, res, *self.draws, **self.m2)   # (as the node: * M_PI / 180.0)
        out["pre"] = pre
        M = co.reshape(-1, 2)[mo.astype(bool)]
        S = scene.reshape(-1, 2)[ms.astype(bool)]
        ri = o.icp_init(M, S, self.pose, kw["icp_iterations"], kw["dist_filter_max"], kw["dist_filter_min"],
                        (0.0, g.max_x, 0.0, g.max_x), pre["T"], nn_mode=kw["nn_mode"])
        T = ri["T"]
        out.update(pairs=ri["pairs"], iterations=ri["iterations"], icp_state=ri["state"])
        Tf = o.f64(T).reshape(9)
        if o.lib().ora_is_registration_error(o.d(Tf), kw["reg_trs_max"], kw["reg_sin_rot_max"]):
            out.update(pose=self.pose.copy(), reg_error=1)
            return out
        self.rays = o.rays_transform(T, self.rays)
        self.pose = o.mat3_mul(self.pose, T)
        out["pose"] = self.pose.copy()
        lp, cp = o.f64(self.last_pose).reshape(9), o.f64(self.pose).reshape(9)
        if o.lib().ora_is_pose_change_significant(o.d(lp), o.d(cp)):
            self.last_pose = self.pose.copy()
            d2, m2 = o.ingest_f64(self.data, kw["max_range"], res)
            g.push(self.pose, d2, m2, res, phi_min, kw["max_range"], kw["min_range"], kw["low_refl_range"])
            out["pushed"] = 1
        return out


@pytest.mark.parametrize("cfg,n", [("cfg1", 12), ("cfg2", 10)])
def test_facade_registration_mode_2_matches_the_test_loop(oracle, restate, cfg, n):
    """ThreadLocalize with registration_mode 2 (before this mode existed on the device the node fell back to plain ICP and had no
    pre-registration to report): the whole closed loop against the test-side loop, both fed the same rand() draws"""
    gc, geo, scene = synth.CONFIGS[cfg]
    world = synth.World(scene, gc)
    poses = synth.trajectory(world, n)
    scans = synth.scans_for(world, geo, poses)
    geo_msg = synth.ScanGeometry(geo.beams, float(np.float32(geo.angle_min)), float(np.float32(geo.angle_increment)))
    trials, ctrl, phimax, seed = 100, 140, 30.0, 4711
    kw = slam_kwargs(gc, geo_msg, ransac_phi_max=phimax)
    node_keys = dict(zhit=0.45, zphi=0.0, zshort=0.25, zmax=0.05, zrand=0.25, percentagePointsInC=0.9, rangemax=20.0,
                     sigphi=math.pi / 180.0 * 3, sighit=0.2, lamshort=0.08, maxAngleDiff=3.0, maxAnglePenalty=0.5)
    m2 = dict(trials=trials, size_control_set=ctrl, zhit=0.45, zphi=0.0, zshort=0.25, zmax=0.05, zrand=0.25,
              percentage_points_in_c=0.9, rangemax=20.0, sigphi=math.pi / 180.0 * 3, sighit=0.2, lamshort=0.08,
              max_angle_diff=3.0, max_angle_penalty=0.5)
    loop = _Mode2Loop(oracle, restate, kw, m2)
    params = facade.node_params(gc, geo)
    params.update({"registration_mode": 2, "trials": trials, "sizeControlSet": ctrl, "ransac_phi_max": phimax, "tsdpdf_seed": seed},
                  **node_keys)
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
            won += pr["idx"] >= 0
        pushes += rh["pushed"]
    assert pushes >= n // 2 and won > 0
    H.assert_grids_equal(loop.g.dump(), node.grid().download_tiles(), 1e-5)
    e = math.hypot(rh["pose"][0, 2] - poses[-1, 0], rh["pose"][1, 2] - poses[-1, 1])
    assert e < 0.1, f"tracking error {e} m"
    node.close()
