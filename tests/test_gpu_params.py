"""The kernels against the oracle away from the default node parameters (tests/param_points.py: truncation radius, max_range,
min_range, low_reflectivity_range).  The fp32 per-beam limit and the tile cull of the push (push_device.hpp), the launch window, the
batched push's own copy of both (push_multi.hip), the ray cast's negative-band mask, the map update's rectangle and the
relocalisation's scores all take these four numbers in; tests/test_cpu_params.py shows the oracle itself right at every point.

Bars: the push as tools/fuzz_parity.py demands it (statistics equal, tile flags / _initWeight / NaN pattern exact, cells with max abs
diff 0); the ray cast, the batch, the closed loop and the relocalisation with the bars of the tests they are named after.
"""
import contextlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, synth
from tests import helpers as H
from tests import param_points as PP
from tests import reloc_ref as R
from tests.slam_driver import HipSlamFused, slam_kwargs

pytestmark = pytest.mark.gpu

# every point on both shapes, the second shape once more on a device that shows two compute units (several tiles per workgroup)
CASES = [(s, p, None) for s in PP.SHAPES for p in PP.POINTS] + [("pillars9", p, 2) for p in PP.POINTS]
IDS = [f"{s}-{p}" + (f"-{c}cus" if c else "") for s, p, c in CASES]


@contextlib.contextmanager
def n_cus(n):
    """TSD_DEBUG_N_CUS in the environment around the creation of a context (read by tsd_create)"""
    old = os.environ.get("TSD_DEBUG_N_CUS")
    if n:
        os.environ["TSD_DEBUG_N_CUS"] = str(n)
    else:
        os.environ.pop("TSD_DEBUG_N_CUS", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("TSD_DEBUG_N_CUS", None)
        else:
            os.environ["TSD_DEBUG_N_CUS"] = old


def make_pair(oracle, shape, point, cus=None):
    gc = PP.grid_config(shape, point)
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    with n_cus(cus):
        dg = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    assert dg.max_trunc == og.max_trunc == max(PP.POINTS[point].trunc, 2) * gc.cell_size       # setMaxTruncation's clamp
    return og, dg


def pushed_pair(oracle, shape, point, cus=None, compare=False):
    """both grids after the case's five pushes, each side by its own push (the device's band mask is the push kernels' own);
    compare: statistics and the whole grid after every push"""
    og, dg = make_pair(oracle, shape, point, cus)
    P, geo = PP.POINTS[point], PP.geometry(shape)
    stats = []
    for k, (pose, (x, y, yaw), r32) in enumerate(PP.scans(shape, point)[:PP.N_PUSHES]):
        data, mask = oracle.ingest_f32(r32, P.max_range, geo.angle_increment)
        a = (pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
        so, sd = og.push(*a), dg.push(*a)
        stats.append(so)
        if compare:
            assert so == sd, f"push {k}: stats differ\n oracle {so}\n hip    {sd}"
            H.assert_grids_equal(og.dump(), dg.download_tiles(), 0.0)
        if k == 2:
            c = [x + PP.FOOTPRINT[0], y]
            assert og.free_footprint(c, *PP.FOOTPRINT[1:]) and dg.free_footprint(c, *PP.FOOTPRINT[1:])
            if compare:
                H.assert_grids_equal(og.dump(), dg.download_tiles(), 0.0)
    return og, dg, stats


def assert_raycast_equal(oracle, og, dg, shape, point, pose, what):
    P = PP.POINTS[point]
    rw = PP.raycast_rays(oracle, shape, point, pose)
    co, no, mo, cnt_o = og.raycast(pose, rw, P.min_range, P.max_range)
    cd, nd, md, cnt_d = dg.raycast(pose, rw, P.min_range, P.max_range)
    assert np.array_equal(mo, md), f"{what}: hit masks differ at beams {np.nonzero(mo != md)[0][:10]}"
    assert cnt_o == cnt_d, f"{what}: {cnt_o} / {cnt_d} hits"
    sel = np.repeat(mo.astype(bool), 2)
    if sel.any():
        assert np.max(np.abs(co[sel] - cd[sel])) <= 1e-9, f"{what}: coordinates"
        assert np.max(np.abs(no[sel] - nd[sel])) <= 1e-9, f"{what}: normals"
    return cnt_o


# ------------------------------------------------------------------------------------------------ push
@pytest.mark.parametrize("shape,point,cus", CASES, ids=IDS)
def test_push_matches_oracle(oracle, shape, point, cus):
    """k_push_tables, the classification, k_push_update and the halo pass: five pushes, a freed footprint after the third"""
    og, dg, stats = pushed_pair(oracle, shape, point, cus, compare=True)
    c = PP.counts_of(point, stats, PP.ORACLE_COUNTS[point][list(PP.SHAPES).index(shape)][3], PP.geometry(shape).beams)
    PP.assert_not_vacuous(point, c)
    assert (c["cells"], c["emptied"], c["culled"]) == PP.ORACLE_COUNTS[point][list(PP.SHAPES).index(shape)][:3]


@pytest.mark.parametrize("shape", list(PP.SHAPES))
def test_clamped_request_gives_the_minimum_grid(oracle, shape):
    """a request below 2 cells: tsd_create reports 2 cells, and the grid equals trunc_min's bit for bit"""
    _, da, _ = pushed_pair(oracle, shape, "trunc_clamped")
    _, db, _ = pushed_pair(oracle, shape, "trunc_min")
    assert da.max_trunc == db.max_trunc == 2 * da.cell_size
    for x, y in zip(da.download_tiles(), db.download_tiles()):
        assert np.array_equal(x, y, equal_nan=True)
    assert da.digest() == db.digest()


# ------------------------------------------------------------------------------------------------ ray cast
@pytest.mark.parametrize("shape,point,cus", CASES, ids=IDS)
def test_raycast_matches_oracle(oracle, shape, point, cus):
    """from pose 5, from outside the grid and -- at trunc_min and trunc_tile -- from behind a wall, where the beams start inside the
    negative band and the miss event (prev < 0 < cur) has to end them as in the oracle"""
    og, dg, _ = pushed_pair(oracle, shape, point, cus)
    geo = PP.geometry(shape)
    cnt = assert_raycast_equal(oracle, og, dg, shape, point, PP.scans(shape, point)[PP.RAYCAST_K][0], "pose 5")
    assert cnt >= PP.MIN_HIT_SHARE * geo.beams and cnt == PP.ORACLE_COUNTS[point][list(PP.SHAPES).index(shape)][3]
    assert_raycast_equal(oracle, og, dg, shape, point, PP.outside_pose(shape), "outside")
    if point in ("trunc_min", "trunc_tile"):
        pose = PP.behind_wall_pose(shape, point)
        st, v = og.bilinear(pose[0, 2], pose[1, 2])
        assert st == 0 and v < 0, "the pose behind the wall is not in the negative band"
        assert_raycast_equal(oracle, og, dg, shape, point, pose, "behind the wall")


# ------------------------------------------------------------------------------------------------ maps, image, digest, text file
@pytest.mark.parametrize("shape,point", [(s, p) for s in PP.SHAPES for p in PP.POINTS])
def test_maps_image_digest_and_text_file_match_oracle(oracle, shape, point, tmp_path):
    og, dg, _ = pushed_pair(oracle, shape, point)
    N = dg.cells
    for inflate in (False, True):
        content = np.full(N * N, -1, dtype=np.int8)
        oo, no = og.occupancy(content, inflate, 2)
        od, nd = dg.occupancy(inflate, 2)
        assert no == nd and no > 0, f"inflate {inflate}: surface counts {no} / {nd}"
        assert np.array_equal(oo.reshape(N, N), od), f"inflate {inflate}: {np.count_nonzero(oo.reshape(N, N) != od)} cells differ"
    for (w, h) in ((N, N), (300, 200)):
        assert np.array_equal(og.color_image(w, h), dg.color_image(w, h)), f"colour image {w} x {h}"
    do, dd = og.digest(), dg.digest()
    assert do["hash"] == dd["hash"] and do["cells_valid"] == dd["cells_valid"] > 0 and do["tiles_initialized"] == dd["tiles_initialized"]
    assert abs(do["sum_tsd"] - dd["sum_tsd"]) <= 1e-9 * max(1.0, abs(do["sum_tsd"]))
    assert abs(do["sum_weight"] - dd["sum_weight"]) <= 1e-9 * max(1.0, abs(do["sum_weight"]))
    fo, fh = tmp_path / "oracle.grid", tmp_path / "hip.grid"
    assert og.store_text(fo)
    dg.store_text(fh)
    bo = fo.read_bytes()
    assert bo == fh.read_bytes() and len(bo) > 1000
    assert float(bo.split(b"\n")[3]) == pytest.approx(og.max_trunc, rel=1e-5)          # (%g: 6 digits of the truncation)


@pytest.mark.parametrize("shape", list(PP.SHAPES))
def test_load_text_adopts_the_files_truncation(oracle, shape, tmp_path):
    """a file written at trunc_wide loaded into a context created at the default: the context reports the file's truncation and
    equals the oracle's loaded grid cell for cell -- and the next push and ray cast work with the adopted band"""
    og, dg, _ = pushed_pair(oracle, shape, "trunc_wide")
    f = tmp_path / "wide.grid"
    dg.store_text(f)
    gc = PP.grid_config(shape, "default")
    other = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    assert other.max_trunc == 3 * gc.cell_size
    other.load_text(f)
    og2 = oracle.Grid.load_text(f, gc.cell_size)
    want = float(f.read_bytes().split(b"\n")[3])
    assert other.lib.tsd_max_truncation(other.h) == og2.max_trunc == want and abs(want - 12 * gc.cell_size) < 1e-6 * want
    H.assert_grids_equal(og2.dump(), other.download_tiles(), 0.0)
    P, geo = PP.POINTS["trunc_wide"], PP.geometry(shape)
    pose, _, r32 = PP.scans(shape, "trunc_wide")[PP.RAYCAST_K]
    data, mask = oracle.ingest_f32(r32, P.max_range, geo.angle_increment)
    a = (pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
    assert og2.push(*a) == other.push(*a)
    H.assert_grids_equal(og2.dump(), other.download_tiles(), 0.0)
    assert_raycast_equal(oracle, og2, other, shape, "trunc_wide", PP.scans(shape, "trunc_wide")[4][0], "after the load")


# ------------------------------------------------------------------------------------------------ batched push
@pytest.mark.parametrize("multi", [True, False])
def test_batch_with_a_row_of_ranges_per_sensor(oracle, multi):
    """k_mp_update: three sensors on one grid, each with its own max_range / min_range / low_refl (default, short_sensor,
    lowrefl_beyond), the grid's truncation (5 cells) shared; against the same order on the oracle's primitives, with the bars of
    test_gpu_batch.py, once in one pass per tile and once as serial pushes"""
    from tests.test_gpu_batch import OFFSETS, Robot, _compare
    gc0, geo, scene = synth.CONFIGS["cfg1"]
    gc = synth.GridConfig(gc0.map_size_log2, gc0.cell_size, 5)
    geo_msg = synth.ScanGeometry(geo.beams, float(np.float32(geo.angle_min)), float(np.float32(geo.angle_increment)))
    rows = [PP.POINTS[n] for n in ("default", "short_sensor", "lowrefl_beyond")]
    kws = [slam_kwargs(gc, geo_msg, max_range=r.max_range, min_range=r.min_range, low_refl_range=r.low_refl) for r in rows]
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    dg = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    dg.set_push_multi(multi)
    n_scans = 8
    robots, scans, sensors = [], [], []
    # (3 to 4 m from the room's left and lower wall: two walls at right angles inside every sensor's 7 m, beyond its min_range)
    offsets = [(o[0] - 4.5, o[1] - 2.8, o[2]) for o in OFFSETS[:3]]
    for off, kw in zip(offsets, kws):
        w = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
        scans.append(synth.scans_for(w, geo, synth.trajectory(w, n_scans, yaw0=off[2])))
        robots.append(Robot(oracle, gc, geo, off, kw))
    for rb, sc in zip(robots, scans):
        rb.init_both(og, dg, sc[0])
    H.assert_grids_equal(og.dump(), dg.download_tiles(), 0.0)
    for rb, kw in zip(robots, kws):
        s = capi.TsdSensorDevice(dg, geo.beams, kw["angle_increment"], kw["angle_min"], kw["max_range"], kw["min_range"], kw["low_refl_range"])
        s.set_pose(rb.pose, rb.rays, rb.rays_local)
        sensors.append(s)
    params = dg.icp_params(kws[0]["icp_iterations"], kws[0]["dist_filter_max"], kws[0]["dist_filter_min"])
    gates = capi.GateParams(kws[0]["reg_trs_max"], kws[0]["reg_sin_rot_max"], 0.05, 0.03)
    batch = capi.TsdBatch(dg, len(robots))
    bounds = (dg.min_x, dg.max_x, dg.min_y, dg.max_y)
    pushed = [0] * len(robots)
    for k in range(1, n_scans):
        ing = [rb.ingest(sc[k]) for rb, sc in zip(robots, scans)]
        ros = [rb.localise(og, d_, m_, bounds) for rb, (d_, m_, _) in zip(robots, ing)]
        for rb in robots:
            rb.apply_push(og)
        batch.begin(sensors, [x[0] for x in ing], [x[1] for x in ing], [x[2] for x in ing], params, gates)
        for i, (ro, sr) in enumerate(zip(ros, batch.results())):
            _compare(k, i, ro, sr)
            pushed[i] += ro["pushed"]
        H.assert_grids_equal(og.dump(), dg.download_tiles(), 1e-5)
    assert all(n >= 3 for n in pushed), f"pushes per robot {pushed}: the batched push had nothing to do"
    batch.close()
    for s in sensors:
        s.close()


# ------------------------------------------------------------------------------------------------ fused scan
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("point", ["trunc_min", "trunc_wide", "short_sensor"])
def test_fused_scan_closed_loop(oracle, point, mode):
    """tsd_scan: a 12-scan closed loop through HipSlamFused against the oracle's loop with the bars of test_closed_loop_trajectory
    (the second shape: its pillars keep a 7 m sensor observable in x and y); mode 3: the TSD_PDF pre-registration inside the scan"""
    shape = "pillars9"
    P, gc, geo = PP.POINTS[point], PP.grid_config(shape, point), PP.geometry(shape)
    world = synth.World(PP.SHAPES[shape][2], gc)
    poses = synth.trajectory(world, 12)
    scans = synth.scans_for(world, geo, poses)
    trials, ctrl, zrand, phimax = 100, 140, 0.25, 30.0
    kw = slam_kwargs(gc, geo, truncation_radius=P.trunc, max_range=P.max_range, min_range=P.min_range, low_refl_range=P.low_refl,
                     registration_mode=mode, trials=trials, size_control_set=ctrl, zrand=zrand, ransac_phi_max=phimax)
    so = oracle.Slam(**kw)
    sh = HipSlamFused(oracle, **kw)
    assert sh.grid.max_trunc == so.grid.max_trunc == P.trunc * gc.cell_size
    rng = np.random.default_rng(31 + mode)
    pushes = 0
    for k in range(len(scans)):
        if mode == 3 and k > 0:
            draws = tuple(rng.integers(0, 2 ** 31 - 1, n).astype(np.int32) for n in (geo.beams, ctrl, trials))
            so.set_draws(*draws)
            r = np.array(scans[k], dtype=np.float32)
            r[r < kw["laser_min_range"]] = 0.0
            data, mask = oracle.ingest_f32(r, kw["max_range"], geo.angle_increment)
            scn, ms, _ = oracle.scene_from_scan(sh.rays_local, data, mask)
            sh.sensor.preregister(scn, ms, trials, ctrl, zrand, math.radians(phimax), geo.angle_increment, *draws)
        ro = so.process_scan(scans[k])
        rh = sh.process_scan(scans[k])
        Po = np.array(ro.pose[:]).reshape(3, 3)
        d, a = H.pose_delta(Po, rh["pose"])
        assert d <= 1e-4 and a <= 1e-4, f"scan {k}: {d} {a}"
        assert ro.pushed == rh["pushed"] and ro.reg_error == rh["reg_error"]
        if k > 0:
            assert ro.pairs == rh["pairs"] and ro.valid_model == rh["valid_model"]
            assert np.hypot(Po[0, 2] - poses[k, 0], Po[1, 2] - poses[k, 1]) < 0.15          # tracks ground truth
        pushes += ro.pushed
    assert pushes >= 6
    oi, oiw, ot, ow = so.grid.dump()
    gi, giw, gt, gw = sh.grid.download_tiles()
    assert np.array_equal(oi, gi)
    sel = oi.astype(bool)
    m = ~np.isnan(ot[sel])
    assert np.array_equal(np.isnan(ot[sel]), np.isnan(gt[sel]))
    assert np.max(np.abs(ot[sel][m] - gt[sel][m])) <= 1e-5
    assert np.max(np.abs(ow[sel] - gw[sel])) <= 1e-5


# ------------------------------------------------------------------------------------------------ map update window
@pytest.mark.parametrize("inflate", [False, True])
@pytest.mark.parametrize("point", ["trunc_tile", "short_sensor"])
def test_map_update_window_holds_every_cell_that_changed(oracle, point, inflate):
    """a frame, two more pushes, then tsd_map_update: the window pasted over the previous full frame equals a fresh full extraction
    (tsd_occupancy / tsd_color_image on the same context).  A reach that forgot the band would lose the cells at its rim."""
    shape = "pillars9"
    dg = make_pair(oracle, shape, point)[1]
    P, geo, N = PP.POINTS[point], PP.geometry(shape), dg.cells
    updates = []
    for k, (pose, (x, y, yaw), r32) in enumerate(PP.scans(shape, point)[:PP.N_PUSHES]):
        data, mask = oracle.ingest_f32(r32, P.max_range, geo.angle_increment)
        dg.push(pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl, want_stats=False)
        if k == 2:
            occ, rgb, _ = dg.map_frame(inflate, 2)
            updates.append(((0, 0, N, N), occ, rgb))
    win, occ, rgb, ns = dg.map_update(inflate, 2)
    want, _ = dg.occupancy(inflate, 2)
    img = dg.color_image(N, N)
    assert win[2] > 0 and win[3] > 0
    assert np.array_equal(occ, want), f"window {win}: {np.count_nonzero(occ != want)} cells differ at {np.argwhere(occ != want)[:4]}"
    assert np.array_equal(rgb, img), f"window {win}: image differs at {np.argwhere(rgb != img)[:4]}"
    assert not np.array_equal(updates[0][1], want), "the two pushes changed nothing in the map"
    if point == "short_sensor":
        assert win[2] < N or win[3] < N, f"a 7 m sensor on a 25.6 m grid: window {win}"


# ------------------------------------------------------------------------------------------------ relocalisation
def _reloc_scene(oracle, point):
    """reloc_ref.scene(1081) at another truncation, with the smallest lattice test_gpu_reloc.py searches (5 x 5 positions; 7 rotations)"""
    P, gc, geo = PP.POINTS[point], PP.grid_config("pillars9", point), PP.geometry("pillars9")
    world = synth.World("pillars", gc)
    grid = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for p in synth.trajectory(world, R.PUSHED, step_x=0.25, step_yaw=0.01):
        data, mask = oracle.ingest_f32(world.scan(p[0], p[1], p[2], geo), P.max_range, geo.angle_increment)
        grid.push(synth.pose_matrix(*p), data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
    truth = (world.start[0] + R.TRUTH_OFFSET[0], world.start[1] + R.TRUTH_OFFSET[1], R.TRUTH_OFFSET[2])
    rays_local = oracle.rays_local(geo.beams, geo.angle_min, geo.angle_increment)
    data, mask = oracle.ingest_f32(world.scan(*truth, geo), P.max_range, geo.angle_increment)
    scene_xy, ms, _ = oracle.scene_from_scan(rays_local, data, mask)
    points = scene_xy.reshape(-1, 2)[ms.astype(bool)].copy()
    lat = dict(x0=truth[0] - 2.4 * R.STEP, y0=truth[1] - 1.7 * R.STEP, nx=5, ny=5)
    table = R.rotation_table(7, truth[2] - 3.3 * R.DTHETA, R.DTHETA)
    return gc, grid, truth, rays_local, data, mask, points, lat, table


@pytest.mark.parametrize("point", ["trunc_min", "trunc_wide"])
def test_relocalize_scores_and_pose(oracle, point):
    """tsd_relocalize scores poses on TSD values whose scale is max_trunc: the score volume against tests/reloc_ref.py, uint32 for
    uint32, and the refined pose inside test_relocalize_finds_the_pose's bar"""
    P = PP.POINTS[point]
    gc, grid, truth, rays_local, data, mask, points, lat, table = _reloc_scene(oracle, point)
    dump = grid.dump()
    want, gate = R.scores(R.GridView(dump, grid.cells, gc.cell_size), points, lat["x0"], lat["y0"], R.STEP, lat["nx"], lat["ny"], table)
    assert gate.any() and want.max() > 0 and len(np.unique(want)) > 20
    g = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    g.upload_tiles(*dump)
    out = g.relocalize(points, rays_local, data, mask, P.min_range, P.max_range,
                       g.icp_params(R.ICP["iterations"], R.ICP["dist_max"], R.ICP["dist_min"]), x0=lat["x0"], y0=lat["y0"],
                       step_xy=R.STEP, nx=lat["nx"], ny=lat["ny"], ntheta=len(table), cos_sin=table, theta_wraps=False, K=16,
                       min_pairs=len(points) // 4)
    got = g.debug_reloc_scores().reshape(len(table), lat["ny"], lat["nx"])
    assert np.array_equal(got, want)
    assert out["found"]
    d, a = R.pose_error(out["pose"], truth)
    assert d <= 0.5 * R.STEP and a <= 0.5 * R.DTHETA, f"relocalised {d} m, {a} rad from the truth"


# ------------------------------------------------------------------------------------------------ truncation of a live grid
@pytest.mark.parametrize("shape", list(PP.SHAPES))
def test_truncation_changed_on_a_live_grid(oracle, shape):
    """three pushes at 3 cells, setMaxTruncation(6 cells), three more: pushes, ray cast and occupancy equal the oracle's"""
    og, dg = make_pair(oracle, shape, "default")
    P, geo, cs = PP.POINTS["default"], PP.geometry(shape), dg.cell_size
    for k, (pose, _, r32) in enumerate(PP.scans(shape, "default")):
        if k == 3:
            assert og.set_max_truncation(6 * cs) == dg.set_max_truncation(6 * cs) == 6 * cs == dg.lib.tsd_max_truncation(dg.h)
        data, mask = oracle.ingest_f32(r32, P.max_range, geo.angle_increment)
        a = (pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
        so, sd = og.push(*a), dg.push(*a)
        assert so == sd, f"push {k}: stats differ\n oracle {so}\n hip    {sd}"
        H.assert_grids_equal(og.dump(), dg.download_tiles(), 0.0)
    cnt = assert_raycast_equal(oracle, og, dg, shape, "default", PP.scans(shape, "default")[4][0], "after the change")
    assert cnt >= PP.MIN_HIT_SHARE * geo.beams
    assert_raycast_equal(oracle, og, dg, shape, "default", PP.outside_pose(shape), "outside")
    N = dg.cells
    for inflate in (False, True):
        oo, no = og.occupancy(np.full(N * N, -1, dtype=np.int8), inflate, 2)
        od, nd = dg.occupancy(inflate, 2)
        assert no == nd > 0 and np.array_equal(oo.reshape(N, N), od)


def test_setter_below_two_cells_reports_the_minimum(oracle):
    og, dg = make_pair(oracle, "room8", "trunc_wide")
    cs = dg.cell_size
    for req in (1.0 * cs, 0.0, -1.0, 1.999 * cs):
        assert dg.set_max_truncation(req) == og.set_max_truncation(req) == 2 * cs
        assert dg.lib.tsd_max_truncation(dg.h) == 2 * cs
    assert dg.set_max_truncation(2.5 * cs) == og.set_max_truncation(2.5 * cs) == 2.5 * cs


def test_map_update_after_a_truncation_change_covers_the_grid(oracle):
    """tsd_set_max_truncation clears frame_prev_valid: the next update is the whole map, and right"""
    shape = "pillars9"
    dg = make_pair(oracle, shape, "short_sensor")[1]
    P, geo, N = PP.POINTS["short_sensor"], PP.geometry(shape), dg.cells
    sc = PP.scans(shape, "short_sensor")

    def push(k):
        data, mask = oracle.ingest_f32(sc[k][2], P.max_range, geo.angle_increment)
        dg.push(sc[k][0], data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl, want_stats=False)

    push(0)
    dg.map_frame(False, 2)
    push(1)
    win, occ, rgb, _ = dg.map_update(False, 2)
    assert win[2] > 0 and win[3] > 0 and (win[2] < N or win[3] < N)       # windowed while nothing but pushes happened
    dg.set_max_truncation(6 * dg.cell_size)
    push(2)
    win, occ, rgb, _ = dg.map_update(False, 2)
    assert win == (0, 0, N, N)
    assert np.array_equal(occ, dg.occupancy(False, 2)[0]) and np.array_equal(rgb, dg.color_image(N, N))


# ------------------------------------------------------------------------------------------------ randomised
def test_randomised_parity_sweep_with_random_parameters():
    """tools/fuzz_parity.py ... params: the four parameters drawn per case (truncation 1-40 cells, max_range 3-30, min_range 0.001-3,
    low_refl 0-12) on top of the hard cases; 24 cases here, a longer run in profiles/params_fuzz_parity.txt"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "24", "5100", "hard", "params"], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "all 24 cases ok" in p.stdout
