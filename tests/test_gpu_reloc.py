"""tsd_relocalize on the device against the numpy restatement of tests/reloc_ref.py (whose fairness tests/test_cpu_reloc.py shows):
scores uint32 for uint32, peaks index for index, the refined pose bit for bit against tsd_localize, and the facade's start in a
stored map."""
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import reloc_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -5


def make_grid(sc):
    g = capi.TsdGridDevice(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
    g.upload_tiles(*sc.dump)
    return g


def icp_params(g):
    return g.icp_params(R.ICP["iterations"], R.ICP["dist_max"], R.ICP["dist_min"])


def reloc(g, sc, points=None, **kw):
    a = dict(x0=sc.x0, y0=sc.y0, step_xy=R.STEP, nx=R.NXY, ny=R.NXY, ntheta=R.NTHETA, cos_sin=sc.table, theta_wraps=True, K=16)
    a.update(kw)
    return g.relocalize(sc.points if points is None else points, sc.rays_local, sc.data, sc.mask, R.MIN_RANGE, R.MAX_RANGE,
                        icp_params(g), **a)


def device_volume(g, nt, ny, nx):
    return g.debug_reloc_scores().reshape(nt, ny, nx)


@pytest.mark.parametrize("beams", [360, 1081])
def test_scores_equal_the_restatement(beams):
    sc = R.scene(beams)
    assert (len(sc.points) % 64 != 0) or beams == 360
    want, gate = R.scene_scores(beams)
    g = make_grid(sc)
    reloc(g, sc, K=1)
    got = device_volume(g, R.NTHETA, R.NXY, R.NXY)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert not got[:, ~gate].any()
    # the table the host fills in for a NULL cos_sin is libm's: the same volume
    reloc(g, sc, K=1, cos_sin=None, theta0=sc.theta0, dtheta=R.DTHETA)
    assert np.array_equal(device_volume(g, R.NTHETA, R.NXY, R.NXY), want)


def _halo_points(sc):
    """sensor-frame points whose look-ups, from the lattice node next to the truth with the identity rotation, are anchored at
    local cell 31 in x, in y and in both"""
    cs = sc.gc.cell_size
    t = (sc.x0 + 11 * R.STEP, sc.y0 + 12 * R.STEP)
    m0, n0 = int(t[0] / cs) // 32, int(t[1] / cs) // 32
    pts = []
    for m in (m0 - 1, m0, m0 + 1):
        for j in range(0, 96, 5):
            pts.append(((32 * m + 31.5 + 0.37) * cs, (32 * (n0 - 1) + j + 0.5 + 0.21) * cs))       # lx == 31
            pts.append(((32 * (m0 - 1) + j + 0.5 + 0.63) * cs, (32 * (n0 + m - m0) + 31.5 + 0.4) * cs))   # ly == 31
        pts.append(((32 * m + 31.5 + 0.5) * cs, (32 * n0 + 31.5 + 0.25) * cs))                       # both
    w = np.array(pts)
    return w - np.array(t)[None, :], t


EDGE_CASES = ["nx1", "ntheta1", "P1", "P63", "border", "nan_cells", "halo", "share_rotations", "share_single_position"]


def edge_case(case):
    """(points, table, lattice, restated volume, restated gate) of one edge case, checked to be what its name says"""
    sc = R.scene(1081)
    pts, table = sc.points, sc.table
    lat = dict(x0=sc.x0 + 9 * R.STEP, y0=sc.y0 + 9 * R.STEP, step=R.STEP, nx=5, ny=5)
    if case == "nx1":
        lat.update(nx=1, ny=6); table = sc.table[8:15]
    elif case == "ntheta1":
        table = sc.table[12:13]
    elif case == "P1":
        pts = sc.points[500:501]
    elif case == "P63":
        pts = sc.points[:63]
    elif case == "border":
        # 30 x 30 nodes, 1 m apart, from 2 m outside the grid's corner to beyond its far border: positions outside the grid, in tiles no
        # scan ever initialised and in the map; the scan stretched so that end points leave the grid and reach empty tiles
        lat = dict(x0=-2.0, y0=-2.0, step=1.0, nx=30, ny=30); table = sc.table[::9]
        pts = np.concatenate([sc.points, 1.7 * sc.points])[:capi.MAX_ICP_POINTS]
    elif case == "nan_cells":
        table = sc.table[10:15]
    elif case == "halo":
        pts, t = _halo_points(sc)
        lat = dict(x0=t[0], y0=t[1], step=R.STEP, nx=2, ny=2); table = np.array([[1.0, 0.0], [0.0, 1.0]])
    elif case == "share_rotations":
        lat.update(nx=5, ny=3); table = sc.table[:7]           # 15 positions, 7 rotations: workgroups of 4 and of 3 rotations
    elif case == "share_single_position":
        lat.update(nx=1, ny=1, x0=sc.x0 + 11 * R.STEP, y0=sc.y0 + 12 * R.STEP); table = sc.table[:13]     # 13 rotations over 4 workgroups
    nt = len(table)
    want, gate = R.scores(sc.view, pts, lat["x0"], lat["y0"], lat["step"], lat["nx"], lat["ny"], table)
    # the case is what it says
    xs = lat["x0"] + np.arange(lat["nx"]) * lat["step"]; ys = lat["y0"] + np.arange(lat["ny"]) * lat["step"]
    seen = set()
    for iy, ix in zip(*np.nonzero(gate)):
        for c, s in table:
            wx = (c * pts[:, 0] - s * pts[:, 1]) + xs[ix]; wy = (s * pts[:, 0] + c * pts[:, 1]) + ys[iy]
            st, _ = sc.view.bilinear(wx, wy)
            seen |= set(st.tolist())
            if case == "halo" and (c, s) == (1.0, 0.0) and (ix, iy) == (0, 0):
                cs = sc.gc.cell_size
                lx = np.floor(wx / cs - 0.5).astype(int) & 31; ly = np.floor(wy / cs - 0.5).astype(int) & 31
                ok = st == R.SUCCESS
                assert (ok & (lx == 31) & (ly != 31)).any() and (ok & (ly == 31) & (lx != 31)).any() and (ok & (lx == 31) & (ly == 31)).any()
    assert gate.any() and want.max() > 0
    if case == "border":
        gst, _ = sc.view.bilinear(np.tile(xs, lat["ny"]), np.repeat(ys, lat["nx"]))
        assert {R.INVALIDINDEX, R.EMPTYPARTITION, R.SUCCESS} <= set(gst.tolist())
        assert {R.INVALIDINDEX, R.EMPTYPARTITION, R.SUCCESS} <= seen and not gate.all()
    if case == "nan_cells":
        assert R.ISNAN in seen
    return pts, table, lat, want, gate


@pytest.mark.parametrize("case", EDGE_CASES)
def test_edge_lattices_equal_the_restatement(case):
    sc = R.scene(1081)
    pts, table, lat, want, gate = edge_case(case)
    nt = len(table)
    g = make_grid(sc)
    reloc(g, sc, points=pts, x0=lat["x0"], y0=lat["y0"], step_xy=lat["step"], nx=lat["nx"], ny=lat["ny"], ntheta=nt, cos_sin=table,
          theta_wraps=False, K=4)
    got = device_volume(g, nt, lat["ny"], lat["nx"])
    assert np.array_equal(got, want)
    assert not got[:, ~gate].any()


@pytest.mark.parametrize("name", sorted(R.handmade_volumes()) + ["scene"])
def test_peaks_equal_the_restatement(name):
    if name == "scene":
        vol, wraps = R.scene_scores(1081)[0], True
    else:
        vol, wraps, _ = R.handmade_volumes()[name]
    g = capi.TsdGridDevice(5, 0.05, 0.15)
    all_idx, all_score = R.peaks(vol, vol.shape, wraps, 64)        # (the K best are the first K of the 64 best)
    for K in (1, 5, 64):
        idx, score = g.debug_reloc_peaks(vol, vol.shape, wraps, K)
        assert idx.tolist() == all_idx[:K].tolist() and score.tolist() == all_score[:K].tolist()


@pytest.mark.parametrize("beams", [360, 1081])
def test_relocalize_finds_the_pose(beams):
    sc = R.scene(beams)
    g = make_grid(sc)
    K = 16
    out = reloc(g, sc, K=K, min_pairs=beams // 4)
    vol, _ = R.scene_scores(beams)
    idx, score = R.peaks(vol, vol.shape, True, K)
    assert out["n_peaks"] == len(idx) == out["n_refined"]
    # the winner rule on the device's own registrations from every peak
    runs = []
    for i in idx:
        pose = R.candidate_pose(i, sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, sc.table)
        runs.append((pose, g.localize(pose, R.rays_world(pose, sc.rays_local, sc.gc.cell_size), sc.rays_local, sc.data, sc.mask,
                                      R.MIN_RANGE, R.MAX_RANGE, icp_params(g))))
    w = R.winner([r.pairs for _, r in runs])
    assert out["found"] and out["idx"] == int(idx[w]) and out["score"] == int(score[w])
    assert w == 0                                  # here the best peak is the one next to the truth (tests/test_cpu_reloc.py)
    pose, r = runs[w]
    assert out["icp"].pairs == r.pairs and np.array_equal(out["icp"].T, r.T)
    from oracle import pyoracle as O
    final = O.mat3_mul(pose, r.T)
    assert np.array_equal(out["pose"], final)      # bit for bit
    assert out["coarse"] == (pose[0, 2], pose[1, 2], pose[0, 0], pose[1, 0])
    d, a = R.pose_error(out["pose"], sc.truth)
    print(f"relocalised within {d:.4f} m, {math.degrees(a):.3f} deg; {r.pairs} pairs")
    assert d <= 0.5 * R.STEP and a <= 0.5 * R.DTHETA


def test_an_empty_room_is_not_found():
    sc = R.scene(360)
    from oracle import pyoracle as O
    room = synth.World("room", sc.gc)
    data, mask = O.ingest_f32(room.scan(*sc.truth, sc.geo), R.MAX_RANGE, sc.geo.angle_increment)
    sxy, ms, _ = O.scene_from_scan(sc.rays_local, data, mask)
    g = make_grid(sc)
    out = g.relocalize(sxy.reshape(-1, 2)[ms.astype(bool)], sc.rays_local, data, mask, R.MIN_RANGE, R.MAX_RANGE, icp_params(g),
                       sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, R.NTHETA, cos_sin=sc.table, theta_wraps=True, K=16, min_pairs=sc.geo.beams // 2)
    assert not out["found"] and np.isnan(out["pose"]).all()
    assert out["n_refined"] == out["n_peaks"] and out["icp"].pairs < sc.geo.beams // 2


def test_refused_calls_leave_the_grid_alone():
    sc = R.scene(360)
    g = make_grid(sc)
    d0 = g.digest()

    def refused(code, text, **kw):
        with pytest.raises(capi.TsdError):
            reloc(g, sc, **kw)
        assert g.last_rc == code
        assert g.lib.tsd_last_error(g.h).decode() == "tsd_relocalize: " + text, kw
        assert g.digest() == d0

    K_RANGE, SHAPE = "K outside 1 .. TSD_RELOC_MAX_PEAKS", "nx, ny, ntheta must be >= 1"
    REACH = "the lattice reaches further than TSD_RELOC_MAX_REACH grid widths from the grid"
    FAR_POINT = "a scan point is not finite or further than TSD_RELOC_MAX_REACH grid widths from the sensor"
    refused(E_ARG, "no scan point", points=np.zeros((0, 2)))
    refused(E_CAPACITY, "points > TSD_MAX_ICP_POINTS", points=np.zeros((capi.MAX_ICP_POINTS + 1, 2)))
    refused(E_ARG, K_RANGE, K=65)
    refused(E_ARG, K_RANGE, K=0)
    refused(E_ARG, "min_pairs < 0", min_pairs=-1)
    refused(E_CAPACITY, "nx * ny * ntheta > TSD_RELOC_MAX_CANDIDATES", nx=4096, ny=4096, ntheta=5, cos_sin=sc.table[:5])
    refused(E_ARG, "without a cos_sin table, theta0 and a non-zero dtheta are needed", cos_sin=None, theta0=0.3, dtheta=0.0)
    refused(E_ARG, SHAPE, nx=0)
    refused(E_ARG, "x0, y0 finite and step_xy > 0", step_xy=0.0)
    # a lattice, or a scan point, further from the grid than TSD_RELOC_MAX_REACH grid widths (its cell index would not fit an int);
    # a table entry that is not finite
    width = sc.gc.cells * sc.gc.cell_size
    refused(E_ARG, REACH, x0=1e300)
    refused(E_ARG, REACH, y0=-4.0 * width - 1.0)
    refused(E_ARG, REACH, x0=5.0 * width - (R.NXY - 1) * R.STEP + 1.0)
    far = sc.points.copy(); far[3, 1] = 4.0 * width + 1.0
    refused(E_ARG, FAR_POINT, points=far)
    bad = sc.table.copy(); bad[7, 0] = np.nan
    refused(E_ARG, "cos_sin is not finite", cos_sin=bad)
    # several bad arguments: the one that is checked first is named -- K, min_pairs, the lattice (shape, then x0 / y0 / step_xy), the
    # points, the table
    refused(E_ARG, K_RANGE, K=0, nx=0)
    refused(E_ARG, "min_pairs < 0", min_pairs=-1, nx=0)
    refused(E_ARG, SHAPE, nx=0, x0=float("nan"))
    refused(E_ARG, FAR_POINT, points=far, cos_sin=bad)
    # while a scan of the context is in flight
    s = capi.TsdSensorDevice(g, sc.geo.beams, sc.geo.angle_increment, sc.geo.angle_min, R.MAX_RANGE, R.MIN_RANGE, R.LOW_REFL)
    pose = synth.pose_matrix(*sc.poses[-1])
    s.set_pose(pose, R.rays_world(pose, sc.rays_local, sc.gc.cell_size), sc.rays_local)
    from oracle import pyoracle as O
    data, mask = O.ingest_f32(sc.world.scan(*sc.poses[-1], sc.geo), R.MAX_RANGE, sc.geo.angle_increment)
    gates = capi.GateParams(1.0, 0.5, 10.0, 10.0)      # (a push gate nothing passes: the scan leaves the grid as it is)
    prm = icp_params(g)
    import ctypes as C
    rg, mk = np.ascontiguousarray(data), np.ascontiguousarray(mask, dtype=np.uint8)
    g._check(g.lib.tsd_scan_submit(s.h, capi._d(rg), capi._u8(mk), None, C.byref(prm), C.byref(gates)), "tsd_scan_submit")
    with pytest.raises(capi.TsdError):
        reloc(g, sc)
    assert g.last_rc == E_ARG
    assert g.lib.tsd_last_error(g.h).decode() == "tsd_relocalize: a scan of this context is in flight (collect it first)"
    res = capi.ScanResult()
    g._check(g.lib.tsd_scan_collect(s.h, C.byref(res)), "tsd_scan_collect")
    assert not res.pushed and g.digest() == d0
    assert reloc(g, sc)["found"]                      # collected: accepted again
    s.close()


def test_relocalize_only_reads_the_grid():
    sc = R.scene(360)
    from oracle import pyoracle as O
    p = (sc.truth[0] - 0.3, sc.truth[1], 0.4)
    data, mask = O.ingest_f32(sc.world.scan(*p, sc.geo), R.MAX_RANGE, sc.geo.angle_increment)
    outs = []
    for with_reloc in (False, True):
        g = make_grid(sc)
        g.map_update(image=True)
        g.push(synth.pose_matrix(*p), data, mask, sc.geo.angle_increment, sc.geo.angle_min, R.MAX_RANGE, R.MIN_RANGE, R.LOW_REFL,
               want_stats=False)
        d_before = g.digest()
        if with_reloc:
            assert reloc(g, sc)["found"]
            assert g.digest() == d_before
        outs.append((g.digest(), g.map_update(image=True)))
        g.close()
    (d0, (w0, o0, r0, n0)), (d1, (w1, o1, r1, n1)) = outs
    assert d0 == d1 and w0 == w1 and w0[2] > 0 and n0 == n1
    assert np.array_equal(o0, o1) and np.array_equal(r0, r1)


def _node_in_stored_map(sc, tmp_path):
    path = tmp_path / "map.tsd"
    assert sc.grid.store_text(path)
    prm = facade.node_params(sc.gc, sc.geo, occ_grid_time_interval=0.0)
    node = facade.SlamNode(prm, synchronous=True)
    g = node.grid()
    g.load_text(path)
    return node, g, prm


def test_facade_starts_in_a_stored_map_without_overwriting_it(tmp_path):
    sc = R.scene(360)
    geo = sc.geo
    node, g, prm = _node_in_stored_map(sc, tmp_path)
    d0 = g.digest()
    scan0 = sc.world.scan(*sc.truth, geo)
    out = node.relocalize(scan0, geo.angle_min, geo.angle_increment, sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, R.NTHETA, cos_sin=sc.table,
                          theta_wraps=True, K=16, min_pairs=geo.beams // 4)
    assert out["found"]
    d, a = R.pose_error(out["pose"], sc.truth)
    assert d <= 0.5 * R.STEP and a <= 0.5 * R.DTHETA
    rep = node.report()
    assert rep["initialised"] and not rep["pushed"] and np.array_equal(rep["pose"], out["pose"])
    assert g.digest() == d0                            # started: the stored map is as it was
    node.laser(scan0, geo.angle_min, geo.angle_increment)      # the robot has not moved: registered, not pushed
    rep = node.report()
    assert not rep["reg_error"] and not rep["pushed"] and not rep["no_model"] and g.digest() == d0
    # it drives back towards the mapped trajectory: tracked, and pushed once the pose change passes the gate
    pushed = 0
    for k in range(1, 11):
        p = (sc.truth[0] - 0.06 * k, sc.truth[1], sc.truth[2] + 0.01 * k)
        node.laser(sc.world.scan(*p, geo), geo.angle_min, geo.angle_increment)
        rep = node.report()
        assert not rep["reg_error"] and not rep["no_model"], k
        dk, ak = R.pose_error(rep["pose"], p)
        assert dk <= 0.5 * R.STEP and ak <= 0.5 * R.DTHETA, (k, dk, ak)
        if rep["pushed"] and not pushed:
            assert g.digest() != d0
        pushed += rep["pushed"]
    assert pushed >= 1
    node.close()


def test_facade_ordinary_start_overwrites_the_stored_map(tmp_path):
    """what starting through relocalize avoids: the first scan of an ordinary start is pushed at the configured start pose"""
    sc = R.scene(360)
    node, g, _ = _node_in_stored_map(sc, tmp_path)
    d0 = g.digest()
    node.laser(sc.world.scan(*sc.truth, sc.geo), sc.geo.angle_min, sc.geo.angle_increment)
    assert node.report()["pushed"] and g.digest() != d0
    node.close()


def test_facade_reseats_a_running_localiser(tmp_path):
    sc = R.scene(360)
    geo = sc.geo
    node, g, prm = _node_in_stored_map(sc, tmp_path)
    scan0 = sc.world.scan(*sc.truth, geo)
    first = node.relocalize(scan0, geo.angle_min, geo.angle_increment, sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, R.NTHETA, cos_sin=sc.table,
                            theta_wraps=True, K=4)
    assert first["found"]
    lost = synth.pose_matrix(sc.truth[0] + 3.0, sc.truth[1] - 2.0, 0.0)
    node.start_at(lost, scan0, geo.angle_min, geo.angle_increment)         # a running localiser, re-seated somewhere wrong
    assert np.array_equal(node.report()["pose"], lost)
    d0 = g.digest()
    again = node.relocalize(scan0, geo.angle_min, geo.angle_increment, sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, R.NTHETA, cos_sin=sc.table,
                            theta_wraps=True, K=4)
    assert again["found"] and np.array_equal(again["pose"], first["pose"]) and g.digest() == d0
    node.laser(scan0, geo.angle_min, geo.angle_increment)
    rep = node.report()
    d, a = R.pose_error(rep["pose"], sc.truth)
    assert not rep["reg_error"] and d <= 0.5 * R.STEP and a <= 0.5 * R.DTHETA
    node.close()
