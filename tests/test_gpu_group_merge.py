"""The same-device merge group on the GPU (tsd_group_*, multigpu.LocalOccupancyGroup, facade.SlamFleet): byte equality with the numpy
restatement of tests/group_merge_ref.py -- no tolerance anywhere -- and the common-frame property of tests/nranks_common.py."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, multigpu, synth
from tests import group_merge_ref as R
from tests import helpers as H
from tests import nranks_common as NC

pytestmark = pytest.mark.gpu

XS, YS = (0, 16, 32, 1, 17, -5), (0, 7, -40)


def _offsets(n, k0=0):
    return [(XS[(k0 + i) % len(XS)], YS[(k0 + i) % len(YS)]) for i in range(n)]


# (member map_size_log2 per member, offsets, explicit window or (0, 0))
CASES = {
    "n1": ([9], [(0, 0)], (0, 0)),
    "n1_shifted_window": ([9], [(17, 7)], (512, 512)),
    "n2_aligned": ([9, 9], [(0, 0), (16, -40)], (0, 0)),
    "n2_unaligned": ([9, 9], [(1, 7), (-5, 0)], (0, 0)),
    "n3": ([9, 9, 9], _offsets(3, 1), (0, 0)),
    "n3_zero": ([9, 9, 9], [(0, 0)] * 3, (0, 0)),
    "n8": ([9] * 8, _offsets(8), (0, 0)),
    "mixed_sizes": ([8, 9, 8], [(0, 0), (17, -40), (32, 7)], (0, 0)),
    "mixed_sizes_far": ([8, 9], [(-5, 0), (300, 7)], (0, 0)),
    "window_smaller_than_box": ([9, 9, 9], [(-5, -40), (16, 7), (33, 0)], (400, 300)),
    "window_width_not_16": ([9, 9], [(1, 0), (17, 7)], (500, 410)),
    "cfg2_n2": ([12, 12], [(0, 0), (17, -40)], (0, 0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_random_int8_maps_equal_the_restatement(case):
    """any int8 value, not only -1 / 0 / 100: merged map and n_occupied byte for byte"""
    logs, offs, (W, Hh) = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    grids = [capi.TsdGridDevice(l, 0.05, 0.15) for l in logs]
    maps = [rng.integers(-128, 128, size=(g.cells, g.cells), dtype=np.int16).astype(np.int8) for g in grids]
    for m in maps:                                   # enough cells at exactly 100 and at the extremes
        m[rng.integers(0, m.shape[0], 4000), rng.integers(0, m.shape[1], 4000)] = 100
        m[rng.integers(0, m.shape[0], 500), rng.integers(0, m.shape[1], 500)] = -128
    grp = multigpu.LocalOccupancyGroup(grids, offs, W, Hh)
    try:
        want = R.merge(maps, offs, W, Hh)
        assert (grp.height, grp.width) == want.shape
        assert grp.corner == R.window([m.shape for m in maps], offs, W, Hh)[:2]
        grp.merge_maps_async(maps)
        got = grp.merged()
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} cells differ"
        assert grp.n_occupied == R.n_occupied(want) and grp.n_occupied > 0
        # again with other maps: the count starts from zero, the previous merge leaves nothing behind
        maps2 = [np.roll(m, 3, axis=1) for m in maps]
        grp.merge_maps_async(maps2)
        want2 = R.merge(maps2, offs, W, Hh)
        assert np.array_equal(grp.merged(), want2) and grp.n_occupied == R.n_occupied(want2)
    finally:
        grp.close()


def _ingest(host, geo, ranges_f32):
    data = np.zeros(geo.beams); mask = np.zeros(geo.beams, dtype=np.uint8)
    r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
    host.tsd_host_sensor_ingest_f32(r.ctypes.data_as(C.POINTER(C.c_float)), geo.beams, geo.angle_increment, geo.angle_min, H.MAX_RANGE,
                                    data.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    return data, mask


def _push_scans(host, grid, world, geo, robot, k0, k1, shift_xy=(0.0, 0.0)):
    """scans k0 .. k1-1 of `robot` pushed at its ground-truth GRID pose; the scan is taken at the WORLD position = grid position + shift"""
    for k in range(k0, k1):
        pose, (x, y, yaw) = NC.robot_pose(world, robot, k)
        data, mask = _ingest(host, geo, world.scan(x + shift_xy[0], y + shift_xy[1], yaw, geo))
        grid.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL, want_stats=False)


def test_three_robots_three_grids_one_map():
    gc, geo, world = NC.setup()
    host = facade.load_library()
    grids = [capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc) for _ in range(3)]
    for r, g in enumerate(grids):
        _push_scans(host, g, world, geo, r, 0, 12)
    grp = multigpu.LocalOccupancyGroup(grids)
    try:
        grp.merge_async()
        merged = grp.merged()
        own = [g.occupancy(False, 2)[0] for g in grids]
        assert np.array_equal(merged, np.maximum.reduce(own)), f"{int((merged != np.maximum.reduce(own)).sum())} cells differ"
        assert grp.n_occupied == int((merged == 100).sum()) > 200
        assert any((own[0] != m).any() for m in own[1:]), "all robots hold the same map: the merge is not exercised"
        for a in range(3):
            for b in range(a + 1, 3):
                NC.assert_common_frame(own[a], own[b], gc, a, b)
        # inflation reaches the members' extractions
        grp.merge_async(True, 3)
        assert np.array_equal(grp.merged(), np.maximum.reduce([g.occupancy(True, 3)[0] for g in grids]))
    finally:
        grp.close()


def test_shifted_grids_meet_in_the_merged_frame():
    gc, geo, world = NC.setup()
    host = facade.load_library()
    shift = (24, -8)                               # grid 1's origin lies (+24, -8) cells from grid 0's
    offs = [(0, 0), shift]
    grids = [capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc) for _ in range(2)]
    _push_scans(host, grids[0], world, geo, 0, 0, 12)
    _push_scans(host, grids[1], world, geo, 1, 0, 12, (shift[0] * gc.cell_size, shift[1] * gc.cell_size))
    grp = multigpu.LocalOccupancyGroup(grids, offs)
    try:
        grp.merge_async()
        merged = grp.merged()
        own = [g.occupancy(False, 2)[0] for g in grids]
        assert np.array_equal(merged, R.merge(own, offs))
        assert (grp.width, grp.height) == (gc.cells + 24, gc.cells + 8) and grp.corner == (0, -8)
        # each member alone in the merged window; rows well inside the room hold only the two walls that run along y
        x0, y0 = grp.corner
        placed = [R.merge([m], [(ox - x0, oy - y0)], grp.width, grp.height) for m, (ox, oy) in zip(own, offs)]
        assert all((p == 100).sum() > 200 for p in placed)
        hy = min(6.0, 0.3 * gc.width)
        cy = gc.cells // 2 - y0                        # the room's centre row in the window
        r0, r1 = cy - int((hy - 0.5) / gc.cell_size), cy + int((hy - 0.5) / gc.cell_size)
        ab, ba = NC.wall_agreement(placed[0][r0:r1], placed[1][r0:r1]), NC.wall_agreement(placed[1][r0:r1], placed[0][r0:r1])
        assert ab >= 0.99 and ba >= 0.99, (ab, ba)
        # the members' raw maps, without the shift, do not agree: the check can fail
        c = gc.cells // 2
        q0, q1 = c - int((hy - 1.0) / gc.cell_size), c + int((hy - 1.0) / gc.cell_size)
        wrong = NC.wall_agreement(own[0][q0:q1], own[1][q0:q1])
        assert wrong < 0.2, wrong
    finally:
        grp.close()


def _slam_run(oracle, merge_at, n_scans, n_robots=3):
    from tests.slam_driver import HipSlamFused, slam_kwargs
    gc, geo, world = NC.setup()
    slams = [HipSlamFused(oracle, **slam_kwargs(gc, geo, local_offset_x=multigpu.robot_offset_x(r))) for r in range(n_robots)]
    grp = multigpu.LocalOccupancyGroup([s.grid for s in slams])
    out = {"poses": [[] for _ in slams]}
    try:
        def scans(k0, k1):
            for k in range(k0, k1):
                for r, s in enumerate(slams):
                    _, (x, y, yaw) = NC.robot_pose(world, r, k)
                    out["poses"][r].append(s.process_scan(world.scan(x, y, yaw, geo))["pose"])
        scans(0, merge_at)
        if n_scans["merge"]:
            grp.merge_async()                      # begun, not waited for: the scans below are enqueued behind the extractions
        else:
            out["maps_at_merge"] = [s.grid.occupancy(False, 2)[0] for s in slams]
        scans(merge_at, merge_at + n_scans["after"])
        if n_scans["merge"]:
            out["merged"] = grp.merged()
        out["digests"] = [s.grid.digest() for s in slams]
    finally:
        grp.close()
        for s in slams:
            s.grid.close()
    return out


def test_scans_overlap_a_merge_in_flight(oracle):
    """20 scans per member submitted between merge_async and wait: poses and grids are those of a run without a merge, and the
    merged map is the maximum of the maps as they were at the merge point"""
    a = _slam_run(oracle, 10, {"merge": True, "after": 20})
    b = _slam_run(oracle, 10, {"merge": False, "after": 20})
    for pa, pb in zip(a["poses"], b["poses"]):
        assert len(pa) == 30 and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert a["digests"] == b["digests"]
    assert len({d["hash"] for d in a["digests"]}) == 3
    want = np.maximum.reduce(b["maps_at_merge"])
    assert np.array_equal(a["merged"], want), f"{int((a['merged'] != want).sum())} cells differ"
    assert (want == 100).sum() > 200


def _fleet_nodes(x_offsets):
    gc = synth.GridConfig(10, 0.025)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 6))
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=float(xo), occ_grid_time_interval=1000.0), synchronous=True,
                             name=f"tsd_slam_{i}") for i, xo in enumerate(x_offsets)]
    return gc, geo, scans, nodes


def test_slam_fleet_publishes_the_merged_map():
    gc, geo, scans, nodes = _fleet_nodes([0.0, 0.6])
    fleet = facade.SlamFleet(nodes)
    try:
        for k, s in enumerate(scans):
            for i, n in enumerate(nodes):
                n.laser(s if i == 0 else scans[len(scans) - 1 - k], geo.angle_min, geo.angle_increment)
        assert fleet.merged_frames() == 0
        m = fleet.publish_merged_map()
        for n in nodes:
            n.publish_map()
        own = [n.map_msg() for n in nodes]
        assert (m["width"], m["height"]) == (1048, 1024)
        assert m["origin_position"][0] == min(o["origin_position"][0] for o in own) == own[1]["origin_position"][0]
        assert m["origin_position"][1] == own[0]["origin_position"][1] and m["origin_position"][2] == 0.0
        assert m["resolution"] == own[0]["resolution"] and m["frame_id"] == own[0]["frame_id"]
        offs = [(R.cell_offset(o["origin_position"][0], m["origin_position"][0], gc.cell_size),
                 R.cell_offset(o["origin_position"][1], m["origin_position"][1], gc.cell_size)) for o in own]
        assert offs == [(24, 0), (0, 0)]
        want = R.merge([o["data"] for o in own], offs)
        assert np.array_equal(m["data"], want), f"{int((m['data'] != want).sum())} cells differ"
        assert (want == 100).sum() > 0 and any((own[0]["data"] != own[1]["data"]).ravel())
        g = fleet.get_merged_map()
        assert np.array_equal(g["data"], m["data"]) and g["stamp_ns"] >= m["stamp_ns"] and (g["width"], g["height"]) == (1048, 1024)
        assert fleet.merged_frames() == 1 and m["count"] == 1
        fleet.publish_merged_map()
        assert fleet.merged_frames() == 2 and fleet.merged_map_msg()["count"] == 2
    finally:
        fleet.close()
        for n in nodes:
            n.close()


def test_slam_fleet_refuses_a_fraction_of_a_cell():
    gc, geo, scans, nodes = _fleet_nodes([0.0, 0.61])
    try:
        with pytest.raises(capi.TsdError, match="whole cells"):
            facade.SlamFleet(nodes)
    finally:
        for n in nodes:
            n.close()
