"""The merge group under rigid transforms on the GPU (tsd_group_create_rigid / k_group_merge_rigid, multigpu.LocalOccupancyGroup's
``transforms``, facade.SlamFleet.set_transforms): byte equality with the numpy restatement of tests/group_rigid_ref.py -- no tolerance,
no excluded cells --, with the translation group's kernel at whole-cell identity transforms, on two aligned oracle-built grids and
through the facade's fleet."""
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, multigpu, synth
from tests import align_ref as A
from tests import group_merge_ref as GR
from tests import group_rigid_ref as R

pytestmark = pytest.mark.gpu

CS = 0.05
DEG = math.pi / 180.0


def _transform(spec, cs, side):
    """("I",) | ("sh", ox, oy) whole cells | ("rot", angle, fx, fy) about the grid's centre, then a shift in cells | ("raw", angle, fx, fy)
    about the grid's corner | ("q", k, fx, fy) an exact quarter turn about the centre, then a shift in cells"""
    kind = spec[0]
    if kind == "I":
        return np.eye(3)
    if kind == "sh":
        return R.shift(spec[1], spec[2], cs)
    if kind == "rot":
        h = 0.5 * side * cs
        return R.about(spec[1], (h, h), (spec[2] * cs, spec[3] * cs))
    if kind == "raw":
        return R.rigid(spec[1], spec[2] * cs, spec[3] * cs)
    T = R.quarter_turn(spec[1], side * cs)
    T[0, 2] += spec[2] * cs
    T[1, 2] += spec[3] * cs
    return T


# (map_size_log2 per member, transform per member, explicit window or (0, 0), cell size)
CASES = {
    "n1_identity": ([9], [("I",)], (0, 0), CS),
    "n1_7deg": ([9], [("raw", 7.3 * DEG, 8.624, -5.436)], (0, 0), CS),
    "n1_quarter_turn_shifted": ([8], [("q", 1, 3.0, -2.0)], (0, 0), CS),
    "n1_45deg_window_not_16": ([8], [("rot", 45.0 * DEG, 0.0, 0.0)], (250, 203), CS),
    "n2_7deg": ([9, 9], [("I",), ("rot", 7.3 * DEG, 8.624, -5.436)], (0, 0), CS),
    "n2_quarter_and_half_cell": ([9, 9], [("I",), ("raw", 0.0, 17.25, -40.5)], (0, 0), CS),
    "n2_tiny_angle": ([9, 9], [("I",), ("raw", 1e-6, 0.5, 0.25)], (0, 0), CS),
    "n2_half_turn_mixed": ([9, 8], [("I",), ("q", 2, 10.5, 3.25)], (0, 0), CS),
    "n2_three_quarter_turn_far": ([8, 9], [("sh", -5, 0), ("q", 3, 300.0, 7.0)], (0, 0), CS),
    "n2_cell_size_0025": ([9, 9], [("I",), ("rot", -17.0 * DEG, 3.25, 11.5)], (0, 0), 0.025),
    "n3_mixed_sizes": ([8, 9, 8], [("I",), ("rot", 30.0 * DEG, 17.0, -40.0), ("rot", 123.4 * DEG, 32.3, 7.7)], (0, 0), CS),
    "n3_45deg": ([9, 9, 9], [("I",), ("rot", 45.0 * DEG, 0.0, 0.0), ("rot", -17.0 * DEG, 3.25, -0.5)], (0, 0), CS),
    "n3_whole_cells": ([9, 9, 9], [("sh", 1, 7), ("sh", -5, 0), ("sh", 16, -40)], (0, 0), CS),
    "n8": ([9] * 8, [("I",), ("q", 1, 0.0, 0.0), ("q", 2, 1.0, 7.0), ("q", 3, -5.0, 0.25), ("raw", 1e-6, 16.0, -40.0),
                     ("rot", 7.3 * DEG, 0.25, 0.5), ("rot", 30.0 * DEG, 31.7, 2.2), ("rot", 123.4 * DEG, -20.0, 9.0)], (0, 0), CS),
    "window_width_not_16": ([9, 9], [("sh", 1, 0), ("rot", 7.3 * DEG, 17.5, 7.25)], (500, 410), CS),
    "window_smaller_than_box": ([9, 9, 9], [("sh", -5, -40), ("rot", 30.0 * DEG, 16.0, 7.0), ("rot", 45.0 * DEG, 33.0, 0.0)], (400, 300), CS),
    "member_outside_the_window": ([9, 8], [("I",), ("rot", 45.0 * DEG, 2000.0, 2000.0)], (512, 512), CS),
    "member_half_outside": ([9, 9], [("I",), ("rot", -17.0 * DEG, 256.0, 0.0)], (512, 512), CS),
    "n2_2048": ([11, 11], [("I",), ("rot", 7.3 * DEG, 8.6, -5.4)], (0, 0), CS),
}


def _random_maps(grids, rng):
    maps = [rng.integers(-128, 128, size=(g.cells, g.cells), dtype=np.int16).astype(np.int8) for g in grids]
    for m in maps:                                   # enough cells at exactly 100 and at the extremes
        m[rng.integers(0, m.shape[0], 4000), rng.integers(0, m.shape[1], 4000)] = 100
        m[rng.integers(0, m.shape[0], 500), rng.integers(0, m.shape[1], 500)] = -128
    return maps


@pytest.mark.parametrize("case", list(CASES))
def test_random_int8_maps_equal_the_restatement(case):
    """any int8 value, not only -1 / 0 / 100: merged map and n_occupied byte for byte"""
    logs, specs, (W, Hh), cs = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    grids = [capi.TsdGridDevice(l, cs, 3 * cs) for l in logs]
    Ts = [_transform(s, cs, g.cells) for s, g in zip(specs, grids)]
    maps = _random_maps(grids, rng)
    grp = multigpu.LocalOccupancyGroup(grids, None, W, Hh, transforms=Ts)
    try:
        x0, y0, ww, wh = R.window([m.shape for m in maps], Ts, cs, W, Hh)
        assert (grp.width, grp.height) == (ww, wh) and grp.corner == (x0, y0)
        assert all(np.array_equal(a, b) for a, b in zip(grp.transforms, Ts))
        want = R.merge(maps, Ts, cs, W, Hh)
        grp.merge_maps_async(maps)
        got = grp.merged()
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} cells differ"
        assert grp.n_occupied == R.n_occupied(want) and grp.n_occupied > 0
        if case == "member_outside_the_window":
            assert np.array_equal(want, maps[0])
        if max(logs) > 9:
            return
        # again with other maps: the count starts from zero, the previous merge leaves nothing behind
        maps2 = [np.roll(m, 3, axis=1) for m in maps]
        grp.merge_maps_async(maps2)
        want2 = R.merge(maps2, Ts, cs, W, Hh)
        assert np.array_equal(grp.merged(), want2) and grp.n_occupied == R.n_occupied(want2)
    finally:
        grp.close()


@pytest.mark.parametrize("offs,window", [([(0, 0), (16, -40)], (0, 0)), ([(1, 7), (-5, 0), (17, -40)], (0, 0)), ([(1, 0), (17, 7)], (500, 410))])
def test_whole_cell_identity_transforms_equal_the_translation_kernel(offs, window):
    """k_group_merge_rigid against k_group_merge on the SAME device maps: bytes, count, corner, width, height"""
    rng = np.random.default_rng(len(offs) + window[0])
    grids = [capi.TsdGridDevice(9, CS, 3 * CS) for _ in offs]
    maps = _random_maps(grids, rng)
    old = multigpu.LocalOccupancyGroup(grids, offs, *window)
    new = multigpu.LocalOccupancyGroup(grids, None, *window, transforms=[R.shift(ox, oy, CS) for ox, oy in offs])
    try:
        old.merge_maps_async(maps)
        want = old.merged()
        assert np.array_equal(want, GR.merge(maps, offs, *window))
        new.merge_maps_async([old.lib.tsd_group_member_map_dev(old.h, i) for i in range(len(grids))])     # the caller's device maps
        got = new.merged()
        assert (new.width, new.height, new.corner) == (old.width, old.height, old.corner)
        assert np.array_equal(got, want), f"{int((got != want).sum())} cells differ"
        assert new.n_occupied == old.n_occupied > 0
        # a translation group answers with its shifts as transforms
        assert all(np.array_equal(a, b) for a, b in zip(old.transforms, new.transforms))
    finally:
        old.close()
        new.close()


def test_two_aligned_grids_merge_into_one_map():
    """scene "diff" (tests/align_ref.py): B and A uploaded from the oracle's dumps, T from tsd_map_align(B, A); the group [B: I, A: T]
    merges the grids' own extractions as the restatement merges their occupancy() maps, and A warped into B's frame agrees with B.
    Observed on an MI355X: 1353 / 1361 = 0.9941 (tests/test_cpu_group_rigid.py has 0.994 under the true transform, 0.144 under a wrong one)."""
    sc = A.scene("diff")
    gb, ga = (capi.TsdGridDevice(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc) for _ in range(2))
    gb.upload_tiles(*sc.dump_b)
    ga.upload_tiles(*sc.dump_a)
    out = gb.align_to(ga, **sc.lattice, K=A.K, iterations=A.ITERATIONS)
    assert out["found"] and out["cell_error"] > 0.5
    T = out["T"]
    digests = [gb.digest(), ga.digest()]
    Ts = [np.eye(3), T]
    grp = multigpu.LocalOccupancyGroup([gb, ga], transforms=Ts)
    warp = multigpu.LocalOccupancyGroup([ga], None, sc.cells, sc.cells, transforms=[T])
    try:
        grp.merge_async()
        merged = grp.merged()
        own = [g.occupancy(False, 2)[0] for g in (gb, ga)]
        want = R.merge(own, Ts, sc.cs)
        assert np.array_equal(merged, want), f"{int((merged != want).sum())} cells differ"
        assert grp.n_occupied == R.n_occupied(want) > (own[0] == 100).sum()
        warp.merge_async()
        warped = warp.merged()
        assert np.array_equal(warped, R.merge([own[1]], [T], sc.cs, sc.cells, sc.cells))
        share, hits, counted = R.agreement(own[0], warped)
        print(f"agreement of A warped by the aligned T with B: {hits} / {counted} = {share:.4f}")
        assert counted > 1000 and share >= 0.97
        # inflation reaches the members' extractions
        grp.merge_async(True, 3)
        assert np.array_equal(grp.merged(), R.merge([g.occupancy(True, 3)[0] for g in (gb, ga)], Ts, sc.cs))
        assert [gb.digest(), ga.digest()] == digests
    finally:
        grp.close()
        warp.close()


def test_refusals_and_a_good_call_follows(capfd):
    grids = [capi.TsdGridDevice(8, CS, 3 * CS) for _ in range(2)]
    good = R.rigid(0.3, 1.0, -2.0)

    def refused(T, **kw):
        with pytest.raises(capi.TsdError):
            multigpu.LocalOccupancyGroup(grids, transforms=[np.eye(3), T], **kw)

    scaled = good.copy(); scaled[:2, :2] *= 1.001
    shear = np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    mirror = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = good.copy(); nan[0, 2] = np.nan
    inf = good.copy(); inf[1, 1] = np.inf
    row = good.copy(); row[2, 0] = 1e-3
    row2 = good.copy(); row2[2, 2] = 2.0
    far = R.rigid(0.0, (2 ** 24 + 1) * CS, 0.0)
    wide = R.rigid(0.0, 65400 * CS, 0.0)                 # 65400 + 256 cells: a box over 65536
    for T in (scaled, shear, mirror, nan, inf, row, row2, far, wide):
        refused(T)
    assert "tsd_group_create_rigid" in capfd.readouterr().err
    refused(good, width=512, height=0)
    with pytest.raises(capi.TsdError, match="exclusive"):
        multigpu.LocalOccupancyGroup(grids, [(0, 0), (1, 1)], transforms=[np.eye(3), good])
    with pytest.raises(capi.TsdError):
        multigpu.LocalOccupancyGroup(grids, transforms=[good])                      # one transform for two grids
    with pytest.raises(capi.TsdError):
        multigpu.LocalOccupancyGroup([grids[0], grids[0]], transforms=[np.eye(3), good])
    # the good call on the same contexts; `wide` within the limit with an explicit window
    rng = np.random.default_rng(3)
    maps = _random_maps(grids, rng)
    for Ts, win in (([np.eye(3), good], (0, 0)), ([np.eye(3), wide], (300, 256))):
        grp = multigpu.LocalOccupancyGroup(grids, None, *win, transforms=Ts)
        try:
            grp.merge_maps_async(maps)
            assert np.array_equal(grp.merged(), R.merge(maps, Ts, CS, *win))
        finally:
            grp.close()


def test_slam_fleet_merges_maps_turned_against_each_other():
    """Two nodes map the same room; node 1's scans are taken from poses turned by 12 degrees about the start against node 0's, so its
    map is the room turned by -12 degrees in its grid.  Before set_transforms the fleet publishes the whole-cell merge; after
    align + set_transforms it publishes the rigid merge of the two nodes' own maps.  Observed on an MI355X: node 1's map warped by
    the aligned transform agrees with node 0's in 3453 / 3470 = 0.9951 of its occupied cells."""
    gc = synth.GridConfig(10, 0.025)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    poses = synth.trajectory(world, 6)
    yaw = 12.0 * DEG
    turn = R.about(yaw, (float(world.start[0]), float(world.start[1])))             # node 1's grid coordinates into node 0's
    turned = [(turn @ np.array([p[0], p[1], 1.0]))[:2].tolist() + [p[2] + yaw] for p in poses]
    scans = [synth.scans_for(world, geo, poses), synth.scans_for(world, geo, np.array(turned))]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=1000.0), synchronous=True, name=f"tsd_slam_{i}")
             for i in range(2)]
    fleet = facade.SlamFleet(nodes)
    try:
        for k in range(len(poses)):
            for n, s in zip(nodes, scans):
                n.laser(s[k], geo.angle_min, geo.angle_increment)
        cs, cells = gc.cell_size, gc.cells
        before = fleet.publish_merged_map()
        for n in nodes:
            n.publish_map()
        own = [n.map_msg() for n in nodes]
        assert (before["width"], before["height"]) == (cells, cells)
        assert np.array_equal(before["data"], GR.merge([o["data"] for o in own]))
        # the lattice of tests/test_gpu_align.py::test_slam_fleet_align (0.05 m, half a degree: a node must lie inside the cut)
        land = turn @ np.array([0.5 * gc.width, 0.5 * gc.width, 1.0])
        lat = dict(step_xy=0.05, nx=12, ny=12, ntheta=9, theta0=yaw - 4.3 * 0.5 * DEG, dtheta=0.5 * DEG, K=8, iterations=64)
        out = fleet.align(0, 1, x0=land[0] - 5.4 * 0.05, y0=land[1] - 5.7 * 0.05, **lat)
        T = out["T"]
        d, a = A.map_error(T, turn, gc.width)
        print(f"fleet: align found {out['found']}, {d:.3g} m and {a:.3g} rad from the turn, cell_error {out['cell_error']:.3g}")
        assert out["found"] and out["cell_error"] > 0.5
        Ts = [np.eye(3), T]
        with pytest.raises(capi.TsdError):
            fleet.set_transforms([np.eye(3)])
        with pytest.raises(capi.TsdError):
            fleet.set_transforms([T, np.eye(3)])
        with pytest.raises(capi.TsdError):
            fleet.set_transforms([np.eye(3), T * 1.01])
        assert np.array_equal(fleet.publish_merged_map()["data"], before["data"])      # a refused call leaves the group as it was
        fleet.set_transforms(Ts)
        m = fleet.publish_merged_map()
        x0, y0, W, H = R.window([(cells, cells)] * 2, Ts, cs)
        assert (m["width"], m["height"]) == (W, H) and W > cells and H > cells
        assert m["origin_position"][0] == own[0]["origin_position"][0] + float(x0) * cs
        assert m["origin_position"][1] == own[0]["origin_position"][1] + float(y0) * cs and m["origin_position"][2] == 0.0
        assert m["resolution"] == own[0]["resolution"] and m["frame_id"] == own[0]["frame_id"]
        want = R.merge([o["data"] for o in own], Ts, cs)
        assert np.array_equal(m["data"], want), f"{int((m['data'] != want).sum())} cells differ"
        share, hits, counted = R.agreement(own[0]["data"], R.merge([own[1]["data"]], [T], cs, cells, cells))
        print(f"fleet: node 1's map warped into node 0's agrees in {hits} / {counted} = {share:.4f}")
        assert counted > 200 and share >= 0.97
        g = fleet.get_merged_map()
        assert np.array_equal(g["data"], m["data"]) and (g["width"], g["height"]) == (W, H) and g["stamp_ns"] >= m["stamp_ns"]
        assert np.array_equal(g["origin_position"], m["origin_position"])
        assert m["origin_orientation_xyzw"].tolist() == [0.0, 0.0, 0.0, 1.0]
        with pytest.raises(capi.TsdError):
            fleet.fuse_tsd()
        # whole-cell shifts fuse as before
        fleet.set_transforms([np.eye(3), R.shift(3, -2, cs)])
        assert fleet.fuse_tsd().digest()["cells_valid"] > 0
    finally:
        fleet.close()
        for n in nodes:
            n.close()


OFFS = [(1, 7), (-5, 0), (17, -40)]


def _cell_offsets(n, **kw):
    """(cell_offsets(), corner) of a group of n 256^2 grids"""
    grids = [capi.TsdGridDevice(8, CS, 3 * CS) for _ in range(n)]
    grp = multigpu.LocalOccupancyGroup(grids, **kw)
    try:
        return grp.cell_offsets(), grp.corner
    finally:
        grp.close()


@pytest.mark.parametrize("how", ["offsets", "shifts"])
def test_cell_offsets_of_whole_cell_groups(how):
    """the group answers with the offsets it was given, in the offsets' frame (the bounding box's corner is not (0, 0)), whichever
    constructor made it"""
    kw = dict(cell_offsets=OFFS) if how == "offsets" else dict(transforms=[R.shift(ox, oy, CS) for ox, oy in OFFS])
    offs, corner = _cell_offsets(3, **kw)
    assert corner == (-5, -40)
    assert offs == OFFS


@pytest.mark.parametrize("T,want", [(R.shift(17 + 5e-7, -40, CS), [(0, 0), (17, -40)]),      # the 1e-6-cell rule, inside
                                    (R.shift(17 + 2e-6, -40, CS), None),                      # and outside
                                    (R.rigid(1e-6), None),
                                    (R.shift(17.25, -40.5, CS), None)],
                         ids=["5e-7_off", "2e-6_off", "turned_1e-6_rad", "quarter_and_half_cell"])
def test_cell_offsets_follow_the_groups_whole_cell_decision(T, want):
    offs, _ = _cell_offsets(2, transforms=[np.eye(3), T])
    assert offs == want


def test_slam_fleet_fuses_by_the_groups_placement():
    """Two nodes whose grids lie 12 cells apart (x_offset 0 and 0.6 m).  A fleet that places them by those offsets from the start and a
    fleet over the same nodes that is told the same placement by set_transforms fuse to the same grid, bit for bit; between the two
    a turn makes fuse_tsd raise, and the whole-cell shift after it fuses again: fuse() asks the group it has, not a copy."""
    gc = synth.GridConfig(8, CS)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, occ_grid_time_interval=1000.0), synchronous=True,
                             name=f"tsd_slam_{i}") for i, xo in enumerate((0.0, 0.6))]
    try:
        for k in range(len(scans)):
            for i, n in enumerate(nodes):
                n.laser(scans[(k + i) % len(scans)], geo.angle_min, geo.angle_increment)
        placed = facade.SlamFleet(nodes)
        try:
            want = placed.fuse_tsd().digest()
        finally:
            placed.close()
        assert want["cells_valid"] > 1000
        fleet = facade.SlamFleet(nodes)
        try:
            h = 0.5 * gc.cells * CS
            fleet.set_transforms([np.eye(3), R.about(7.3 * DEG, (h, h))])
            with pytest.raises(capi.TsdError):
                fleet.fuse_tsd()
            off = GR.cell_offset(GR.map_origin(gc.cells, CS, 0.6), GR.map_origin(gc.cells, CS, 0.0), CS)
            assert off == -12
            fleet.set_transforms([np.eye(3), R.shift(off, 0, CS)])
            assert fleet.fuse_tsd().digest() == want
        finally:
            fleet.close()
    finally:
        for n in nodes:
            n.close()
