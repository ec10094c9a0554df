"""TSD-level fusion on the GPU (tsd_fuse_*, capi.TsdGridDevice.fuse_from, facade.SlamFleet.fuse_tsd): byte equality with the numpy
restatement of tests/tsd_fuse_ref.py -- flags, _initWeight, tsd and weight, interiors and halos, fp64 storage -- and the fused grid
used as a grid: ray cast and push against the oracle on the same cells, store / load, ordering against scans in flight."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import group_merge_ref as GR
from tests import helpers as H
from tests import nranks_common as NC
from tests import tsd_fuse_ref as F

pytestmark = pytest.mark.gpu

TOL_CELL = 1e-5      # the push's cell-for-cell bar (tests/test_gpu_parity.py)


def _ingest(host, geo, ranges_f32):
    data = np.zeros(geo.beams); mask = np.zeros(geo.beams, dtype=np.uint8)
    r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
    host.tsd_host_sensor_ingest_f32(r.ctypes.data_as(C.POINTER(C.c_float)), geo.beams, geo.angle_increment, geo.angle_min, H.MAX_RANGE,
                                    data.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    return data, mask


def _push_scans(host, grid, world, geo, robot, ks, shift_cells=(0, 0), beams_off=None):
    """scans `ks` of `robot`: taken at its world pose, pushed at the pose in the grid's own frame (the world's shifted by -shift cells)"""
    cs = grid.cell_size
    for k in ks:
        _, (x, y, yaw) = NC.robot_pose(world, robot, k)
        data, mask = _ingest(host, geo, world.scan(x, y, yaw, geo))
        if beams_off is not None:
            mask[beams_off] = 0
        pose = synth.pose_matrix(x - shift_cells[0] * cs, y - shift_cells[1] * cs, yaw)
        grid.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL, want_stats=False)


def _setup(log2=9, cs=0.05):
    gc = synth.GridConfig(log2, cs)
    return gc, synth.ScanGeometry.full_circle_360(), synth.World("room", gc)


# name -> (grid log2 / cell size of the room, destination log2, [(member log2, offset, scans or None, freed)])
CASES = {
    "two_512_offset_0": (9, 0.05, 9, [(9, (0, 0), range(0, 6), False), (9, (0, 0), range(6, 12), False)]),
    "three_512_offsets": (9, 0.05, 9, [(9, (0, 0), range(0, 5), False), (9, (32, 64), range(5, 9), False), (9, (17, -5), range(9, 14), False)]),
    "two_512_misaligned": (9, 0.05, 9, [(9, (1, 0), range(0, 6), False), (9, (17, -5), range(6, 12), False)]),
    "sizes_differ": (9, 0.05, 9, [(8, (130, 121), range(0, 5), False), (9, (0, 0), range(5, 9), False), (10, (-250, -260), range(9, 12), False)]),
    "partly_outside": (9, 0.05, 9, [(9, (0, 0), range(0, 4), False), (9, (-203, 300), range(4, 9), False)]),
    "an_empty_member": (9, 0.05, 9, [(9, (0, 0), None, False), (9, (3, 3), range(0, 6), False), (9, (-40, 9), None, False)]),
    "freed_footprints": (9, 0.05, 9, [(9, (0, 0), range(0, 3), True), (9, (17, -5), None, True), (9, (17, -5), range(3, 4), True)]),
    "two_4096": (12, 0.025, 12, [(12, (0, 0), range(0, 6), False), (12, (17, -5), range(6, 12), False)]),
    "three_4096": (12, 0.025, 12, [(12, (0, 0), range(0, 4), False), (12, (32, 64), range(4, 8), False), (12, (1, 0), range(8, 12), False)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fusion_equals_the_restatement_byte_for_byte(case):
    log2, cs, dst_log2, members = CASES[case]
    gc, geo, world = _setup(log2, cs)
    host = facade.load_library()
    grids, offs = [], []
    for r, (ml, off, ks, freed) in enumerate(members):
        g = capi.TsdGridDevice(ml, cs, gc.max_trunc)
        # a member of another size holds the same world: its frame is the room's shifted by its offset
        if freed:
            assert g.free_footprint([world.cx - off[0] * cs + 0.3 * r, world.cy - off[1] * cs], 1.0, 1.0)
        if ks is not None:
            _push_scans(host, g, world, geo, r, ks, off)
        grids.append(g); offs.append(off)
    dst = capi.TsdGridDevice(dst_log2, cs, gc.max_trunc)
    _push_scans(host, dst, world, geo, 0, range(2))               # previous content: discarded
    stats = dst.fuse_from(grids, offs)
    want, want_stats = F.fuse_ref([g.download_tiles() for g in grids], offs, dst.cells)
    print(case, stats)
    F.assert_dumps_identical(dst.download_tiles(), want, case)
    assert stats == want_stats
    assert stats["tiles_materialised"] > 0 and stats["cells_valid"] > 1000
    if sum(ks is not None or fr for _, _, ks, fr in members) > 1:
        assert stats["cells_many_sources"] > 0
    # the push bookkeeping is as after a reset
    assert dst.push_stats_total()[1] == 0


def test_one_grid_fuses_to_itself_and_offsets_default_to_zero():
    gc, geo, world = _setup()
    host = facade.load_library()
    a, dst = capi.TsdGridDevice(9, 0.05, gc.max_trunc), capi.TsdGridDevice(9, 0.05, gc.max_trunc)
    _push_scans(host, a, world, geo, 0, range(8))
    dst.fuse_from([a])
    got, src = dst.download_tiles(), a.download_tiles()
    assert np.array_equal(got[0], src[0]) and got[1].tobytes() == src[1].tobytes()
    sel = src[0].astype(bool)
    for g, s in ((got[2], src[2]), (got[3], src[3])):
        gi, si = g.reshape(-1, 33, 33)[sel][:, :32, :32], s.reshape(-1, 33, 33)[sel][:, :32, :32]
        assert np.array_equal(np.isnan(gi), np.isnan(si)) and np.array_equal(gi[~np.isnan(si)], si[~np.isnan(si)])
    # (not the digest: it covers the halos, which the fusion fills where the push's incremental propagateBorders leaves stale ones)
    assert a.digest()["tiles_initialized"] == dst.digest()["tiles_initialized"] > 0


def test_the_fused_grid_is_a_grid(oracle):
    """robot A never saw what lies behind it (half its beams masked), robot B saw the whole room: a ray cast in the fused grid from
    B's pose gives the oracle's hits on the restated cells (mask exactly, coordinates within 1e-9: the ray cast's bar), and a push
    into the fused grid leaves the cells of the oracle's push into the same cells (the push's bar) -- sign masks, halos, tile state"""
    gc, geo, world = _setup()
    host = facade.load_library()
    a, b, dst = (capi.TsdGridDevice(9, 0.05, gc.max_trunc) for _ in range(3))
    offs = [(0, 0), (17, -5)]
    _push_scans(host, a, world, geo, 0, range(0, 6), offs[0], beams_off=slice(0, 180))
    _push_scans(host, b, world, geo, 2, range(0, 6), offs[1])
    dst.fuse_from([a, b], offs)
    want, _ = F.fuse_ref([a.download_tiles(), b.download_tiles()], offs, dst.cells)
    og = oracle.Grid(9, 0.05, gc.max_trunc)
    og.load(*want)
    alone = oracle.Grid(9, 0.05, gc.max_trunc)
    alone.load(*a.download_tiles())
    seen_only_by_b = 0
    for k in (1, 4):
        pose, _ = NC.robot_pose(world, 2, k)
        rl, rw = H.world_rays(oracle, geo, pose, gc.cell_size)
        co, no, mo, cnt_o = og.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)
        cd, nd, md, cnt_d = dst.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)
        assert np.array_equal(mo, md), f"hit masks differ at beams {np.nonzero(mo != md)[0][:10]}"
        assert cnt_o == cnt_d and cnt_o > 0.5 * geo.beams
        sel = np.repeat(mo.astype(bool), 2)
        assert np.max(np.abs(co[sel] - cd[sel])) <= 1e-9 and np.max(np.abs(no[sel] - nd[sel])) <= 1e-9
        seen_only_by_b += int((mo.astype(bool) & ~alone.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)[2].astype(bool)).sum())
    assert seen_only_by_b > 50, "robot A's own grid shows the same hits: the fused map adds nothing here"
    for k in (7, 9):
        pose, (x, y, yaw) = NC.robot_pose(world, 1, k)
        data, mask = _ingest(host, geo, world.scan(x, y, yaw, geo))
        so = og.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
        sd = dst.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
        assert so == sd, f"push {k}: stats differ\n oracle {so}\n hip    {sd}"
        H.assert_grids_equal(og.dump(), dst.download_tiles(), TOL_CELL)
    pose, _ = NC.robot_pose(world, 1, 9)
    rl, rw = H.world_rays(oracle, geo, pose, gc.cell_size)
    mo, md = og.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)[2], dst.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)[2]
    assert np.array_equal(mo, md) and mo.sum() > 0.5 * geo.beams


def _ordering_run(sync_before_fusion, fuse=True):
    gc, geo, world = _setup()
    host = facade.load_library()
    grids = [capi.TsdGridDevice(9, 0.05, gc.max_trunc) for _ in range(3)]
    dst = capi.TsdGridDevice(9, 0.05, gc.max_trunc)
    offs = [(0, 0), (17, -5), (32, 64)]
    for k in range(20):                                  # enqueued, never waited for (want_stats=False: no host sync)
        for r, g in enumerate(grids):
            _push_scans(host, g, world, geo, r, [k], offs[r])
    if sync_before_fusion:
        for g in grids:
            g.sync()
    if fuse:
        dst.fuse_begin(grids, offs)
    for r, g in enumerate(grids):                        # the members' next writes: behind the fusion's reads
        _push_scans(host, g, world, geo, r, [20, 21], offs[r])
    stats = dst.fuse_wait() if fuse else None
    return (dst.download_tiles() if fuse else None), stats, [g.download_tiles() for g in grids], [g.digest() for g in grids]


def test_fusion_is_ordered_against_scans_in_flight():
    fused_a, stats_a, members_a, dig_a = _ordering_run(False)
    fused_b, stats_b, members_b, dig_b = _ordering_run(True)
    _, _, members_c, dig_c = _ordering_run(True, fuse=False)
    F.assert_dumps_identical(fused_a, fused_b, "fusion without a host sync vs after tsd_sync of every member")
    assert stats_a == stats_b and stats_a["cells_many_sources"] > 10000
    assert dig_a == dig_b == dig_c
    for ma, mc in zip(members_a, members_c):
        F.assert_dumps_identical(ma, mc, "a member after the fusion vs without a fusion")


def test_stored_fused_grid_loads_with_an_equal_digest(oracle, tmp_path):
    """tsd_store_grid_text of the fused grid, loaded into a fresh context, has the digest -- the hash over every cell's bits, the
    counts; the two sums to the 1e-9 that their different summation orders leave -- of the oracle's grid that took the same route
    from the restated cells (loaded, stored as text, loaded from the text), and the two files are equal byte for byte.  (The text format prints every value with "%g" and stores no halos, so no grid equals its own stored copy bit for
    bit; against the fused grid itself the counts are equal and the sums agree to the format's six digits.)"""
    gc, geo, world = _setup()
    host = facade.load_library()
    a, b, dst, back = (capi.TsdGridDevice(9, 0.05, gc.max_trunc) for _ in range(4))
    _push_scans(host, a, world, geo, 0, range(5))
    _push_scans(host, b, world, geo, 1, range(5, 10), (17, -5))
    dst.fuse_from([a, b], [(0, 0), (17, -5)])
    path, path_o = tmp_path / "fused.grid", tmp_path / "restated.grid"
    dst.store_text(path)
    back.load_text(path)
    want, _ = F.fuse_ref([a.download_tiles(), b.download_tiles()], [(0, 0), (17, -5)], dst.cells)
    og = oracle.Grid(9, 0.05, gc.max_trunc)
    og.load(*want)
    assert og.store_text(path_o)
    assert path.read_bytes() == path_o.read_bytes() and len(path.read_bytes()) > 100000
    og2 = oracle.Grid.load_text(path_o, gc.cell_size)
    da, db = dst.digest(), back.digest()
    print(da, db, og2.digest())
    do = og2.digest()
    # (the bar of test_grid_digest_matches_oracle between a device digest and the oracle's: the two sum in different orders)
    assert db["hash"] == do["hash"] and db["cells_valid"] == do["cells_valid"] > 1000 and db["tiles_initialized"] == do["tiles_initialized"]
    assert abs(db["sum_tsd"] - do["sum_tsd"]) <= 1e-9 * max(1.0, abs(do["sum_tsd"]))
    assert abs(db["sum_weight"] - do["sum_weight"]) <= 1e-9 * max(1.0, abs(do["sum_weight"]))
    assert da["tiles_initialized"] == db["tiles_initialized"] > 0
    assert np.array_equal(dst.download_tile_state()[0], back.download_tile_state()[0])
    t0, t1 = dst.download_tiles(), back.download_tiles()
    sel = t0[0].astype(bool)
    i0, i1 = t0[2].reshape(-1, 33, 33)[sel][:, :32, :32], t1[2].reshape(-1, 33, 33)[sel][:, :32, :32]
    assert np.array_equal(np.isnan(i0), np.isnan(i1)) and np.nanmax(np.abs(i0 - i1)) <= 1e-5


def test_refused_arguments_name_their_reason_and_touch_nothing():
    gc, geo, world = _setup()
    host = facade.load_library()
    lib = capi.load_library()
    a, b, dst = (capi.TsdGridDevice(9, 0.05, gc.max_trunc) for _ in range(3))
    other_cs = capi.TsdGridDevice(9, 0.025, gc.max_trunc)
    other_trunc = capi.TsdGridDevice(9, 0.05, 2 * gc.max_trunc)
    for g in (a, dst):
        _push_scans(host, g, world, geo, 0, range(2))
    before = [g.digest() for g in (a, b, dst)]

    def refused(n, handles, offsets, text):
        hs = (C.c_void_p * max(len(handles), 1))(*handles)
        off = None if offsets is None else (C.c_int32 * len(offsets))(*offsets)
        for call in (lambda: lib.tsd_fuse_begin(dst.h, n, hs, off), lambda: lib.tsd_fuse(dst.h, n, hs, off, None)):
            assert call() == -1
            assert text in lib.tsd_last_error(dst.h).decode(), lib.tsd_last_error(dst.h).decode()

    refused(0, [a.h], None, "1 .. 64")
    refused(65, [a.h] * 65, None, "1 .. 64")
    refused(2, [a.h, None], None, "NULL")
    refused(2, [a.h, dst.h], None, "destination is among the members")
    refused(2, [a.h, a.h], None, "listed twice")
    refused(2, [a.h, other_cs.h], None, "cell size")
    refused(2, [a.h, other_trunc.h], None, "max_truncation")
    refused(2, [a.h, b.h], [0, 0, (1 << 24) + 1, 0], "offset")
    if lib.tsd_device_count() > 1:
        far = capi.TsdGridDevice(9, 0.05, gc.max_trunc, device=1)
        refused(2, [a.h, far.h], None, "one device")
    assert lib.tsd_fuse_wait(dst.h, None) == -1 and "without tsd_fuse_begin" in lib.tsd_last_error(dst.h).decode()
    assert [g.digest() for g in (a, b, dst)] == before


def test_destroying_a_member_or_the_destination_with_a_fusion_in_flight():
    gc, geo, world = _setup()
    host = facade.load_library()
    a, b, dst = (capi.TsdGridDevice(9, 0.05, gc.max_trunc) for _ in range(3))
    _push_scans(host, a, world, geo, 0, range(4))
    _push_scans(host, b, world, geo, 1, range(4))
    want, _ = F.fuse_ref([a.download_tiles(), b.download_tiles()], None, dst.cells)
    dst.fuse_begin([a, b])
    a.close()                                             # a member goes while the fusion may still read it
    dst.fuse_wait()
    F.assert_dumps_identical(dst.download_tiles(), want, "fusion whose member was destroyed in flight")
    dst.fuse_begin([b])
    dst.close()                                           # the destination goes with its fusion enqueued
    _push_scans(host, b, world, geo, 1, range(4, 6))      # the surviving member works on
    assert b.digest()["cells_valid"] > 1000


def test_slam_fleet_fuses_its_nodes_grids():
    gc = synth.GridConfig(10, 0.025)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 6))
    x_offsets = [0.0, 0.6, -0.425]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=float(xo), occ_grid_time_interval=1000.0), synchronous=True,
                             name=f"tsd_slam_{i}") for i, xo in enumerate(x_offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        for k in range(len(scans)):
            for i, n in enumerate(nodes):
                n.laser(scans[(k + 2 * i) % len(scans)], geo.angle_min, geo.angle_increment)
        fused = fleet.fuse_tsd()
        o0 = GR.map_origin(gc.cells, gc.cell_size, x_offsets[0])
        offs = [(GR.cell_offset(GR.map_origin(gc.cells, gc.cell_size, xo), o0, gc.cell_size), 0) for xo in x_offsets]
        assert offs == [(0, 0), (-24, 0), (17, 0)]
        views = [n.grid() for n in nodes]
        own = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, views[0].max_trunc)
        own.fuse_from(views, offs)
        F.assert_dumps_identical(fused.download_tiles(), own.download_tiles(), "SlamFleet.fuse_tsd vs fuse_from")
        assert fused.digest() == own.digest() and fused.digest()["cells_valid"] > 10000
        msg = fleet.fused_image_msg()
        assert (msg["height"], msg["width"], msg["step"], msg["encoding"]) == (gc.cells, gc.cells, 3 * gc.cells, "rgb8")
        assert np.array_equal(msg["data"], own.color_image()) and len(np.unique(msg["data"].reshape(-1, 3), axis=0)) > 2
        # every call fuses anew, into the same grid
        nodes[0].laser(scans[0], geo.angle_min, geo.angle_increment)
        again = fleet.fuse_tsd()
        assert again.h == fused.h
        own.fuse_from(views, offs)
        assert again.digest() == own.digest()
    finally:
        fleet.close()
        for n in nodes:
            n.close()
