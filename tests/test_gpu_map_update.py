"""The windowed map update (tsd_map_update_begin / tsd_map_update_wait, csrc/map_publish.hip).

An update recomputes and copies only the rectangle around the tiles that were pushed or freed since the context's previous frame; the
caller's full buffers, patched by every update, must always equal a full extraction.  The yardstick is tsd_occupancy /
tsd_color_image on the SAME context: an independent path that does not touch the frame staging.  Every comparison is exact.
A 1024^2 grid and a sensor that sees 2 m: a push's launch window is a few tiles, the map is 32 x 32 of them.
"""
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, multigpu, synth
from tests import helpers as H
from tests.slam_driver import HipSlamFused, slam_kwargs

pytestmark = pytest.mark.gpu

GC = synth.GridConfig(10, 0.05)
GEO = synth.ScanGeometry.full_circle_360()
N = GC.cells
SHORT_RANGE = 2.0                  # the room's walls are 16 m and 12 m long
FULL = (0, 0, N, N)


def _loop_poses(world, n):
    """once around the room, 1 m inside its walls: every step crosses into the next tile or so, the last pose is the first again"""
    ax, ay = world.hx - 1.0, world.hy - 1.0
    per = 4 * (ax + ay)
    out = []
    for k in range(n):
        s = per * k / (n - 1) % per
        if s < 2 * ax: x, y, yaw = -ax + s, -ay, 0.0
        elif s < 2 * ax + 2 * ay: x, y, yaw = ax, -ay + (s - 2 * ax), 0.5 * math.pi
        elif s < 4 * ax + 2 * ay: x, y, yaw = ax - (s - 2 * ax - 2 * ay), ay, math.pi
        else: x, y, yaw = -ax, ay - (s - 4 * ax - 2 * ay), 1.5 * math.pi
        out.append((world.cx + x + 0.013 * k, world.cy + y - 0.007 * k, yaw + 0.05))
    return out


def _push(oracle, dg, world, pose3):
    x, y, yaw = pose3
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, GEO), SHORT_RANGE, GEO.angle_increment)
    dg.push(synth.pose_matrix(x, y, yaw), data, mask, GEO.angle_increment, GEO.angle_min, SHORT_RANGE, H.MIN_RANGE, H.LOW_REFL,
            want_stats=False)


def _grid():
    return capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)


def _assert_current(dg, occ, rgb, inflate, factor, what):
    want, _ = dg.occupancy(inflate, factor)
    assert np.array_equal(occ, want), f"{what}: {np.count_nonzero(occ != want)} cells differ from tsd_occupancy at {np.argwhere(occ != want)[:4]}"
    if rgb is not None:
        img = dg.color_image(N, N)
        assert np.array_equal(rgb, img), f"{what}: image differs from tsd_color_image at {np.argwhere(rgb != img)[:4]}"
    return want


@pytest.mark.parametrize("inflate,factor", [(False, 2), (True, 2), (True, 31)])
def test_closed_loop_updates_keep_the_host_map_current(oracle, inflate, factor):
    world = synth.World("room", GC)
    dg = _grid()
    poses = _loop_poses(world, 30)
    windows, n_total = [], 0
    for k, pose in enumerate(poses):
        _push(oracle, dg, world, pose)
        if k == 17:
            # a buffer of the caller's own for one update: written inside the window only
            mine, mine_rgb = np.full((N, N), 55, dtype=np.int8), np.full((N, N, 3), 55, dtype=np.uint8)
            win, occ1, rgb1, ns = dg.map_update(inflate, factor, occ=mine, rgb=mine_rgb)
            x, y, w, h = win
            want = dg.occupancy(inflate, factor)[0]
            img = dg.color_image(N, N)
            inside = np.zeros((N, N), bool)
            inside[y:y + h, x:x + w] = True
            assert 0 < w <= N // 2 and 0 < h <= N // 2
            assert (occ1[~inside] == 55).all() and (rgb1[~inside] == 55).all(), "written outside the window"
            assert np.array_equal(occ1[inside], want[inside]) and np.array_equal(rgb1[inside], img[inside])
            # (the update is spent: the wrapper's own buffers get this window from a full frame)
            occ, rgb, _ = dg.map_frame(inflate, factor)
        else:
            win, occ, rgb, ns = dg.map_update(inflate, factor)
            windows.append(win)
        n_total += ns
        print(f"scan {k}: window {win}, marks {ns}")
        _assert_current(dg, occ, rgb, inflate, factor, f"scan {k} window {win}")
    assert windows[0] == FULL, "the first update is the whole map"
    for k, (x, y, w, h) in enumerate(windows[1:], 1):
        assert 0 < w <= N // 2 and 0 < h <= N // 2, f"update {k}: window {w} x {h}"
        assert x % 32 == 0 and y % 32 == 0 and x + w <= N and y + h <= N
    assert len({(x, y) for x, y, _, _ in windows}) > 8, "the window did not move"
    assert n_total > 0 and (occ == 100).sum() > 200 and (occ == 0).sum() > 10000


def test_free_footprint_removes_the_marks(oracle):
    world = synth.World("room", GC)
    dg = _grid()
    x0, y0 = world.cx - world.hx + 1.0, world.cy - world.hy + 1.0
    _push(oracle, dg, world, (x0, y0, 0.3))
    _, occ0, _, _ = dg.map_update(True, 5)
    wall = (slice(int((y0 - 1.5) / GC.cell_size), int((y0 + 1.5) / GC.cell_size)), slice(int((x0 - 1.4) / GC.cell_size), int((x0 - 0.6) / GC.cell_size)))
    assert (occ0[wall] == 100).sum() > 50
    assert dg.free_footprint([x0 - 1.0, y0], 1.0, 2.0)                          # over the left wall
    win, occ, rgb, _ = dg.map_update(True, 5)
    assert 0 < win[2] <= N // 2 and 0 < win[3] <= N // 2
    _assert_current(dg, occ, rgb, True, 5, "after freeFootprint")
    assert (occ[wall] == 100).sum() < (occ0[wall] == 100).sum(), "the freed wall's marks are still there"


def test_no_change_gives_an_empty_window(oracle):
    world = synth.World("room", GC)
    dg = _grid()
    _push(oracle, dg, world, (world.cx, world.cy - world.hy + 1.0, 0.0))
    _, occ, rgb, _ = dg.map_update(True, 2)
    mine, mine_rgb = np.full((N, N), 55, dtype=np.int8), np.full((N, N, 3), 55, dtype=np.uint8)
    win = dg.map_update_begin(True, 2, occ=mine, rgb=mine_rgb)
    assert win == (0, 0, 0, 0)
    o, r, ns = dg.map_update_wait()
    assert ns == 0 and (o == 55).all() and (r == 55).all()
    win, occ2, rgb2, _ = dg.map_update(True, 2)                                 # ... and on the wrapper's own buffers
    assert win[2] == 0 and np.array_equal(occ2, occ) and np.array_equal(rgb2, rgb)
    with pytest.raises(capi.TsdError, match="no frame in flight"):
        dg.map_update_wait()


def test_fallbacks_return_the_whole_map(oracle):
    world = synth.World("room", GC)
    dg, other = _grid(), _grid()
    p0 = (world.cx - 3.0, world.cy - world.hy + 1.0, 0.2)
    _push(oracle, dg, world, p0)
    _push(oracle, other, world, (world.cx + 4.0, world.cy - world.hy + 1.2, 0.1))

    def full(what, inflate, factor, image=True):
        win, occ, rgb, _ = dg.map_update(inflate, factor, image=image)
        assert win == FULL, f"{what}: window {win}"
        _assert_current(dg, occ, rgb, inflate, factor, what)

    def windowed(what, inflate, factor, image=True):
        _push(oracle, dg, world, (p0[0] + 0.3, p0[1], p0[2]))
        win, occ, rgb, _ = dg.map_update(inflate, factor, image=image)
        assert 0 < win[2] <= N // 2, f"{what}: window {win}"
        _assert_current(dg, occ, rgb, inflate, factor, what)

    full("first call", True, 2)
    windowed("second call", True, 2)
    full("changed factor", True, 3)
    windowed("same factor again", True, 3)
    full("inflation off", False, 3)
    full("factor 32", True, 32)
    _push(oracle, dg, world, p0)
    full("factor 32 again", True, 32)
    full("back to factor 3", True, 3)
    dg.reset()
    full("after tsd_reset", True, 3)
    _push(oracle, dg, world, p0)
    windowed("after the reset's frame", True, 3)
    dg.upload_tiles(*other.download_tiles())
    full("after tsd_upload_tiles", True, 3)          # (the box was empty: it is the upload that asks for the whole map)
    dg.fuse_from([other])
    full("after fuse_from", True, 3)
    # image switched on after map-only frames (a context whose staging never held an image)
    d2 = _grid()
    _push(oracle, d2, world, p0)
    win, occ, rgb, _ = d2.map_update(True, 2, image=False)
    assert win == FULL and rgb is None
    _push(oracle, d2, world, (p0[0] + 0.3, p0[1], p0[2]))
    win, occ, rgb, _ = d2.map_update(True, 2, image=False)
    assert 0 < win[2] <= N // 2 and rgb is None
    _assert_current(d2, occ, None, True, 2, "map-only update")
    _push(oracle, d2, world, (p0[0] + 0.6, p0[1], p0[2]))
    win, occ, rgb, _ = d2.map_update(True, 2, image=True)
    assert win == FULL
    _assert_current(d2, occ, rgb, True, 2, "image switched on")


def test_other_extractions_between_updates_change_nothing(oracle):
    world = synth.World("room", GC)
    dg = _grid()
    y = world.cy - world.hy + 1.0
    _push(oracle, dg, world, (world.cx - 6.0, y, 0.0))
    dg.map_update(True, 2)
    _push(oracle, dg, world, (world.cx - 5.5, y, 0.0))
    dg.occupancy(False, 7)                                          # another extraction, other parameters
    grp = multigpu.LocalOccupancyGroup([dg])
    grp.merge_async(True, 4)
    grp.wait()
    win, occ, rgb, _ = dg.map_update(True, 2)
    assert 0 < win[2] <= N // 2
    _assert_current(dg, occ, rgb, True, 2, "after tsd_occupancy and a group extraction")
    grp.close()
    # a full frame between two updates is the previous frame of the next update: that one covers the later pushes only
    _push(oracle, dg, world, (world.cx - 5.0, y, 0.0))
    dg.map_frame(True, 2)
    win0 = dg.map_update_begin(True, 2)
    dg.map_update_wait()
    assert win0[2] == 0, f"nothing was pushed since the frame: window {win0}"
    far = (world.cx + 6.0, world.cy + world.hy - 1.0, 0.0)
    _push(oracle, dg, world, far)
    win, occ, rgb, _ = dg.map_update(True, 2)
    _assert_current(dg, occ, rgb, True, 2, "after a full frame")
    # (the push's launch window also covers the previous push's tiles; the frame in between did not widen it further)
    assert 0 < win[2] <= N // 2 + 64 and win[0] + win[2] > int(far[0] / GC.cell_size)


def test_updates_behind_batched_pushes(oracle):
    from tests.test_gpu_batch import _setup
    n_robots, n_scans = 2, 5
    gc, geo, kw, og, dg, robots, scans, sensors, params, gates = _setup(oracle, "cfg1", n_robots, n_scans)
    batch = capi.TsdBatch(dg, n_robots)
    pushed = 0
    for k in range(1, n_scans):
        ing = [rb.ingest(sc[k]) for rb, sc in zip(robots, scans)]
        batch.begin(sensors, [x[0] for x in ing], [x[1] for x in ing], [x[2] for x in ing], params, gates)
        batch.push()
        win = dg.map_update_begin(True, 2)                          # right behind the batch's push, nothing synchronised
        occ, rgb, _ = dg.map_update_wait()
        pushed += sum(int(sr.pushed) for sr in batch.results())
        dg.sync()
        assert win[2] > 0
        want, _ = dg.occupancy(True, 2)
        assert np.array_equal(occ, want), f"round {k} window {win}: {np.count_nonzero(occ != want)} cells differ"
        assert np.array_equal(rgb, dg.color_image(gc.cells, gc.cells)), f"round {k}: image differs"
    assert pushed >= 2
    batch.close()
    for s in sensors:
        s.close()


def test_updates_behind_asynchronous_pushes(oracle):
    gc = synth.GridConfig(9, 0.05)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 7))
    sh = HipSlamFused(oracle, **slam_kwargs(gc, geo))
    pushed = 0
    for k, r in enumerate(scans):
        out = sh.process_scan(r)
        if k == 0:
            sh.sensor.set_async_mapping(True)
        pushed += out["pushed"]
        win, occ, rgb, _ = sh.grid.map_update(True, 2)
        want, _ = sh.grid.occupancy(True, 2)
        assert np.array_equal(occ, want), f"scan {k} window {win}: {np.count_nonzero(occ != want)} cells differ"
        assert np.array_equal(rgb, sh.grid.color_image(gc.cells, gc.cells)), f"scan {k}: image differs"
    assert pushed >= 3


def _node_run(updates_on):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    # a sensor that sees 4 m, started 2 m and 1.5 m from two walls of the room: the pushes' windows are a part of the 512^2 map
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 8))
    over = dict(use_object_inflation=True, object_inflation_factor=2, occ_grid_time_interval=1000.0)
    if updates_on is not None:
        over["publish_map_updates"] = updates_on
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    maps, upds = [], []
    try:
        for k, s in enumerate(scans):
            node.laser(s, geo.angle_min, geo.angle_increment)
            if k % 2 == 0:
                continue
            node.publish_map()
            maps.append((node.map_msg(), node.get_map()["data"].copy(), node.map_image_msg()["data"].copy(),
                         node.grid().color_image(gc.cells, gc.cells), node.grid().occupancy(True, 2)[0]))
            upds.append((node.map_updates(), node.map_update_msg()))
        node.publish_map()                                         # nothing was pushed since: no message with updates on
        last = (node.map_msg()["count"], node.map_updates(), node.map_frames())
    finally:
        node.close()
    return maps, upds, last


def test_node_publishes_update_messages():
    maps, upds, last = _node_run(True)
    first = maps[0][0]
    assert first["count"] == 1 and upds[0][0] == 0, "the first publication is a full map"
    pasted = first["data"].copy()
    for k in range(1, len(maps)):
        m, got, img, want_img, want = maps[k]
        n_upd, u = upds[k]
        assert m["count"] == 1 and n_upd == k and u["count"] == k, f"publication {k}: not an update message"
        assert 0 < u["width"] < first["width"] and 0 < u["height"] < first["height"], f"publication {k}: window {u['width']} x {u['height']}"
        assert u["frame_id"] == first["frame_id"] and u["stamp_ns"] > first["stamp_ns"]
        pasted[u["y"]:u["y"] + u["height"], u["x"]:u["x"] + u["width"]] = u["data"]
        assert np.array_equal(pasted, got), f"publication {k}: first map + updates != get_map ({np.count_nonzero(pasted != got)} cells)"
        assert np.array_equal(got, want), f"publication {k}: get_map is not the current map"
        assert np.array_equal(img, want_img), f"publication {k}: the image message is not the full current image"
    assert (pasted == 100).sum() > 0 and not np.array_equal(pasted, first["data"])
    assert last == (1, len(maps) - 1, 1), "a publication with nothing pushed produced a message"
    # with the parameter off (and absent) nothing changes: full maps only, and the same maps
    off, off_upds, off_last = _node_run(False)
    absent, absent_upds, _ = _node_run(None)
    for k in range(len(maps)):
        assert off[k][0]["count"] == k + 1 and off_upds[k][0] == 0 and off_upds[k][1]["width"] == 0
        assert absent[k][0]["count"] == k + 1 and absent_upds[k][0] == 0
        for run in (off, absent):                                   # <node>/map, get_map and the image as they are today
            assert np.array_equal(run[k][0]["data"], run[k][4]) and np.array_equal(run[k][1], run[k][4])
            assert np.array_equal(run[k][2], run[k][3])
    assert off_last == (len(maps) + 1, 0, len(maps) + 1)
