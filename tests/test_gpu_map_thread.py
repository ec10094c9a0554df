"""GPU tests of the façade's ThreadGrid (csrc/host/ThreadGrid.cpp): what SlamNode publishes on <node>/map and <node>/map/image
every occ_grid_time_interval and answers on <node>/get_map (ThreadGrid.cpp:16-142), built from the device's map frames."""
import time

import numpy as np
import pytest

from ohm_tsd_slam_amd import facade, synth

pytestmark = pytest.mark.gpu


def _scans(cfg, n, start_xy=None):
    gc, geo, scene = synth.CONFIGS[cfg]
    world = synth.World(scene, gc, start_xy=start_xy)
    return gc, geo, synth.scans_for(world, geo, synth.trajectory(world, n))


def _oracle_maps(oracle, node, gc, content, inflate, factor):
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    og.load(*node.grid().download_tiles())
    occ, n = og.occupancy(content, inflate, factor)
    return occ.reshape(gc.cells, gc.cells), n, og.color_image(gc.cells, gc.cells)


def test_published_map_follows_the_reference(oracle):
    gc, geo, scans = _scans("cfg1", 6)
    xo, yo = 0.3, -0.2
    params = facade.node_params(gc, geo, x_offset=xo, y_offset=yo, tf_map_frame="world", use_object_inflation=True,
                                object_inflation_factor=3, occ_grid_time_interval=1000.0)
    node = facade.SlamNode(params, synchronous=True)
    content = np.full(gc.cells * gc.cells, -1, dtype=np.int8)
    try:
        for k, s in enumerate(scans):
            node.laser(s, geo.angle_min, geo.angle_increment)
            if k % 2 == 0:
                continue
            node.publish_map()
            m, im = node.map_msg(), node.map_image_msg()
            occ, n, img = _oracle_maps(oracle, node, gc, content, True, 3)     # use_object_inflation / factor reach the marks
            assert np.array_equal(m["data"], occ), f"scan {k}: {np.count_nonzero(m['data'] != occ)} cells differ"
            assert np.array_equal(im["data"], img), f"scan {k}: image differs"
            assert n > 0 and (m["data"] == 100).sum() > 0
        N, cs = gc.cells, gc.cell_size
        assert m["count"] == 3 and im["count"] == 3 and node.map_frames() == 3
        assert m["resolution"] == pytest.approx(np.float32(cs), rel=0, abs=0)
        assert (m["width"], m["height"]) == (N, N)
        assert m["origin_position"][0] == -(N * cs * 0.5 + xo) and m["origin_position"][1] == -(N * cs * 0.5 + yo)
        assert list(m["origin_orientation_xyzw"]) == [0.0, 0.0, 0.0, 1.0] and m["origin_position"][2] == 0.0
        assert m["frame_id"] == "world" and m["stamp_ns"] > 0 and m["map_load_time_ns"] >= m["stamp_ns"]
        assert (im["height"], im["width"], im["step"]) == (N, N, 3 * N)
        assert im["encoding"] == "rgb8" and im["frame_id"] == "map" and im["stamp_ns"] == m["stamp_ns"]
        g = node.get_map()
        assert np.array_equal(g["data"], m["data"]) and g["frame_id"] == "world" and g["stamp_ns"] >= m["stamp_ns"]
        assert (g["width"], g["height"], g["resolution"]) == (N, N, m["resolution"])
    finally:
        node.close()


def test_timer_publishes_while_scans_run():
    gc, geo, scans = _scans("cfg1", 30)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.02), synchronous=False)
    try:
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
            time.sleep(0.005)
        assert node.wait_idle(20000)
        t0 = time.time()
        while node.map_frames() < 4 and time.time() - t0 < 10:
            time.sleep(0.02)
        assert node.map_frames() >= 4
        m = node.map_msg()
        assert m["count"] >= 4 and (m["data"] == 100).sum() > 0 and (m["data"] == 0).sum() > 0
        assert node.processed() > 0
    finally:
        node.close()


def test_multi_robot_node_publishes(oracle):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    W = gc.width
    params = facade.node_params(gc, geo, robot_nbr=2, occ_grid_time_interval=1000.0)
    params.update({"tsd_slam/robot_1/local_offset_x": 0.7 + 0.37, "tsd_slam/robot_1/local_offset_y": 0.4 - 0.21})
    node = facade.SlamNode(params, synchronous=True)
    content = np.full(gc.cells * gc.cells, -1, dtype=np.int8)
    try:
        s = []
        for off in ((0.0, 0.0), (0.7, 0.4)):
            w = synth.World(scene, gc, start_xy=[0.5 * W + off[0], 0.5 * W + off[1]])
            s.append(synth.scans_for(w, geo, synth.trajectory(w, 4)))
        for k in range(4):
            for r in range(2):
                node.laser(s[r][k], geo.angle_min, geo.angle_increment, robot=r)
        node.publish_map()
        m = node.map_msg()
        occ, n, img = _oracle_maps(oracle, node, gc, content, False, 2)
        assert n > 0 and np.array_equal(m["data"], occ)
        assert np.array_equal(node.map_image_msg()["data"], img)
    finally:
        node.close()


def test_destroying_the_node_while_it_publishes_returns():
    gc, geo, scans = _scans("cfg2", 6)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.001), synchronous=True)
    for s in scans:
        node.laser(s, geo.angle_min, geo.angle_increment)
    t0 = time.time()
    while node.map_frames() < 1 and time.time() - t0 < 20:
        time.sleep(0.001)
    assert node.map_frames() >= 1
    node.close()              # the timer keeps the ThreadGrid busy: a frame is (almost always) in flight here
    assert node.h is None
