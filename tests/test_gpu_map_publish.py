"""ThreadGrid's publication as one device frame (tsd_map_frame_begin / tsd_map_frame_wait, csrc/map_publish.hip).

A frame is the occupancy map of tsd_occupancy and the image of tsd_color_image(cells, cells), built by one pass over the tiles and
copied to the host beside the scans.  The frames below are compared with both existing extraction paths on an identical second
device grid and with the oracle, over several frames in a row (the persistent map carries state from one frame to the next), and
they are taken right behind the three kinds of push (fused scan, asynchronous mapping, batched push) without any synchronisation.
"""
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, synth
from tests import helpers as H
from tests.slam_driver import HipSlamFused, slam_kwargs

pytestmark = pytest.mark.gpu

# (inflate, factor) of the frames in turn
FRAME_PARAMS = [(False, 2), (True, 2), (True, 3), (False, 2), (True, 3)]


def _pose(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]])


def _push_all(oracle, grids, geo, pose, r32):
    data, mask = oracle.ingest_f32(np.asarray(r32, dtype=np.float32), H.MAX_RANGE, geo.angle_increment)
    for g in grids:
        if isinstance(g, capi.TsdGridDevice):
            g.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL, want_stats=False)
        else:
            g.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)


@pytest.mark.parametrize("map_log2,cs,scene", [(9, 0.05, "room"), (12, 0.02, "room")])
def test_frames_equal_both_extraction_paths_and_the_oracle(oracle, map_log2, cs, scene):
    gc = synth.GridConfig(map_log2, cs)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World(scene, gc)
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    da = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)      # frames
    db = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)      # tsd_occupancy + tsd_color_image
    grids = (og, da, db)
    N, tw = gc.cells, 32 * gc.cell_size
    content = np.full(N * N, -1, dtype=np.int8)
    pose0, (x0, y0, _) = H.sensor_pose(world, 0)
    for g in grids:                                                           # empty (freeFootprint) tiles
        g.free_footprint([x0 + 3 * tw, y0], 2.5 * tw, 1.5 * tw)
    ring = np.full(geo.beams, 0.7 * tw, dtype=np.float32)
    steps = [
        (pose0, None),                                                        # surfaces, NaN cells, tile borders
        (_pose(0.9 * tw, 0.9 * tw, 0.0), ring),                               # surfaces on the outer tile ring (corner)
        (H.sensor_pose(world, 6)[0], np.full(geo.beams, 2.0, dtype=np.float32)),
        (_pose(gc.width - 0.9 * tw, 0.5 * gc.width, 0.3), ring),             # the far ring, across a tile row border
        (H.sensor_pose(world, 12)[0], None),
    ]
    for k, (pose, r) in enumerate(steps):
        if r is None:
            x, y, yaw = pose[0, 2], pose[1, 2], math.atan2(pose[1, 0], pose[0, 0])
            r = world.scan(x, y, yaw, geo)
        _push_all(oracle, grids, geo, pose, r)
        inflate, factor = FRAME_PARAMS[k % len(FRAME_PARAMS)]
        image = k != 2                                                        # one map-only frame
        fo, frgb, fn = da.map_frame(inflate=inflate, factor=factor, image=image)
        bo, bn = db.occupancy(inflate, factor)
        oo, on = og.occupancy(content, inflate, factor)
        assert fo.shape == (N, N) and fo.dtype == np.int8
        assert fn == bn == on and fn > 0, f"frame {k}: surface counts {fn} / {bn} / {on}"
        assert np.array_equal(fo, bo), f"frame {k}: {np.count_nonzero(fo != bo)} cells differ from tsd_occupancy"
        assert np.array_equal(fo, oo.reshape(N, N)), f"frame {k}: {np.count_nonzero(fo != oo.reshape(N, N))} cells differ from the oracle"
        if not image:
            assert frgb is None
            continue
        bi = db.color_image(N, N)
        oi = og.color_image(N, N)
        assert frgb.shape == (N, N, 3)
        assert np.array_equal(frgb, bi), f"frame {k}: image differs from tsd_color_image at {np.argwhere(frgb != bi)[:5]}"
        assert np.array_equal(frgb, oi), f"frame {k}: image differs from the oracle at {np.argwhere(frgb != oi)[:5]}"
    # what the grid had to hold for this to mean anything
    ti, tiw = da.download_tile_state()
    PX = N // 32
    ring_tiles = np.zeros((PX, PX), bool)
    ring_tiles[0, :] = ring_tiles[-1, :] = ring_tiles[:, 0] = ring_tiles[:, -1] = True
    assert (ti.reshape(PX, PX) & ring_tiles).any(), "no initialised tile on the outer ring"
    assert ((ti == 0) & (tiw > 0)).any() and ((ti == 0) & (tiw == 0)).any(), "no empty / no untouched tile"
    assert (fo == 100).sum() > 100 and (fo == 0).sum() > 1000 and (fo == -1).any()
    assert (frgb.sum(axis=2) == 3 * 255).any() and (frgb.sum(axis=2) == 0).any() and (frgb[..., 1] == 255).any()
    # surfaces on the outer ring show in the image (black pixel row / column 0 aside)
    edge = frgb[1:33, 1:33]
    assert ((edge[..., 1] == 0) & (edge[..., 0] > 0)).any() or (edge[..., 1] == 255).any()


def test_second_begin_is_refused_and_wait_needs_a_frame(oracle):
    gc = synth.GridConfig(8, 0.05)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    dg = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    pose, (x, y, yaw) = H.sensor_pose(world, 0)
    _push_all(oracle, (dg,), geo, pose, world.scan(x, y, yaw, geo))
    with pytest.raises(capi.TsdError, match="no frame in flight"):
        dg.map_frame_wait()
    dg.map_frame_begin()
    with pytest.raises(capi.TsdError, match="in flight"):
        dg.map_frame_begin(image=False)
    occ, rgb, n = dg.map_frame_wait()
    assert n > 0 and rgb is not None
    occ2, rgb2, n2 = dg.map_frame()                     # the context takes the next frame again
    assert n2 == n and np.array_equal(occ, occ2) and np.array_equal(rgb, rgb2)


def _oracle_of(oracle, dg, gc):
    """an oracle grid holding the device grid's current content (cells and halos, as the device has them)"""
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    og.load(*dg.download_tiles())
    return og


def _check_frame_against_grid(oracle, dg, gc, frame, content, inflate, factor, what):
    occ, rgb, n = frame
    og = _oracle_of(oracle, dg, gc)
    oo, on = og.occupancy(content, inflate, factor)
    assert n == on, f"{what}: surface count {n} != {on}"
    assert np.array_equal(occ, oo.reshape(gc.cells, gc.cells)), f"{what}: {np.count_nonzero(occ != oo.reshape(gc.cells, gc.cells))} cells differ"
    assert np.array_equal(rgb, og.color_image(gc.cells, gc.cells)), f"{what}: image differs"


@pytest.mark.parametrize("async_map", [False, True])
def test_frame_right_behind_a_fused_scan_reflects_its_push(oracle, async_map):
    """tsd_scan leaves the push's halo pass to the ray cast it enqueues behind the push; with asynchronous mapping the push is on the
    push stream.  A frame begun right after the scan returns must hold the push, halos included: it equals the oracle's extraction
    from the device grid as it stands once everything has finished (nothing is enqueued after the frame)."""
    gc = synth.GridConfig(9, 0.05)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 7))
    kw = slam_kwargs(gc, geo)
    sh = HipSlamFused(oracle, **kw)
    content = np.full(gc.cells * gc.cells, -1, dtype=np.int8)
    pushed = 0
    for k, r in enumerate(scans):
        out = sh.process_scan(r)
        if k == 0 and async_map:
            sh.sensor.set_async_mapping(True)
        pushed += out["pushed"]
        inflate, factor = FRAME_PARAMS[k % len(FRAME_PARAMS)]
        frame = sh.grid.map_frame(inflate=inflate, factor=factor)
        _check_frame_against_grid(oracle, sh.grid, gc, frame, content, inflate, factor, f"scan {k}")
        assert frame[2] > 0
    assert pushed >= 3


def test_frame_right_behind_a_batched_push_reflects_it(oracle):
    from tests.test_gpu_batch import _setup
    n_robots, n_scans = 3, 5
    gc, geo, kw, og, dg, robots, scans, sensors, params, gates = _setup(oracle, "cfg1", n_robots, n_scans)
    batch = capi.TsdBatch(dg, n_robots)
    content = np.full(gc.cells * gc.cells, -1, dtype=np.int8)
    pushed = 0
    for k in range(1, n_scans):
        ing = [rb.ingest(sc[k]) for rb, sc in zip(robots, scans)]
        batch.begin(sensors, [x[0] for x in ing], [x[1] for x in ing], [x[2] for x in ing], params, gates)
        batch.push()
        dg.map_frame_begin(inflate=True, factor=2)            # right behind the batch's push, nothing synchronised
        frame = dg.map_frame_wait()
        pushed += sum(int(sr.pushed) for sr in batch.results())
        dg.sync()
        _check_frame_against_grid(oracle, dg, gc, frame, content, True, 2, f"round {k}")
    assert pushed >= 2
    batch.close()
    for s in sensors:
        s.close()
