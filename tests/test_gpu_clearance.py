"""The clearance field and the cost map on the device (csrc/clearance.hip; tsd_clearance_dev, tsd_costmap_begin / _wait, the facade's
<node>/costmap) against the numpy restatement of tests/clearance_ref.py: every comparison is byte for byte."""
import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, multigpu, synth
from tests import clearance_ref as R_
from tests import helpers as H

pytestmark = pytest.mark.gpu

# (width, height, stride) and three radii each; every radius of {1, 2, 7, 31, 32, 33, 64, 255} at least once: they sit on both sides
# of the steps at which the tile summary's reach (and the mask words a row reads) grow
SHAPES = {
    "256x256": ((256, 256, 256), (31, 64, 255)),
    "200x137_stride208": ((200, 137, 208), (7, 32, 33)),
    "33x65": ((33, 65, 33), (1, 2, 33)),
    "16x16": ((16, 16, 16), (2, 7, 255)),
    "1x300": ((1, 300, 1), (1, 31, 64)),
}
CASES = [(name, R) for name, (_, radii) in SHAPES.items() for R in radii]
SENTINEL = (0xABCD, 0x55)


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


def _upload(grid, src, stride):
    """the map as `height` rows of `stride` bytes on the device; the padding holds 100s, which must not be read as obstacles"""
    H_, W = src.shape
    padded = np.full((H_, stride), 100, dtype=np.int8)
    padded[:, :W] = src
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    return buf


def _base(rng, W, H_):
    return rng.choice(np.array([-1, 0], dtype=np.int8), size=(H_, W))


def _contents(rng, W, H_, R):
    """name -> map"""
    out = {}
    out["no_obstacle"] = _base(rng, W, H_)
    m = _base(rng, W, H_)
    for y in (0, H_ // 2, H_ - 1):
        for x in (0, W // 2, W - 1):
            if (x, y) != (W // 2, H_ // 2):
                m[y, x] = 100
    out["corners_and_mid_edges"] = m
    out["all_obstacles"] = np.full((H_, W), 100, dtype=np.int8)
    for name, p in (("density_1e-3", 1e-3), ("density_0.3", 0.3)):
        m = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(H_, W), p=[(1 - p) / 2, (1 - p) / 2, p])
        if p < 0.01:
            m[rng.integers(H_), rng.integers(W)] = 100
        out[name] = m
    m = _base(rng, W, H_)                      # a one-cell wall along a tile seam
    if W > 32:
        m[:, 32] = 100
    elif H_ > 32:
        m[32, :] = 100
    else:
        m[H_ // 2, :] = 100
    out["seam_wall"] = m
    return out


def _check(grid, src, stride, R, tab, what):
    H_, W = src.shape
    buf = _upload(grid, src, stride)
    try:
        d2, cost = grid.clearance_of(buf.ptr, W, H_, stride, R, table=tab, prefill=SENTINEL)
    finally:
        buf.free()
    want_d2, want_c = R_.both(src, R, tab)
    assert np.array_equal(d2, want_d2), f"{what}: {np.count_nonzero(d2 != want_d2)} d2 cells differ at {np.argwhere(d2 != want_d2)[:4]}"
    assert np.array_equal(cost, want_c), f"{what}: {np.count_nonzero(cost != want_c)} cost cells differ at {np.argwhere(cost != want_c)[:4]}"
    return d2, cost


@pytest.mark.parametrize("name,R", CASES)
def test_shapes_radii_and_contents_equal_the_restatement(grid, name, R):
    (W, H_, stride), _ = SHAPES[name]
    rng = np.random.default_rng(1000 * R + W)
    tab = R_.table(0.05, R, 0.12, 1.5)
    tab[1:] = np.maximum(tab[1:] - (np.arange(1, tab.size) % 3 == 0), 1)       # not monotone: T is a table, nothing else is assumed
    for what, src in _contents(rng, W, H_, R).items():
        _check(grid, src, stride, R, tab, f"{name} R={R} {what}")


@pytest.mark.parametrize("name,R", [c for c in CASES if c[0] in ("256x256", "200x137_stride208", "1x300")])
def test_probe_exactly_at_the_radius(grid, name, R):
    """an obstacle exactly R away counts (d2 = R^2), one sqrt(R^2 + 1) away does not"""
    (W, H_, stride), _ = SHAPES[name]
    tab = R_.table(0.05, R, 0.12, 1.5)
    if W > R + 1:
        probe, at_r, beyond = (0, 1), (R, 1), (R, 0)          # (x, y): offsets (R, 0) and (R, -1)
    else:
        probe, at_r, beyond = (0, 0), (0, R), None            # one column: only the vertical probe exists
    assert at_r[0] < W and at_r[1] < H_
    src = np.zeros((H_, W), dtype=np.int8)
    src[at_r[1], at_r[0]] = 100
    d2, _ = _check(grid, src, stride, R, tab, f"{name} R={R} obstacle at R")
    assert d2[probe[1], probe[0]] == R * R
    if beyond is not None:
        src = np.zeros((H_, W), dtype=np.int8)
        src[beyond[1], beyond[0]] = 100
        d2, cost = _check(grid, src, stride, R, tab, f"{name} R={R} obstacle at sqrt(R^2 + 1)")
        assert d2[probe[1], probe[0]] == 0xFFFF and cost[probe[1], probe[0]] == 0


@pytest.mark.parametrize("name,R", [("256x256", 7), ("200x137_stride208", 33), ("256x256", 64)])
def test_windows_write_only_their_cells(grid, name, R):
    (W, H_, stride), _ = SHAPES[name]
    rng = np.random.default_rng(77 + R)
    src = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(H_, W), p=[0.3, 0.69, 0.01])
    tab = R_.table(0.05, R, 0.12, 1.5)
    want_d2, want_c = R_.both(src, R, tab)
    windows = [(W // 2, H_ // 2, 1, 1), (16, 32, 64, 48), (5, 9, 77, 41), (0, 20, 9, 30), (21, 0, 50, 3), (W - 13, 11, 13, 40),
               (3, H_ - 7, 100, 7), (0, 0, W, H_)]
    buf = _upload(grid, src, stride)
    try:
        for win in windows:
            x, y, w, h = win
            d2, cost = grid.clearance_of(buf.ptr, W, H_, stride, R, window=win, table=tab, prefill=SENTINEL)
            inside = np.zeros((H_, W), bool)
            inside[y:y + h, x:x + w] = True
            assert (d2[~inside] == SENTINEL[0]).all() and (cost[~inside] == SENTINEL[1]).all(), f"{win}: written outside the window"
            assert np.array_equal(d2[inside], want_d2[inside]) and np.array_equal(cost[inside], want_c[inside]), f"window {win}"
        # the distance field alone
        d2, cost = grid.clearance_of(buf.ptr, W, H_, stride, R, window=(5, 9, 77, 41), prefill=SENTINEL)
        assert cost is None and np.array_equal(d2[9:50, 5:82], want_d2[9:50, 5:82]) and d2[0, 0] == SENTINEL[0]
    finally:
        buf.free()


@pytest.mark.parametrize("R", [31, 64])
def test_tile_skip_changes_nothing(grid, R):
    """a map that is nine tenths empty: most workgroups skip; with the skip off the bytes are the same"""
    W = H_ = 512
    rng = np.random.default_rng(5 + R)
    src = rng.choice(np.array([-1, 0], dtype=np.int8), size=(H_, W))
    src[40:90, 300:460][rng.random((50, 160)) < 0.05] = 100          # 50 x 160 of 512 x 512 cells hold the obstacles
    src[H_ - 1, 0] = 100
    tab = R_.table(0.05, R, 0.12, 1.5)
    want_d2, want_c = R_.both(src, R, tab)
    assert (want_d2 == 0xFFFF).mean() > 0.5
    buf = _upload(grid, src, W)
    try:
        on = grid.clearance_of(buf.ptr, W, H_, W, R, table=tab, prefill=SENTINEL)
        grid.set_clearance_skip(False)
        try:
            off = grid.clearance_of(buf.ptr, W, H_, W, R, table=tab, prefill=SENTINEL)
        finally:
            grid.set_clearance_skip(True)
    finally:
        buf.free()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[0], want_d2) and np.array_equal(on[1], want_c)


def test_refusals(grid):
    src = np.zeros((16, 16), dtype=np.int8)
    buf = _upload(grid, src, 16)
    try:
        for kw in (dict(radius=0), dict(radius=256), dict(radius=3, window=(10, 0, 7, 4)), dict(radius=3, window=(0, -1, 4, 4)),
                   dict(radius=3, window=(0, 0, 0, 4))):
            with pytest.raises(capi.TsdError):
                grid.clearance_of(buf.ptr, 16, 16, 16, kw["radius"], window=kw.get("window"))
            assert grid.last_rc == -1
        with pytest.raises(capi.TsdError):
            grid.clearance_of(buf.ptr, 16, 16, 15, 3)                    # stride < width
        with pytest.raises(capi.TsdError):
            grid.clearance_of(0, 16, 16, 16, 3)
        d2, _ = grid.clearance_of(buf.ptr, 16, 16, 16, 3)                # ... and the context still works
        assert (d2 == 0xFFFF).all()
    finally:
        buf.free()


# ---- the cost map of a frame: a pushed grid
GC = synth.GridConfig(8, 0.1)
GEO = synth.ScanGeometry.full_circle_360()
N = GC.cells
SHORT_RANGE = 3.0
RADIUS = 6
COST = dict(inscribed_radius_m=0.25, cost_scaling=3.0)


def _push(oracle, dg, world, pose3):
    x, y, yaw = pose3
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, GEO), SHORT_RANGE, GEO.angle_increment)
    dg.push(synth.pose_matrix(x, y, yaw), data, mask, GEO.angle_increment, GEO.angle_min, SHORT_RANGE, H.MIN_RANGE, H.LOW_REFL,
            want_stats=False)


def _corner_poses(world, k0, k1):
    """2 m and 1.5 m inside the room's lower left corner, 0.3 m along x per scan"""
    return [(world.cx - world.hx + 2.0 + 0.3 * k, world.cy - world.hy + 1.5, 0.1 + 0.02 * k) for k in range(k0, k1)]


def test_costmap_of_a_pushed_grid_and_its_windowed_update(oracle):
    world = synth.World("room", GC)
    dg = capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)
    tab = dg.costmap_table(RADIUS, **COST)
    assert np.array_equal(tab, R_.table(GC.cell_size, RADIUS, COST["inscribed_radius_m"], COST["cost_scaling"]))
    for pose in _corner_poses(world, 0, 8):
        _push(oracle, dg, world, pose)
    occ, _, ns = dg.map_frame(False, 2, image=False)
    assert ns > 0 and (occ == 100).sum() > 20
    win, cost, d2 = dg.costmap(RADIUS, want_dist2=True, **COST)
    want_d2, want_c = R_.both(occ, RADIUS, tab)
    assert win == (0, 0, N, N)
    assert np.array_equal(d2, want_d2) and np.array_equal(cost, want_c)
    assert (cost == 99).sum() > 0 and (cost == -1).sum() > 0 and ((cost > 0) & (cost < 99)).sum() > 0

    # more pushes, a windowed update, the cost map of its window into the same buffers
    for pose in _corner_poses(world, 8, 11):
        _push(oracle, dg, world, pose)
    mwin, occ2, _, _ = dg.map_update(False, 2, image=False)
    assert 0 < mwin[2] < N or 0 < mwin[3] < N, f"the update's window is the whole map: {mwin}"
    assert (occ2 != occ).any()
    cwin, cost2, d22 = dg.costmap(RADIUS, map_win=mwin, want_dist2=True, **COST)
    assert cwin == R_.grown(mwin, RADIUS, N, N)
    want_d2, want_c = R_.both(occ2, RADIUS, tab)
    assert np.array_equal(d22, want_d2) and np.array_equal(cost2, want_c), "the patched buffers are not the full recomputation"

    # an empty update enqueues nothing
    ewin, occ3, _, _ = dg.map_update(False, 2, image=False)
    assert ewin == (0, 0, 0, 0) and np.array_equal(occ3, occ2)
    mine = np.full((N, N), 0x55, dtype=np.int8)
    assert dg.costmap_begin(RADIUS, map_win=ewin, cost=mine, **COST) == (0, 0, 0, 0)
    c3, _ = dg.costmap_wait()
    assert (c3 == 0x55).all()

    # the same field in metres
    metres = dg.clearance(RADIUS)
    near = want_d2 != 0xFFFF
    assert metres.dtype == np.float32 and np.isinf(metres[~near]).all()
    assert np.array_equal(metres[near], (np.sqrt(want_d2[near].astype(np.float64)) * GC.cell_size).astype(np.float32))


def test_costmap_refusals(oracle):
    world = synth.World("room", GC)
    dg = capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)

    def refused(**kw):
        with pytest.raises(capi.TsdError):
            dg.costmap_begin(kw.pop("radius", RADIUS), **kw)
        assert dg.last_rc == -1

    refused()                                      # no previous frame
    _push(oracle, dg, world, _corner_poses(world, 0, 1)[0])
    dg.map_frame_begin(False, 2, image=False)
    refused()                                      # a frame in flight
    dg.map_frame_wait()
    refused(radius=0)
    refused(radius=256)
    refused(map_win=(N - 10, 0, 20, 5))            # a window outside the map
    refused(map_win=(-1, 0, 20, 5))
    assert dg.costmap_begin(RADIUS) == (0, 0, N, N)
    refused()                                      # a second cost map
    with pytest.raises(capi.TsdError):             # a frame begun while a cost map is in flight is refused like a second frame
        dg.map_frame_begin(False, 2, image=False)
    with pytest.raises(capi.TsdError):
        dg.map_update_begin(False, 2, image=False)
    cost, _ = dg.costmap_wait()
    occ, _, _ = dg.map_frame(False, 2, image=False)
    assert np.array_equal(cost, R_.both(occ, RADIUS, dg.costmap_table(RADIUS))[1])
    with pytest.raises(capi.TsdError):
        dg.costmap_wait()                          # none in flight


def test_clearance_of_a_groups_merged_map():
    rng = np.random.default_rng(11)
    grids = [capi.TsdGridDevice(8, 0.05, 0.15) for _ in range(2)]
    maps = [rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(g.cells, g.cells), p=[0.4, 0.597, 0.003]) for g in grids]
    grp = multigpu.LocalOccupancyGroup(grids, [(0, 0), (17, -40)])
    try:
        grp.merge_maps_async(maps)
        merged = grp.merged()
        assert (merged == 100).sum() > 100
        R = 13
        tab = grids[0].costmap_table(R, 0.2, 4.0)
        ptr = grp.lib.tsd_group_map_dev(grp.h)
        d2, cost = grids[0].clearance_of(ptr, grp.width, grp.height, grp.width, R, table=tab)
        want_d2, want_c = R_.both(merged, R, tab)
        assert merged.shape == (grp.height, grp.width) and grp.width % 8 != 0
        assert np.array_equal(d2, want_d2) and np.array_equal(cost, want_c)
    finally:
        grp.close()


# ---- the facade: <node>/costmap and <node>/costmap_updates
def _node_run(costmap_on, updates_on):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 8))
    over = dict(occ_grid_time_interval=1000.0, publish_map_updates=updates_on)
    if costmap_on is not None:
        over["publish_costmap"] = costmap_on
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    out = []
    try:
        radius = node.costmap_radius_cells()
        for k, s in enumerate(scans):
            node.laser(s, geo.angle_min, geo.angle_increment)
            if k % 2 == 0:
                continue
            node.publish_map()
            out.append(dict(map=node.map_msg(), map_update=node.map_update_msg(), costmap=node.costmap_msg(),
                            costmap_update=node.costmap_update_msg(), costmaps=node.costmaps()))
        node.publish_map()                     # nothing was pushed since: with updates on, no message
        last = dict(costmaps=node.costmaps(), costmap=node.costmap_msg(), costmap_update=node.costmap_update_msg())
    finally:
        node.close()
    return gc, radius, out, last


def test_node_publishes_the_costmap_of_every_map():
    gc, radius, out, last = _node_run(True, False)
    assert radius == 11                         # ceil(0.55 / 0.05)
    tab = capi.costmap_table(gc.cell_size, radius, 0.25, 10.0)
    for k, o in enumerate(out):
        m, c = o["map"], o["costmap"]
        assert c["topic"] == "tsd_slam/costmap" and c["count"] == m["count"] == k + 1 and o["costmaps"] == k + 1
        assert c["frame_id"] == m["frame_id"] and c["stamp_ns"] == m["stamp_ns"] and c["resolution"] == m["resolution"]
        assert (c["width"], c["height"]) == (m["width"], m["height"]) and np.array_equal(c["origin_position"], m["origin_position"])
        assert np.array_equal(c["data"], R_.both(m["data"], radius, tab)[1]), f"publication {k}"
    assert (out[-1]["costmap"]["data"] == 99).sum() > 0
    assert last["costmaps"] == len(out) + 1 and last["costmap_update"]["count"] == 0


def test_node_publishes_costmap_updates():
    gc, radius, out, last = _node_run(True, True)
    tab = capi.costmap_table(gc.cell_size, radius, 0.25, 10.0)
    first = out[0]
    assert first["costmap"]["count"] == 1 and first["costmap_update"]["count"] == 0, "the first publication is a full cost map"
    pasted_map, pasted = first["map"]["data"].copy(), first["costmap"]["data"].copy()
    assert np.array_equal(pasted, R_.both(pasted_map, radius, tab)[1])
    for k in range(1, len(out)):
        mu, cu = out[k]["map_update"], out[k]["costmap_update"]
        assert out[k]["costmap"]["count"] == 1 and cu["count"] == mu["count"] == k and out[k]["costmaps"] == k + 1
        assert (cu["x"], cu["y"], cu["width"], cu["height"]) == R_.grown((mu["x"], mu["y"], mu["width"], mu["height"]), radius, gc.cells, gc.cells)
        assert cu["stamp_ns"] == mu["stamp_ns"] and cu["frame_id"] == mu["frame_id"]
        pasted_map[mu["y"]:mu["y"] + mu["height"], mu["x"]:mu["x"] + mu["width"]] = mu["data"]
        pasted[cu["y"]:cu["y"] + cu["height"], cu["x"]:cu["x"] + cu["width"]] = cu["data"]
    assert len(out) >= 3 and out[-1]["map_update"]["width"] < gc.cells
    assert np.array_equal(pasted, R_.both(pasted_map, radius, tab)[1]), "the first cost map patched by every update is not the final map's"
    assert last["costmaps"] == len(out), "an empty update published a cost map"


@pytest.mark.parametrize("costmap_on", [None, False])
def test_node_without_the_parameter_publishes_none(costmap_on):
    _, radius, out, last = _node_run(costmap_on, True)
    assert radius == 0 and last["costmaps"] == 0 and all(o["costmaps"] == 0 for o in out)
    assert last["costmap"]["topic"] is None and last["costmap"]["count"] == 0 and last["costmap_update"]["count"] == 0
