"""The surface list of the device (tsd_surface_extract / _fetch / _dev) against the restatement of tests/surface_ref.py run
on the tiles downloaded from the same context.

n, the order, xy and normal_ok are compared BIT FOR BIT (the coordinates use only IEEE +, -, x, / in a fixed order); the normals where
ok is set at the ray cast's coordinate bar, 1e-9 (README "Correctness bar").  tests/test_cpu_surface.py pins the restatement to the
oracle.
"""
import functools

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import helpers as H
from tests import surface_ref as S

pytestmark = pytest.mark.gpu

NORMAL_BAR = 1e-9
PT2 = S.PT * S.PT


def _compare(dg, log2, cs, window=None, normals=True, tiles=None):
    """one extraction on the device and the restatement on its tiles -> the device's (xy, normals, ok), the restatement's `where`"""
    tiles = dg.download_tiles() if tiles is None else tiles
    r_xy, where = S.points(log2, cs, tiles[0], tiles[2], window)
    xy, nr, ok = dg.surface_points(window, normals)
    assert xy.shape == r_xy.shape, f"window {window}: n = {len(xy)}, the restatement's {len(r_xy)}"
    assert xy.tobytes() == r_xy.tobytes(), f"window {window}: {np.count_nonzero(xy != r_xy)} coordinates differ (or the order)"
    if not normals:
        assert nr is None and ok is None
        return xy, nr, ok, where
    r_nr, r_ok = S.normals(log2, cs, tiles[0], tiles[2], r_xy)
    assert np.array_equal(ok, r_ok), f"window {window}: normal_ok differs at {np.nonzero(ok != r_ok)[0][:10]}"
    assert np.all(nr[ok == 0] == 0.0)
    worst = float(np.max(np.abs(nr[ok == 1] - r_nr[ok == 1]))) if ok.any() else 0.0
    print(f"surface: n = {len(xy)}, ok = {int(ok.sum())}, max |normal - restatement| = {worst:.3g}")
    assert worst <= NORMAL_BAR
    return xy, nr, ok, where


def _pushed(oracle, log2, cs, geo, scene, scans, storage="f64"):
    gc = synth.GridConfig(log2, cs)
    world = synth.World(scene, gc)
    dg = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc, storage=storage)
    for k in range(scans):
        pose, (x, y, yaw) = H.sensor_pose(world, 3 * k)
        data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), H.MAX_RANGE, geo.angle_increment)
        dg.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL, want_stats=False)
    return dg


@pytest.mark.parametrize("log2,cs,geo,scene,storage", [
    (8, 0.1, synth.ScanGeometry.full_circle_360(), "room", "f64"),
    (9, 0.05, synth.ScanGeometry.utm30lx(), "pillars", "f64"),
    (8, 0.1, synth.ScanGeometry.full_circle_360(), "room", "q32"),
])
def test_pushed_grid(oracle, log2, cs, geo, scene, storage):
    dg = _pushed(oracle, log2, cs, geo, scene, 8, storage)
    xy, nr, ok, where = _compare(dg, log2, cs)
    _, n_surface = dg.occupancy()
    assert len(xy) == n_surface and len(xy) > 200
    assert ok.sum() > len(xy) // 2                               # a pushed surface has its normals
    assert len(np.unique(where[:, 0])) > 4


# ---- uploaded tiles ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_tiles(log2, seed, dense, p_uninit=1.0 / 3.0):
    """(init, iw, tsd, w): a third (p_uninit) of the tiles uninitialised, some of those "empty" (initWeight > 0).  dense: every cell drawn from
    {+u, -u, 0, NaN}; otherwise a tile is +u with a random number (0 .. 40) of such cells, so the tiles' counts differ widely."""
    rng = np.random.default_rng(seed)
    PX = (1 << log2) // 32
    T = PX * PX
    init = (rng.random(T) >= p_uninit).astype(np.uint8)
    init[[1 * PX + 1, (PX - 2) * PX + (PX - 2)]] = 1             # the first and the last processed tile hold data
    iw = np.where((init == 0) & (rng.random(T) < 0.4), 0.5, 0.0)
    u = rng.uniform(0.05, 1.0, size=(T, PT2))
    kind = rng.choice(4, size=(T, PT2), p=[0.42, 0.42, 0.08, 0.08])
    drawn = np.select([kind == 0, kind == 1, kind == 2], [u, -u, 0.0], np.nan)
    if dense:
        tsd = drawn
    else:
        few = rng.random((T, PT2)) < (rng.integers(0, 41, size=(T, 1)) / PT2)
        tsd = np.where(few, drawn, u)
    tsd[init == 0] = np.nan
    w = np.where(np.isnan(tsd), 0.0, 1.0)
    return init, iw, tsd, w


def _uploaded(log2, cs, tiles):
    dg = capi.TsdGridDevice(log2, cs, 3 * cs)
    dg.upload_tiles(*tiles)
    return dg


def test_random_tiles_seams_halos_failing_normals():
    log2, cs = 8, 0.1
    tiles = _random_tiles(log2, 11, True)
    dg = _uploaded(log2, cs, tiles)
    got = dg.download_tiles()
    assert np.array_equal(got[0], tiles[0]) and np.array_equal(got[2][tiles[0] == 1], tiles[2][tiles[0] == 1], equal_nan=True)
    xy, nr, ok, where = _compare(dg, log2, cs, tiles=got)
    PX = (1 << log2) // 32
    p, c = where[:, 0], where[:, 1]
    assert set(np.unique(p)) <= {y * PX + x for y in range(1, PX - 1) for x in range(1, PX - 1)}      # none in the outer ring
    assert PX + 1 in p and (PX - 2) * PX + PX - 2 in p                                                # first and last processed tile
    halo_row = (c < S.ROW_POSITIONS) & (c // 32 == 32)
    halo_col = (c >= S.ROW_POSITIONS) & ((c - S.ROW_POSITIONS) // 32 == 32)
    assert halo_row.any() and halo_col.any()                                                          # events in the halo row / column
    assert (ok == 1).any() and (ok == 0).any()                                                        # normals that exist and that fail
    # a seam found by two tiles whose copies of it differ: the halo row of tile p against row 0 of the tile above it
    differ = 0
    for q in np.unique(p[halo_row]):
        up = q + PX
        if up in p:
            a = xy[(p == q) & halo_row]
            b = xy[(p == up) & (c < 32)]
            differ += len(a) != len(b) or not np.array_equal(a, b)
    assert differ > 0


def test_checkerboard_and_single_event_tiles():
    log2, cs = 8, 0.1
    PX = (1 << log2) // 32
    T = PX * PX
    init, iw = np.zeros(T, dtype=np.uint8), np.zeros(T)
    tsd = np.full((T, PT2), np.nan)
    board, single = 3 * PX + 3, 3 * PX + 4
    yy, xx = np.mgrid[0:S.PT, 0:S.PT]
    tsd[board] = np.where((xx + yy) % 2 == 0, 0.25, -0.75).reshape(-1)
    one = np.full((S.PT, S.PT), np.nan)
    one[5, 5], one[5, 6] = 1.0, -1.0
    tsd[single] = one.reshape(-1)
    init[[board, single]] = 1
    dg = _uploaded(log2, cs, (init, iw, tsd, np.where(np.isnan(tsd), 0.0, 1.0)))
    xy, nr, ok, where = _compare(dg, log2, cs)
    assert np.array_equal(where[:, 0], [board] * 2 * S.ROW_POSITIONS + [single])       # all 2 112 positions, then the one event
    assert np.array_equal(where[:-1, 1], np.arange(2 * S.ROW_POSITIONS))
    assert where[-1, 1] == S.scan_index(5, 6, False)


def test_more_tiles_than_lanes():
    log2, cs = 10, 0.05
    tiles = _random_tiles(log2, 12, False)
    dg = _uploaded(log2, cs, tiles)
    xy, nr, ok, where = _compare(dg, log2, cs, tiles=dg.download_tiles())
    counts = np.bincount(where[:, 0], minlength=len(tiles[0]))
    assert (counts > 0).sum() > 256 and len(xy) > 2000
    PX = (1 << log2) // 32
    ty, tx = np.divmod(np.arange(PX * PX), PX)
    ring = (tx >= 1) & (tx <= PX - 2) & (ty >= 1) & (ty <= PX - 2)
    assert (counts[ring & (tiles[0] == 1)] == 0).any()           # processed, initialised tiles without an event among them
    assert (counts[~ring] == 0).all()


def test_more_tiles_than_one_scan_workgroup():
    """62 x 62 = 3 844 window tiles: the scan takes four workgroups of 1 024 tiles and the pass over their totals"""
    log2, cs = 11, 0.05
    tiles = _random_tiles.__wrapped__(log2, 13, False, 0.85)     # (not kept: 35 MB per array)
    dg = _uploaded(log2, cs, tiles)
    xy, nr, ok, where = _compare(dg, log2, cs, tiles=tiles)
    PX = (1 << log2) // 32
    w = (where[:, 0] // PX - 1) * (PX - 2) + where[:, 0] % PX - 1          # the tiles' numbers in the window
    assert set(np.unique(w // 1024)) == {0, 1, 2, 3} and len(xy) > 2000
    # a window of 1 025 tiles: the smallest that needs the second level
    _compare(dg, log2, cs, (1, 1, 42, 26), tiles=tiles)
    _compare(dg, log2, cs, (1, 1, 33, 33), tiles=tiles)                    # ... and exactly 1 024: the largest that does not


def test_uninitialised_grid_is_empty():
    dg = capi.TsdGridDevice(8, 0.1, 0.3)
    assert dg.surface_extract() == 0
    xy, nr, ok = dg.surface_points()
    assert xy.shape == (0, 2) and nr.shape == (0, 2) and ok.shape == (0,)
    assert dg.surface_dev()[3] == 0
    small = capi.TsdGridDevice(5, 0.1, 0.3)                      # one tile: no processed ring at all
    assert small.surface_extract() == 0


@pytest.mark.parametrize("window", [(3, 3, 4, 4), (1, 2, 4, 5), (0, 0, 3, 2), (4, 4, 8, 8), (3, 3, 3, 6), (0, 0, 1, 8), (5, 5, 2, 2)],
                         ids=["one_tile", "rectangle", "into_the_ring_low", "into_the_ring_high", "empty", "all_clipped", "inverted"])
def test_windows(window):
    log2, cs = 8, 0.1
    tiles = _random_tiles(log2, 11, True)
    dg = _uploaded(log2, cs, tiles)
    xy, nr, ok, where = _compare(dg, log2, cs, window, tiles=tiles)
    PX = (1 << log2) // 32
    tx0, ty0, tx1, ty1 = S.clip_window(PX, window)
    holds_data = bool(tiles[0].reshape(PX, PX)[ty0:max(ty1, ty0), tx0:max(tx1, tx0)].any())
    assert holds_data == (window in [(3, 3, 4, 4), (1, 2, 4, 5), (0, 0, 3, 2), (4, 4, 8, 8)])      # what the case is named after
    assert (len(xy) > 0) == holds_data                            # (a tile of dense random cells always has events)
    # the sublist of the whole list that the window's tiles contribute
    full, _, _, fwhere = _compare(dg, log2, cs, None, tiles=tiles)
    fx, fy = fwhere[:, 0] % PX, fwhere[:, 0] // PX
    keep = (fx >= tx0) & (fx < tx1) & (fy >= ty0) & (fy < ty1)
    assert np.array_equal(xy, full[keep])


def test_without_normals_fetch_ranges_growth_and_reuse():
    log2, cs = 8, 0.1
    tiles = _random_tiles(log2, 11, True)
    dg = _uploaded(log2, cs, tiles)
    # a small list first, then a larger one (the buffers grow), then a smaller one (they are reused)
    small = _compare(dg, log2, cs, (2, 2, 3, 3), tiles=tiles)[0]
    a_small = dg.surface_dev()
    full_xy, full_nr, full_ok, _ = _compare(dg, log2, cs, None, tiles=tiles)
    a_full = dg.surface_dev()
    assert a_full[3] == len(full_xy) > 4 * len(small) > 0 and a_small[3] == len(small)
    assert all(a_full[:3])
    again = _compare(dg, log2, cs, (2, 2, 3, 3), tiles=tiles)[0]
    assert np.array_equal(again, small)
    assert dg.surface_dev()[:3] == a_full[:3], "a smaller list after a larger one allocated again"
    # fetch in pieces
    n = dg.surface_extract()
    assert n == len(full_xy)
    cut = n // 3
    parts = [dg.surface_fetch(0, cut), dg.surface_fetch(cut, n - cut)]
    assert np.array_equal(np.concatenate([q[0] for q in parts]), full_xy)
    assert np.array_equal(np.concatenate([q[1] for q in parts]), full_nr)
    assert np.array_equal(np.concatenate([q[2] for q in parts]), full_ok)
    assert dg.surface_fetch(n, 0)[0].shape == (0, 2) and dg.surface_fetch(5, 0)[0].shape == (0, 2)
    for first, count in ((0, n + 1), (n, 1), (-1, 2), (3, -1), (n - 1, 2)):
        with pytest.raises(capi.TsdError):
            dg.surface_fetch(first, count)
    # without normals: the same points; their fetch is refused
    xy0 = _compare(dg, log2, cs, None, normals=False, tiles=tiles)[0]
    assert np.array_equal(xy0, full_xy)
    dev = dg.surface_dev()
    assert dev[0] and dev[1] == 0 and dev[2] == 0 and dev[3] == n
    with pytest.raises(capi.TsdError):
        dg.surface_fetch(0, 1, normals=True)
    assert np.array_equal(dg.surface_fetch(2, 5, normals=False)[0], full_xy[2:7])


def test_read_only(oracle):
    log2, cs, geo = 8, 0.1, synth.ScanGeometry.full_circle_360()
    a = _pushed(oracle, log2, cs, geo, "room", 4)
    b = _pushed(oracle, log2, cs, geo, "room", 4)
    first_a, first_b = a.map_update(True, 2), b.map_update(True, 2)
    assert np.array_equal(first_a[1], first_b[1])
    world = synth.World("room", synth.GridConfig(log2, cs))
    pose, (x, y, yaw) = H.sensor_pose(world, 20)
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), 4.0, geo.angle_increment)
    for g in (a, b):
        g.push(pose, data, mask, geo.angle_increment, geo.angle_min, 4.0, H.MIN_RANGE, H.LOW_REFL, want_stats=False)
    before = a.digest()
    assert a.surface_extract() > 0 and a.surface_extract((2, 2, 4, 4), normals=False) >= 0
    assert a.digest() == before == b.digest()
    # the windowed frame behind an extraction: the window, bytes and count of a twin context that made none
    ua, ub = a.map_update(True, 2), b.map_update(True, 2)
    assert ua[0] == ub[0] and ua[0][2] > 0
    assert np.array_equal(ua[1], ub[1]) and np.array_equal(ua[2], ub[2]) and ua[3] == ub[3]
    assert a.occupancy()[1] == b.occupancy()[1] == a.surface_extract()


# ---- facade --------------------------------------------------------------------------------------------------------------------
def _node_run(surface_on):
    gc, geo, scene = synth.GridConfig(8, 0.1), synth.ScanGeometry.full_circle_360(), "room"
    world = synth.World(scene, gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over = dict(occ_grid_time_interval=1000.0)
    if surface_on is not None:
        over["publish_surface_cloud"] = surface_on
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m, cloud = node.map_msg(), node.surface_msg()
        xy, nr, ok = node.grid().surface_points()
    finally:
        node.close()
    return m, cloud, (xy, nr, ok)


def test_node_publishes_the_surface_cloud():
    m, cloud, (xy, nr, ok) = _node_run(True)
    assert cloud["count"] == 1 and cloud["width"] == len(xy) > 100 and cloud["point_step"] == 24
    assert cloud["fields"] == ["x", "y", "z", "normal_x", "normal_y", "normal_z"]
    assert cloud["frame_id"] == m["frame_id"] and cloud["stamp_ns"] == m["stamp_ns"]
    ox, oy = m["origin_position"][0], m["origin_position"][1]
    want = np.zeros((len(xy), 6), dtype=np.float32)
    want[:, 0], want[:, 1] = (xy[:, 0] + ox).astype(np.float32), (xy[:, 1] + oy).astype(np.float32)
    want[:, 3], want[:, 4] = np.where(ok == 1, nr[:, 0], 0.0).astype(np.float32), np.where(ok == 1, nr[:, 1], 0.0).astype(np.float32)
    assert cloud["points"].tobytes() == want.tobytes()
    assert ok.any()
    # the parameter off, and absent: no message, and the map as it is today
    for run in (_node_run(False), _node_run(None)):
        m2, cloud2, _ = run
        assert cloud2["count"] == 0 and cloud2["width"] == 0
        assert m2["data"].tobytes() == m["data"].tobytes()
        for k in ("resolution", "width", "height", "frame_id", "count"):
            assert m2[k] == m[k]
        assert np.array_equal(m2["origin_position"], m["origin_position"])
