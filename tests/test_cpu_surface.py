"""The restatement of the surface list (tests/surface_ref.py) against the oracle, without a GPU.

The device list (tests/test_gpu_surface.py) is compared with the restatement bit for bit; here the restatement itself is pinned to the
reference's arithmetic through what the oracle already restates: the number of calcCoords' points, the cells ThreadGrid marks from them,
and interpolateBilinear at the positions the normals sample.  Hand-made tiles cover what a pushed grid does not reach on purpose: exact
zeros, NaNs, and the order of a tile's row and column events.
"""
import numpy as np
import pytest

from ohm_tsd_slam_amd import synth
from tests import helpers as H
from tests import surface_ref as S

LOG2, CS = 8, 0.1


@pytest.fixture(scope="module")
def room(oracle):
    """an oracle grid of 2^8 cells of 0.1 m after a dozen scans of the room, 360 beams: (grid, dump, the restatement's list)"""
    gc = synth.GridConfig(LOG2, CS)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for k in range(12):
        pose, (x, y, yaw) = H.sensor_pose(world, 3 * k)
        data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), H.MAX_RANGE, geo.angle_increment)
        og.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
    dump = og.dump()
    xy, where = S.points(LOG2, CS, dump[0], dump[2])
    return og, dump, xy, where


def test_count_equals_the_oracles(room):
    og, dump, xy, where = room
    N = 1 << LOG2
    _, n = og.occupancy(np.full(N * N, -1, dtype=np.int8))
    assert len(xy) == n and n > 200
    assert len(np.unique(where[:, 0])) > 4                       # several tiles contribute


def test_rounded_points_are_the_oracles_marks(room):
    og, dump, xy, where = room
    N = 1 << LOG2
    occ, _ = og.occupancy(np.full(N * N, -1, dtype=np.int8), inflate=False)
    occ = occ.reshape(N, N)
    mine = np.zeros((N, N), dtype=bool)
    for u, v in S.marks(LOG2, CS, xy):
        mine[v, u] = True
    assert mine.sum() > 100
    assert np.array_equal(mine, occ == 100)


def test_bilinear_equals_the_oracles_bit_for_bit(room):
    og, dump, xy, where = room
    sx, sy = S.normal_samples(CS, xy)
    # the normals' sample positions, and positions that fail: outside the grid, in tiles nobody has written
    xs = np.concatenate([sx.reshape(-1), [-0.01, 25.7, 1.0, 12.8]])
    ys = np.concatenate([sy.reshape(-1), [3.0, 3.0, 1.0, -5.0]])
    st, v = S.bilinear(LOG2, CS, dump[0], dump[2], xs, ys)
    seen = set()
    for i in range(len(xs)):
        o_st, o_v = og.bilinear(float(xs[i]), float(ys[i]))
        assert o_st == st[i], (i, xs[i], ys[i], o_st, st[i])
        if o_st == S.SUCCESS:
            assert np.float64(o_v).tobytes() == np.float64(v[i]).tobytes(), (i, o_v, v[i])
        seen.add(int(o_st))
    assert {S.SUCCESS, S.INVALIDINDEX, S.EMPTYPARTITION} <= seen
    nr, ok = S.normals(LOG2, CS, dump[0], dump[2], xy)
    assert ok.any()
    assert np.max(np.abs(np.hypot(nr[ok == 1, 0], nr[ok == 1, 1]) - 1.0)) < 1e-12      # unit normals where they exist
    assert np.all(nr[ok == 0] == 0.0)


def _tile(fill=np.nan):
    return np.full((S.PT, S.PT), fill)


def test_zeros_and_nans_make_no_event():
    t = _tile(1.0)
    t[3, 4:8] = [1.0, 0.0, -1.0, -1.0]           # + 0 - : the zero swallows the change (neither pair changes sign strictly)
    t[3, 8:] = -1.0
    t[4:, :] = np.nan                            # rows of NaN below
    t[0:3, :] = 1.0
    ev = S.tile_points(t.tolist(), 1, 1, 0.1)
    # row 3: 1 -> 0 and 0 -> -1 are no events; columns: 1 -> -1 between rows 2 and 3 for px >= 6 only (px == 5: 1 -> 0), nothing into NaN
    assert [c for c, _, _ in ev] == [S.scan_index(3, px, True) for px in range(6, S.D + 1)]
    t = _tile(np.nan)
    t[5, 5], t[5, 7] = 1.0, -1.0                 # NaN between a + and a -
    assert S.tile_points(t.tolist(), 1, 1, 0.1) == []
    t = _tile(0.0)
    t[::2, :] = -0.0
    assert S.tile_points(t.tolist(), 1, 1, 0.1) == []


def test_order_of_a_tile_with_row_and_column_events():
    t = _tile(1.0)
    t[10:20, 12:18] = -0.5                       # a box of negative cells: row events on its left / right, column events on top / bottom
    cs, X, Y = 0.1, 2, 3
    ev = S.tile_points(t.tolist(), X, Y, cs)
    cc = [c for c, _, _ in ev]
    assert cc == sorted(cc) and len(set(cc)) == len(cc)                      # ascending c is the serial order
    rows = [c for c in cc if c < S.ROW_POSITIONS]
    cols = [c for c in cc if c >= S.ROW_POSITIONS]
    assert len(rows) == 2 * 10 and len(cols) == 2 * 6 and cc == rows + cols   # all row events first
    assert rows[:2] == [S.scan_index(10, 12, False), S.scan_index(10, 18, False)]
    assert cols[:2] == [S.scan_index(10, 12, True), S.scan_index(20, 12, True)]
    # the first row event: between px = 11 (+1) and px = 12 (-0.5): interp = 1 / 1.5
    interp = 1.0 / (1.0 - -0.5)
    assert ev[0][1] == 12 * cs + cs * (interp - 1.0) + (X * 32) * cs and ev[0][2] == 10 * cs + (Y * 32) * cs
    c0 = [e for e in ev if e[0] == S.scan_index(10, 12, True)][0]
    assert c0[1] == 12 * cs + (X * 32) * cs and c0[2] == 10 * cs + cs * (interp - 1.0) + (Y * 32) * cs


def test_window_is_a_sublist():
    rng = np.random.default_rng(3)
    PX = (1 << LOG2) // 32
    init = np.ones(PX * PX, dtype=np.uint8)
    tsd = rng.choice([-0.2, 0.3], size=(PX * PX, S.PT * S.PT))
    full, where = S.points(LOG2, CS, init, tsd)
    assert set(np.unique(where[:, 0])) == {y * PX + x for y in range(1, PX - 1) for x in range(1, PX - 1)}   # never the outer ring
    sub, wsub = S.points(LOG2, CS, init, tsd, window=(0, 2, 3, 9))           # reaches into the ring on two sides: clipped
    keep = np.isin(where[:, 0], [y * PX + x for y in range(2, PX - 1) for x in range(1, 3)])
    assert keep.any() and np.array_equal(sub, full[keep]) and np.array_equal(wsub, where[keep])
    assert len(S.points(LOG2, CS, init, tsd, window=(3, 3, 3, 5))[0]) == 0
