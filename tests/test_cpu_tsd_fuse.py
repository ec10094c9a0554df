"""The TSD-level fusion rule without a device: properties of its numpy restatement (tests/tsd_fuse_ref.py) on grids the oracle
built, and the refusals tsd_fuse_begin makes before its first HIP call."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from oracle import pyoracle as O
from tests import helpers as H
from tests import nranks_common as NC
from tests import tsd_fuse_ref as F


def _scan(world, geo, robot, k):
    pose, (x, y, yaw) = NC.robot_pose(world, robot, k)
    data, mask = O.ingest_f32(np.ascontiguousarray(world.scan(x, y, yaw, geo), dtype=np.float32), H.MAX_RANGE, geo.angle_increment)
    return pose, data, mask


def _push(grid, geo, scan):
    pose, data, mask = scan
    grid.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)


def _grid(gc):
    return O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)


@pytest.fixture(scope="module")
def room():
    O.build()
    gc, geo, world = NC.setup()
    return gc, geo, world, [_scan(world, geo, 0, k) for k in range(20)]


def _built(gc, geo, scans):
    g = _grid(gc)
    for s in scans:
        _push(g, geo, s)
    d = g.dump()
    g.close()
    return d


@pytest.mark.parametrize("n", [5, 10])
def test_split_scans_fuse_to_the_grid_that_saw_them_all(room, n):
    """Alternate scans go to A and B, all of them to C.  fuse(A, B) has C's tiles and C's known cells; tsd and weight agree within
    1e-12: at most 20 running-mean steps on values of magnitude <= 1, a few ulp each, is about 1e-14 (the total weight stays <= 20
    here, so the cap of 32 never enters).  Measured: max abs tsd diff 4.4e-16 (5 + 5) and 6.7e-16 (10 + 10), weight 3.6e-15."""
    gc, geo, world, scans = room
    A, B, Cd = _built(gc, geo, scans[0:2 * n:2]), _built(gc, geo, scans[1:2 * n:2]), _built(gc, geo, scans[:2 * n])
    (fi, fiw, ft, fw), _ = F.fuse_ref([A, B])
    assert np.array_equal(fi, Cd[0]), "tile coverage differs"
    unin = ~Cd[0].astype(bool)
    print("max abs _initWeight diff", np.abs(fiw[unin] - Cd[1][unin]).max())
    assert np.abs(fiw[unin] - Cd[1][unin]).max() <= 1e-12
    px = F._side(Cd)
    sel = Cd[0].astype(bool)
    a, b = F._interior(ft, px), F._interior(Cd[2], px)
    aw, bw = F._interior(fw, px), F._interior(Cd[3], px)
    cell = F._per_cell(sel, px)
    assert np.array_equal(np.isnan(a[cell]), np.isnan(b[cell])), "NaN pattern differs"
    m = cell & ~np.isnan(b)
    assert m.sum() > 10000
    dt, dw = np.abs(a[m] - b[m]).max(), np.abs(aw[cell] - bw[cell]).max()
    print(f"{n} + {n} scans: max abs diff tsd {dt:.3g} weight {dw:.3g}")
    assert dt <= 1e-12 and dw <= 1e-12


def test_one_grid_at_offset_zero_fuses_to_itself(room):
    gc, geo, world, scans = room
    A = _built(gc, geo, scans[:8])
    assert (~A[0].astype(bool) & (A[1] > 0)).any() and A[0].any(), "the grid must hold data tiles and empty tiles"
    (fi, fiw, ft, fw), st = F.fuse_ref([A])
    px = F._side(A)
    assert np.array_equal(fi, A[0]) and fiw.tobytes() == A[1].tobytes()
    sel = A[0].astype(bool)
    for got, want in ((ft, A[2]), (fw, A[3])):
        g = got.reshape(-1, 33, 33)[sel][:, :32, :32]
        w = want.reshape(-1, 33, 33)[sel][:, :32, :32]
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes()     # NaNs included: one NaN pattern on both sides
    assert st["cells_many_sources"] == 0 and st["tiles_materialised"] == int(sel.sum())


def test_member_order_moves_nothing_but_the_rounding_of_the_sums(room):
    """The set of known cells does not depend on the order.  With two members num and den are sums of two terms, which IEEE addition
    gives in either order alike, so a swap changes tsd by at most 1 ulp (in fact by nothing); with three members the sums are
    rounded in another order -- a difference of the SUM's rounding, not of the rule."""
    gc, geo, world, scans = room
    A, B, Cc = _built(gc, geo, scans[0:4]), _built(gc, geo, scans[4:9]), _built(gc, geo, scans[9:12])
    (t1, w1, c1), (t2, w2, c2) = F.fuse_cells([A, B], [(0, 0), (3, -2)], 512), F.fuse_cells([B, A], [(3, -2), (0, 0)], 512)
    assert np.array_equal(np.isnan(t1), np.isnan(t2)) and np.array_equal(c1, c2) and (c1 > 1).sum() > 10000
    m = ~np.isnan(t1)
    assert (np.abs(t1[m] - t2[m]) <= np.spacing(np.abs(t1[m]))).all()
    t3 = [F.fuse_cells([(A, B, Cc)[i] for i in p], [(0, 0)] * 3, 512)[0] for p in ((0, 1, 2), (2, 0, 1), (1, 2, 0))]
    assert all(np.array_equal(np.isnan(t3[0]), np.isnan(t)) for t in t3[1:])
    m = ~np.isnan(t3[0])
    assert max(np.abs(t3[0][m] - t[m]).max() for t in t3[1:]) <= 1e-14


@pytest.mark.parametrize("off", [(1, 0), (17, -5), (32, 64)])
def test_a_shifted_member_alone_is_the_member_shifted(room, off):
    gc, geo, world, scans = room
    A = _built(gc, geo, scans[:6])
    ox, oy = off
    (fi, fiw, ft, fw), st = F.fuse_ref([A], [off])
    c, t, w, _ = F.member_cells(A)
    px = F._side(A)
    n = px * 32
    # the fused cells, whatever the tile's representation
    tiles_t = np.where(F._per_cell(fi.astype(bool), px), F._interior(ft, px), np.where(F._per_cell(fiw, px) > 0, 1.0, np.nan))
    tiles_w = np.where(F._per_cell(fi.astype(bool), px), F._interior(fw, px), F._per_cell(fiw, px))
    want_t = F._place(np.where(c, t, np.nan), ox, oy, n, np.nan)
    want_w = F._place(w, ox, oy, n, 0.0)
    assert np.array_equal(np.isnan(tiles_t), np.isnan(want_t))
    m = ~np.isnan(want_t)
    assert np.array_equal(tiles_t[m], want_t[m]) and np.array_equal(tiles_w[m], want_w[m])
    data = F._blocks(F._place(F._per_cell(A[0].astype(bool), px), ox, oy, n, False), px).any(axis=1)
    assert (fi.astype(bool) & data).sum() == data.sum() > 0
    if ox % 32 == 0 and oy % 32 == 0:
        assert np.array_equal(fi.astype(bool), data)       # whole tiles move onto whole tiles: empty tiles stay unmaterialised
    # halos: the fused state of the duplicated cell
    p = int(np.nonzero(fi)[0][len(np.nonzero(fi)[0]) // 2])
    y0, x0 = (p // px) * 32, (p % px) * 32
    halo = ft[p].reshape(33, 33)
    for iy in range(32):
        v = tiles_t[y0 + iy, x0 + 32] if x0 + 32 < n else np.nan
        assert (np.isnan(v) and np.isnan(halo[iy, 32])) or v == halo[iy, 32]


@pytest.mark.parametrize("off", [(1, 0), (17, -5), (32, 64), (0, 0)])
def test_empty_tiles_of_a_misaligned_member_are_materialised(off):
    """no initialised tile anywhere: two neighbouring empty tiles of different _initWeight.  Shifted by whole tiles they stay
    unmaterialised; shifted by less, the destination tiles they cover in part hold cells that differ and are materialised"""
    px = 8
    init, iw = np.zeros(px * px, np.uint8), np.zeros(px * px)
    iw[2 * px + 2], iw[2 * px + 3] = 3.0, 5.0
    A = (init, iw, np.full((px * px, 1089), np.nan), np.zeros((px * px, 1089)))
    ox, oy = off
    (fi, fiw, ft, fw), st = F.fuse_ref([A], [off])
    if ox % 32 == 0 and oy % 32 == 0:
        assert not fi.any() and st["tiles_empty"] == 2 and st["tiles_materialised"] == 0
        p = (2 + oy // 32) * px + 2 + ox // 32
        assert fiw[p] == 3.0 and fiw[p + 1] == 5.0 and fiw.sum() == 8.0
    else:
        assert fi.sum() == (3 if oy % 32 == 0 else 6) and st["tiles_empty"] == 0 and fiw.sum() == 0.0
        t, w = F._interior(ft, px), F._interior(fw, px)
        y, x = 2 * 32 + oy, 2 * 32 + ox
        assert (t[y:y + 32, x:x + 64] == 1.0).all() and (w[y:y + 32, x:x + 32] == 3.0).all() and (w[y:y + 32, x + 32:x + 64] == 5.0).all()
        assert np.isnan(t).sum() == t.size - 2048 and st["cells_valid"] == st["cells_one_source"] == 2048
        # a halo cell holds the fused state of the cell it duplicates, whatever that neighbour's representation
        p = (2 + oy // 32) * px + 2 + ox // 32
        tile = ft[p].reshape(33, 33)
        assert np.array_equal(np.isnan(tile[:32, 32]), np.isnan(t[(p // px) * 32:(p // px) * 32 + 32, (p % px) * 32 + 32]))
        assert np.array_equal(np.isnan(tile[32, :33]), np.isnan(t[(p // px) * 32 + 32, (p % px) * 32:(p % px) * 32 + 33]))


def test_freed_cells_with_weight_zero_take_the_first_contributor(room):
    gc, geo, world, scans = room
    ga, gb = _grid(gc), _grid(gc)
    c = [world.cx, world.cy]
    assert ga.free_footprint(c, 1.0, 1.0) and gb.free_footprint(c, 1.0, 1.0)
    _push(gb, geo, scans[0])        # B's freed cells now carry weight; A's stay at weight 0
    A, B = ga.dump(), gb.dump()
    gc2 = _grid(gc)
    assert gc2.free_footprint([world.cx + 0.2, world.cy], 1.0, 1.0)
    A2 = gc2.dump()
    for g in (ga, gb, gc2):
        g.close()
    ca, ta, wa, _ = F.member_cells(A)
    freed = ca & (wa == 0.0)
    assert freed.sum() >= 300
    t, w, cnt = F.fuse_cells([A, A2], [(0, 0), (0, 0)], 512)
    c2, t2, w2, _ = F.member_cells(A2)
    both = freed & c2 & (w2 == 0.0)
    assert both.sum() > 100
    assert np.array_equal(t[both], ta[both]) and (w[both] == 0.0).all() and (cnt[both] == 2).all()
    # against a member with weight the freed cell of A counts for nothing: num = t_a * 0 + t_b * w_b
    t, w, cnt = F.fuse_cells([A, B], [(0, 0), (0, 0)], 512)
    cb, tb, wb, _ = F.member_cells(B)
    m = freed & cb & (wb > 0.0)
    assert m.sum() > 100
    assert np.abs(t[m] - tb[m]).max() <= 1e-15 and np.array_equal(w[m], wb[m])


def test_fuse_refuses_bad_arguments_without_a_device(hip_lib):
    """the checks that need no context fields beyond the handles come first: a NULL destination, the count, NULL members"""
    lib = hip_lib
    dummy = (C.c_void_p * 65)(*([1] * 65))
    assert lib.tsd_fuse_begin(None, 1, dummy, None) == -1
    assert lib.tsd_fuse(None, 1, dummy, None, None) == -1
    assert lib.tsd_fuse_wait(None, None) == -1
    assert lib.tsd_abi_sizeof(b"tsd_fuse_stats") == C.sizeof(capi.FuseStats) == 40
