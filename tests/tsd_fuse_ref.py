"""Numpy restatement of the TSD-level fusion rule (tsd_fuse_* in include/tsd_hip.h), written from the rule's text and independent of
the kernel: no tolerance is meant to be needed between the two with fp64 cells.  Works on ``tsd_download_tiles`` / ``O.Grid.dump()``
tuples ``(init[T] uint8, iw[T], tsd[T, 1089], w[T, 1089])`` in the canonical 33 x 33 tile layout (cell (ix, iy) at iy * 33 + ix,
ix == 32 / iy == 32 the halo), tiles row-major.

Contribution of a member cell: initialised tile -> (tsd, w) unless tsd is NaN; uninitialised tile with _initWeight > 0 -> (1, _initWeight);
else none.  Fused cell, contributors in member order: none -> (NaN, 0); one -> (t, min(w, 32)); several -> num = 0 + sum t w,
den = 0 + sum w (left to right), den > 0 -> (num / den, min(den, 32)), den == 0 -> (t of the first, 0)."""
import numpy as np

TILE, PITCH, CELLS = 32, 33, 1089
MAX_WEIGHT = 32.0


def _side(dump):
    px = int(round(np.sqrt(len(dump[0]))))
    assert px * px == len(dump[0])
    return px


def _interior(a, px):
    """[T, 1089] canonical tiles -> [32 px, 32 px] cells, row = y"""
    return a.reshape(px, px, PITCH, PITCH)[:, :, :TILE, :TILE].transpose(0, 2, 1, 3).reshape(px * TILE, px * TILE)


def _per_cell(tile_values, px):
    return np.repeat(np.repeat(tile_values.reshape(px, px), TILE, axis=0), TILE, axis=1)


def _place(src, ox, oy, n, fill):
    """src[y, x] into an n x n frame at cell (x + ox, y + oy), clipped"""
    out = np.full((n, n), fill, dtype=src.dtype)
    h, w = src.shape
    x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + w, n), min(oy + h, n)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = src[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return out


def member_cells(dump):
    """(contributes, t, w, initialised-tile index or -1) per cell of one member"""
    init, iw, tsd, w = dump
    px = _side(dump)
    ini = _per_cell(init.astype(bool), px)
    iwc = _per_cell(np.asarray(iw, dtype=np.float64), px)
    t, ww = _interior(tsd, px), _interior(w, px)
    empty = ~ini & (iwc > 0.0)
    c = (ini & ~np.isnan(t)) | empty
    t = np.where(empty, 1.0, np.where(c, t, 0.0))
    ww = np.where(empty, iwc, np.where(c, ww, 0.0))
    idx = np.where(ini, _per_cell(np.arange(px * px, dtype=np.int64), px), -1)
    return c, t, ww, idx


def fuse_cells(members, offsets, cells):
    """the fused cells of a ``cells`` x ``cells`` destination: (t, w, contributors) as [cells, cells] arrays, row = y"""
    n = cells
    cnt = np.zeros((n, n), dtype=np.int32)
    t0, num, den = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for dump, (ox, oy) in zip(members, offsets):
        c, t, w, _ = member_cells(dump)
        c, t, w = _place(c, ox, oy, n, False), _place(t, ox, oy, n, 0.0), _place(w, ox, oy, n, 0.0)
        t0 = np.where(c & (cnt == 0), t, t0)
        cnt = cnt + c
        num = np.where(c, num + t * w, num)
        den = np.where(c, den + w, den)
    ft, fw = np.full((n, n), np.nan), np.zeros((n, n))
    one, many = cnt == 1, cnt > 1
    ft[one] = t0[one]; fw[one] = np.minimum(den[one], MAX_WEIGHT)
    pos = many & (den > 0.0)
    ft[pos] = num[pos] / den[pos]; fw[pos] = np.minimum(den[pos], MAX_WEIGHT)
    zero = many & ~(den > 0.0)
    ft[zero] = t0[zero]; fw[zero] = 0.0
    return ft, fw, cnt


def _blocks(a, px):
    return a.reshape(px, TILE, px, TILE).transpose(0, 2, 1, 3).reshape(px * px, TILE * TILE)


def fuse_ref(members, offsets=None, cells=None):
    """the fused grid as a dump tuple and the counters of tsd_fuse_stats.  ``cells``: the destination's side (default: member 0's)"""
    offsets = [(0, 0)] * len(members) if offsets is None else [(int(a), int(b)) for a, b in offsets]
    n = _side(members[0]) * TILE if cells is None else int(cells)
    px = n // TILE
    T = px * px
    ft, fw, cnt = fuse_cells(members, offsets, n)
    # representation: materialised where a member's initialised tile intersects; its _initWeight from the first such member, lowest tile
    mat = np.zeros(T, dtype=bool)
    iw_out = np.zeros(T)
    big = np.iinfo(np.int64).max
    for dump, (ox, oy) in zip(members, offsets):
        idx = _place(member_cells(dump)[3], ox, oy, n, -1)
        lowest = _blocks(np.where(idx >= 0, idx, big), px).min(axis=1)
        hit = lowest < big
        first = hit & ~mat
        iw_out[first] = np.asarray(dump[1], dtype=np.float64)[lowest[first]]
        mat |= hit
    # elsewhere: unmaterialised when the 1024 cells are all equal, materialised with those cells when they are not
    bt, bw = _blocks(ft, px), _blocks(fw, px)
    known = ~np.isnan(bt)
    uniform = (known == known[:, :1]).all(axis=1) & ((bt == bt[:, :1]) | ~known).all(axis=1) & (bw.view(np.int64) == bw.view(np.int64)[:, :1]).all(axis=1)
    init = mat | ~uniform
    rest = ~mat & uniform
    iw_out[rest] = np.where(known[rest, 0], bw[rest, 0], 0.0)
    # canonical tiles with halos: the fused state of the duplicated cell, (NaN, 0) beyond the grid's edge
    pt, pw = np.full((n + 1, n + 1), np.nan), np.zeros((n + 1, n + 1))
    pt[:n, :n] = ft; pw[:n, :n] = fw
    tsd, w = np.full((T, CELLS), np.nan), np.zeros((T, CELLS))
    for p in np.nonzero(init)[0]:
        y0, x0 = (p // px) * TILE, (p % px) * TILE
        tsd[p] = pt[y0:y0 + PITCH, x0:x0 + PITCH].reshape(-1)
        w[p] = pw[y0:y0 + PITCH, x0:x0 + PITCH].reshape(-1)
    stats = dict(tiles_materialised=int(init.sum()), tiles_empty=int((~init & (iw_out > 0.0)).sum()), cells_valid=int((~np.isnan(ft)).sum()),
                 cells_one_source=int((cnt == 1).sum()), cells_many_sources=int((cnt > 1).sum()))
    return (init.astype(np.uint8), iw_out, tsd, w), stats


def assert_dumps_identical(got, want, what=""):
    """flags and _initWeight everywhere; tsd and weight of the materialised tiles, interiors and halos: NaNs position for position,
    every other value bit for bit"""
    gi, giw, gt, gw = got
    wi, wiw, wt, ww = want
    assert np.array_equal(gi, wi), f"{what}: tile flags differ at {np.nonzero(gi != wi)[0][:10]}"
    assert np.array_equal(np.asarray(giw).view(np.int64), np.asarray(wiw).view(np.int64)), \
        f"{what}: _initWeight differs at {np.nonzero(np.asarray(giw) != np.asarray(wiw))[0][:10]}"
    sel = wi.astype(bool)
    a, b = np.ascontiguousarray(gt[sel]), np.ascontiguousarray(wt[sel])
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs in {int((np.isnan(a) != np.isnan(b)).sum())} cells"
    m = ~np.isnan(a)
    bad = a[m].view(np.int64) != b[m].view(np.int64)
    assert not bad.any(), f"{what}: {int(bad.sum())} tsd values differ, max abs {np.abs(a[m] - b[m]).max()}"
    aw, bw = np.ascontiguousarray(gw[sel]), np.ascontiguousarray(ww[sel])
    bad = aw.view(np.int64) != bw.view(np.int64)
    assert not bad.any(), f"{what}: {int(bad.sum())} weights differ, max abs {np.abs(aw - bw).max()}"
