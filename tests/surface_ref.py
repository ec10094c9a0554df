"""Plain Python / numpy restatement of the surface list (tsd_surface_extract in include/tsd_hip.h), written for
tests/test_cpu_surface.py and tests/test_gpu_surface.py.

  * the points: the loops of RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105), literally and in their serial order,
    over the canonical tile dump (flags, 33 x 33 row-major tsd per tile) that `download_tiles()` / the oracle's `dump()` hand out;
  * the normals: TsdGrid::interpolateNormal (TsdGrid.cpp:517-546) AT EACH POINT -- not at the array's first point, which is what the
    reference's call computes -- from a numpy bilinear look-up in the operation order of TsdGrid.h:284-340 (coord2Cell,
    interpolateBilinear) and norm2 (mathbase.h:211-218).

Nothing here calls into oracle/ or the device library.  Python floats and numpy float64 are IEEE doubles without contraction, so the
expressions below give the reference's bits.
"""
from __future__ import annotations

import math

import numpy as np

D = 32             # cells per tile side
PT = 33            # pitch of the canonical dump: the tile plus its one-cell halo
ROW_POSITIONS = PT * D          # 1 056 row-scan positions of a tile, then as many column-scan positions
SUCCESS, INVALIDINDEX, EMPTYPARTITION, ISNAN = 0, 1, 2, 3


def scan_index(py: int, px: int, col: bool) -> int:
    """c of a scan position: ascending c is the reference's order inside a tile"""
    return ROW_POSITIONS + px * D + (py - 1) if col else py * D + (px - 1)


def tile_points(t, x: int, y: int, cs: float):
    """the events of one initialised tile (x, y): t is its 33 x 33 tsd as nested lists.  -> [(c, px_coord, py_coord)]"""
    out = []
    for py in range(D + 1):                              # :38-60
        prev = t[py][0]
        for px in range(1, D + 1):
            v = t[py][px]
            if (prev > 0 and v < 0) or (prev < 0 and v > 0):
                interp = prev / (prev - v)
                out.append((scan_index(py, px, False), px * cs + cs * (interp - 1.0) + (x * D) * cs, py * cs + (y * D) * cs))
            prev = v
    for px in range(D + 1):                              # :62-80
        prev = t[0][px]
        for py in range(1, D + 1):
            v = t[py][px]
            if (prev > 0 and v < 0) or (prev < 0 and v > 0):
                interp = prev / (prev - v)
                out.append((scan_index(py, px, True), px * cs + (x * D) * cs, py * cs + cs * (interp - 1.0) + (y * D) * cs))
            prev = v
    return out


def clip_window(PX: int, window):
    """[tx0, tx1) x [ty0, ty1) clipped to the processed ring 1 .. PX-2; None: the ring"""
    tx0, ty0, tx1, ty1 = window if window is not None else (1, 1, PX - 1, PX - 1)
    return max(tx0, 1), max(ty0, 1), min(tx1, PX - 1), min(ty1, PX - 1)


def points(map_size_log2: int, cs: float, init, tsd, window=None):
    """-> (xy [n, 2] float64, where [n, 2] int: (tile, c) of every point), in the reference's order; `window` keeps the tiles of the
    rectangle only (the order among them is unchanged)"""
    PX = (1 << map_size_log2) // D
    cs = float(cs)
    tx0, ty0, tx1, ty1 = clip_window(PX, window)
    xy, where = [], []
    for y in range(1, PX - 1):                           # :25-27 (no round at all for PX < 3)
        for x in range(1, PX - 1):
            p = y * PX + x
            if not init[p] or not (tx0 <= x < tx1 and ty0 <= y < ty1):
                continue                                 # (an initialised partition is never isEmpty(), TsdGridPartition.h:72)
            t = np.asarray(tsd[p], dtype=np.float64).reshape(PT, PT).tolist()
            for c, px_, py_ in tile_points(t, x, y, cs):
                xy.append((px_, py_))
                where.append((p, c))
    return np.array(xy, dtype=np.float64).reshape(-1, 2), np.array(where, dtype=np.int64).reshape(-1, 2)


def bilinear(map_size_log2: int, cs: float, init, tsd, xs, ys):
    """TsdGrid::interpolateBilinear at (xs[i], ys[i]) -> (status [n], value [n]; NaN where the status is not SUCCESS or ISNAN)"""
    N = 1 << map_size_log2
    PX = N // D
    cs = float(cs)
    inv = 1.0 / cs
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    tsd = np.asarray(tsd, dtype=np.float64).reshape(-1, PT * PT)
    init = np.asarray(init)
    with np.errstate(invalid="ignore"):
        # coord2Cell (TsdGrid.h:306-340)
        xi, yi = np.floor(xs * inv).astype(np.int64), np.floor(ys * inv).astype(np.int64)
        dx, dy = (xi.astype(np.float64) + 0.5) * cs, (yi.astype(np.float64) + 0.5) * cs
        lo_x, lo_y = xs < dx, ys < dy
        xi, dx = np.where(lo_x, xi - 1, xi), np.where(lo_x, dx - cs, dx)
        yi, dy = np.where(lo_y, yi - 1, yi), np.where(lo_y, dy - cs, dy)
        inside = ~((xi >= N) | (xi < 0) | (yi >= N) | (yi < 0))
        xc, yc = np.where(inside, xi, 0), np.where(inside, yi, 0)
        p, lx, ly = (yc // D) * PX + xc // D, xc % D, yc % D
        # interpolateBilinear (TsdGrid.h:284-304, TsdGridPartition.h:214-221)
        wx, wy = np.abs((xs - dx) * inv), np.abs((ys - dy) * inv)
        t = tsd[p]
        k = np.arange(len(xs))
        v = (t[k, ly * PT + lx] * (1. - wy) * (1. - wx)
             + t[k, (ly + 1) * PT + lx] * wy * (1. - wx)
             + t[k, ly * PT + lx + 1] * (1. - wy) * wx
             + t[k, (ly + 1) * PT + lx + 1] * wy * wx)
    status = np.full(len(xs), SUCCESS, dtype=np.int64)
    status[np.isnan(v)] = ISNAN
    status[inside & (init[p] == 0)] = EMPTYPARTITION
    status[~inside] = INVALIDINDEX
    v = np.where((status == SUCCESS) | (status == ISNAN), v, np.nan)
    return status, v


def normal_samples(cs: float, xy):
    """the four positions interpolateNormal looks up for every point: (xs [n, 4], ys [n, 4]) in its order +x, -x, +y, -y"""
    cs = float(cs)
    x, y = xy[:, 0], xy[:, 1]
    return np.stack([x + cs, x - cs, x, x], axis=1), np.stack([y, y, y + cs, y - cs], axis=1)


def normals(map_size_log2: int, cs: float, init, tsd, xy):
    """TsdGrid::interpolateNormal at every point -> (normals [n, 2], ok [n] uint8): (0, 0) and ok = 0 where a look-up fails, left
    unnormalised where its length is <= 10e-6"""
    n = len(xy)
    if n == 0:
        return np.zeros((0, 2)), np.zeros(0, dtype=np.uint8)
    sx, sy = normal_samples(cs, xy)
    st, v = bilinear(map_size_log2, cs, init, tsd, sx.reshape(-1), sy.reshape(-1))
    st, v = st.reshape(n, 4), v.reshape(n, 4)
    ok = np.all(st == SUCCESS, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        nx, ny = v[:, 0] - v[:, 1], v[:, 2] - v[:, 3]
        length = np.sqrt(nx * nx + ny * ny)
        unit = ~(np.abs(length) <= 10e-6)
        nx, ny = np.where(unit, nx / length, nx), np.where(unit, ny / length, ny)
    out = np.stack([np.where(ok, nx, 0.0), np.where(ok, ny, 0.0)], axis=1)
    return out, ok.astype(np.uint8)


def surface(map_size_log2: int, cs: float, init, tsd, window=None):
    """the whole list: (xy, normals, ok, where)"""
    xy, where = points(map_size_log2, cs, init, tsd, window)
    nr, ok = normals(map_size_log2, cs, init, tsd, xy)
    return xy, nr, ok, where


def c_round(x: float) -> float:
    """C's round(): halfway cases away from zero"""
    f = math.floor(x)
    d = x - f
    if x >= 0.0:
        return float(f + 1) if d >= 0.5 else float(f)
    return float(f) if d <= 0.5 else float(f + 1)


def marks(map_size_log2: int, cs: float, xy):
    """ThreadGrid's marking rule (ThreadGrid.cpp:96-117, inflation off): the cells (u, v) of the accepted points, 0 < round(x / cs) < N"""
    N = 1 << map_size_log2
    cs = float(cs)
    out = []
    for x, y in xy.tolist():
        ru, rv = c_round(x / cs), c_round(y / cs)
        if 0.0 < ru < N and 0.0 < rv < N:
            out.append((int(ru), int(rv)))
    return out
