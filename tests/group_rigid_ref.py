"""numpy restatement of the merge group under rigid transforms (``tsd_group_create_rigid``): the window, the footprint of a window cell
in a member, the merged map, and the agreement measure the tests use.  Written from the rule stated in include/tsd_hip.h, not from the
kernel: fp64 throughout, one rounding per operation, in the header's order (numpy's multiply and add are separate loops: nothing is
contracted)."""
import math

import numpy as np


def rigid(angle, tx=0.0, ty=0.0):
    """T = [c -s tx; s c ty; 0 0 1] for an angle in radians"""
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, tx], [s, c, ty], [0.0, 0.0, 1.0]])


def about(angle, pivot, shift=(0.0, 0.0)):
    """the rotation by `angle` about `pivot`, then a shift"""
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, pivot[0] - (c * pivot[0] - s * pivot[1]) + shift[0]],
                     [s, c, pivot[1] - (s * pivot[0] + c * pivot[1]) + shift[1]], [0.0, 0.0, 1.0]])


def quarter_turn(k, side_m):
    """the exact rotation by k * 90 degrees about the centre of a grid `side_m` metres wide: entries 0 and +-1, nothing rounded"""
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][k % 4]
    h = 0.5 * side_m
    return np.array([[c, -s, h - (c * h - s * h)], [s, c, h - (s * h + c * h)], [0.0, 0.0, 1.0]])


def shift(ox, oy, cs):
    """the whole-cell shift of a translation group as a transform"""
    return np.array([[1.0, 0.0, float(ox) * cs], [0.0, 1.0, float(oy) * cs], [0.0, 0.0, 1.0]])


def _parts(T):
    T = np.asarray(T, dtype=np.float64)
    return float(T[0, 0]), float(T[1, 0]), float(T[0, 2]), float(T[1, 2])


def window(sizes, Ts, cs, width=0, height=0):
    """(x0, y0, W, H) in frame cells.  sizes: per member (h, w), squares.  width = height = 0: the bounding box rule."""
    if width != 0 or height != 0:
        return 0, 0, width, height
    xs, ys = [], []
    for (_, w), T in zip(sizes, Ts):
        c, s, tx, ty = _parts(T)
        L = float(w) * cs
        for x in (0.0, L):
            for y in (0.0, L):
                xs.append((c * x - s * y) + tx)
                ys.append((s * x + c * y) + ty)
    x0, x1 = math.floor(min(xs) / cs + 1e-9), math.ceil(max(xs) / cs - 1e-9)
    y0, y1 = math.floor(min(ys) / cs + 1e-9), math.ceil(max(ys) / cs - 1e-9)
    return x0, y0, x1 - x0, y1 - y0


def footprint(T, cs, x0, y0, W, H):
    """(kx_lo, kx_hi, ky_lo, ky_hi), int64 (H, W) each: the source cells of every window cell, before clipping to the member"""
    c, s, tx, ty = _parts(T)
    px = ((x0 + np.arange(W, dtype=np.int64)).astype(np.float64) + 0.5) * cs
    py = ((y0 + np.arange(H, dtype=np.int64)).astype(np.float64) + 0.5) * cs
    dx, dy = (px - tx)[None, :], (py - ty)[:, None]
    qx = c * dx + s * dy
    qy = c * dy - s * dx
    u, v = qx / cs, qy / cs
    return (np.ceil(u - 1.25).astype(np.int64), np.floor(u + 0.25).astype(np.int64),
            np.ceil(v - 1.25).astype(np.int64), np.floor(v + 0.25).astype(np.int64))


def merge(maps, Ts, cs, width=0, height=0):
    """the merged (H, W) int8 map: per member the signed maximum over the footprint cells inside it, over the members that cover the
    cell the signed maximum again, -1 where none does"""
    maps = [np.asarray(m, dtype=np.int8) for m in maps]
    x0, y0, W, H = window([m.shape for m in maps], Ts, cs, width, height)
    best = np.full((H, W), -129, dtype=np.int16)              # below every int8: "no member here"
    for m, T in zip(maps, Ts):
        h, w = m.shape
        xa, xb, ya, yb = footprint(T, cs, x0, y0, W, H)
        xa, xb, ya, yb = np.maximum(xa, 0), np.minimum(xb, w - 1), np.maximum(ya, 0), np.minimum(yb, h - 1)
        covered = (xa <= xb) & (ya <= yb)
        xa, xb, ya, yb = (np.clip(k, 0, lim - 1) for k, lim in ((xa, w), (xb, w), (ya, h), (yb, h)))      # (for the gather only)
        m16 = m.astype(np.int16)
        val = np.maximum(np.maximum(m16[ya, xa], m16[ya, xb]), np.maximum(m16[yb, xa], m16[yb, xb]))
        best = np.where(covered, np.maximum(best, val), best)
    best[best == -129] = -1
    return best.astype(np.int8)


def n_occupied(merged):
    return int((np.asarray(merged) == 100).sum())


def agreement(dst_map, warped_map, reach=2):
    """(share, hits, counted): of the cells of `warped_map` equal to 100 where `dst_map` is known (not -1), the share that lies within
    `reach` cells (Chebyshev) of a cell of `dst_map` equal to 100.  Both maps in one frame, same shape."""
    dst, wrp = np.asarray(dst_map), np.asarray(warped_map)
    assert dst.shape == wrp.shape
    occ = dst == 100
    H, W = occ.shape
    pad = np.zeros((H + 2 * reach, W + 2 * reach), dtype=bool)
    pad[reach:reach + H, reach:reach + W] = occ
    near = np.zeros_like(occ)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            near |= pad[dy:dy + H, dx:dx + W]
    counted = (wrp == 100) & (dst != -1)
    n = int(counted.sum())
    hits = int((counted & near).sum())
    return (hits / n if n else 0.0), hits, n
