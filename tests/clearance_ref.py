"""numpy restatement of the clearance field and the cost map (include/tsd_hip.h, "clearance"): the separable exact transform in
integers -- g along the rows, then the loop over dy --, the cost rule, the table formula and the window rule.  The device's outputs
are compared with these byte for byte."""
import numpy as np

NONE = 0xFFFF
OCCUPIED = 100


def row_distance(occ: np.ndarray, R: int) -> np.ndarray:
    """g: per cell the distance along its row to the nearest obstacle, capped at R + 1 (int64, same shape)"""
    H, W = occ.shape
    g = np.full((H, W), R + 1, dtype=np.int64)
    big = 1 << 30
    xs = np.arange(W)
    for y in range(H):
        ox = np.flatnonzero(occ[y])
        if ox.size == 0:
            continue
        last = np.where(occ[y], xs, -big)
        left = xs - np.maximum.accumulate(last)                      # to the nearest obstacle at or below x
        nxt = np.where(occ[y], xs, big)
        right = np.minimum.accumulate(nxt[::-1])[::-1] - xs          # ... at or above x
        g[y] = np.minimum(np.minimum(left, right), R + 1)
    return g


def dist2(src: np.ndarray, R: int) -> np.ndarray:
    """the distance field: uint16 (H, W), min over the obstacles (cells == 100) of dx^2 + dy^2 where <= R^2, else 0xFFFF"""
    src = np.asarray(src)
    H, W = src.shape
    g = row_distance(src == OCCUPIED, R)
    g2 = g * g
    best = g2.copy()
    for dy in range(1, R + 1):
        if dy >= H:
            break
        c = g2[:-dy] + dy * dy                   # row y - dy seen from row y
        best[dy:] = np.minimum(best[dy:], c)
        c = g2[dy:] + dy * dy                    # row y + dy
        best[:-dy] = np.minimum(best[:-dy], c)
    return np.where(best <= R * R, best, NONE).astype(np.uint16)


def cost_from(src: np.ndarray, d2: np.ndarray, table: np.ndarray, R: int) -> np.ndarray:
    """the cost rule: int8 (H, W)"""
    src = np.asarray(src, dtype=np.int8)
    table = np.asarray(table, dtype=np.int8)
    assert table.size == R * R + 1
    near = d2 != NONE
    c = table[np.where(near, d2, 0).astype(np.int64)]
    out = np.where((src == -1) & (c < 99), np.int8(-1), np.maximum(src, c)).astype(np.int8)
    return np.where(near, out, src).astype(np.int8)


def table(cell_size: float, R: int, inscribed_radius_m: float, cost_scaling: float) -> np.ndarray:
    """tsd_costmap_table's formula: int8 [R^2 + 1]"""
    d = np.sqrt(np.arange(R * R + 1, dtype=np.float64)) * cell_size
    e = 98.0 * np.exp(-cost_scaling * (d - inscribed_radius_m))
    t = np.clip(np.floor(np.minimum(e, 1e6)), 1, 98).astype(np.int8)        # (int) truncates: e > 0, so floor
    t[d <= inscribed_radius_m] = 99
    t[0] = 100
    return t


def grown(win, R: int, W: int, H: int):
    """a window (x, y, width, height) grown by R and clipped to the map; an empty one stays empty"""
    x, y, w, h = win
    if w == 0 or h == 0:
        return (0, 0, 0, 0)
    x0, y0 = max(0, x - R), max(0, y - R)
    return (x0, y0, min(W, x + w + R) - x0, min(H, y + h + R) - y0)


def both(src: np.ndarray, R: int, tab=None):
    """(dist2, cost or None) of a whole map"""
    d2 = dist2(src, R)
    return d2, (None if tab is None else cost_from(src, d2, tab, R))


def patch(old: np.ndarray, new: np.ndarray, win) -> np.ndarray:
    """`old` with the cells of window `win` taken from `new` (what a windowed call writes)"""
    x, y, w, h = win
    out = old.copy()
    out[y:y + h, x:x + w] = new[y:y + h, x:x + w]
    return out
