"""numpy restatement of the same-device merge group (``tsd_group_*``): the shifted, clipped signed-int8 maximum, and the rule that
turns two map origins into a whole-cell offset.  Written from the semantics stated in include/tsd_hip.h, not from the kernel."""
import numpy as np


def window(sizes, offsets=None, width=0, height=0):
    """(x0, y0, W, H): the merged window in the offsets' frame.  sizes: per member (h, w); width = height = 0: bounding box."""
    offsets = offsets if offsets is not None else [(0, 0)] * len(sizes)
    if width == 0 and height == 0:
        x0 = min(ox for ox, _ in offsets)
        y0 = min(oy for _, oy in offsets)
        x1 = max(ox + w for (ox, _), (_, w) in zip(offsets, sizes))
        y1 = max(oy + h for (_, oy), (h, _) in zip(offsets, sizes))
        return x0, y0, x1 - x0, y1 - y0
    return 0, 0, width, height


def merge(maps, offsets=None, width=0, height=0):
    """Member i's cell (x, y) lands in cell (x + ox_i, y + oy_i); a merged cell is the signed maximum over the members that cover it,
    -1 where none does; what falls outside the window is clipped.  Returns the (H, W) int8 map."""
    maps = [np.asarray(m, dtype=np.int8) for m in maps]
    offsets = offsets if offsets is not None else [(0, 0)] * len(maps)
    x0, y0, W, H = window([m.shape for m in maps], offsets, width, height)
    best = np.full((H, W), -129, dtype=np.int16)              # below every int8: "no member here"
    for m, (ox, oy) in zip(maps, offsets):
        h, w = m.shape
        dx, dy = ox - x0, oy - y0                             # where the member's cell (0, 0) lands in the window
        xa, xb = max(dx, 0), min(dx + w, W)
        ya, yb = max(dy, 0), min(dy + h, H)
        if xa >= xb or ya >= yb:
            continue
        src = m[ya - dy:yb - dy, xa - dx:xb - dx].astype(np.int16)
        best[ya:yb, xa:xb] = np.maximum(best[ya:yb, xa:xb], src)
    best[best == -129] = -1
    return best.astype(np.int8)


def n_occupied(merged):
    return int((np.asarray(merged) == 100).sum())


def map_origin(cells: int, cell_size: float, offset: float) -> float:
    """info.origin.position of a grid's map along one axis (ThreadGrid.cpp:28-29)"""
    return -(float(cells) * float(cell_size) * 0.5 + offset)


def cell_offset(origin: float, origin_ref: float, cell_size: float) -> int:
    """whole-cell offset of a map at `origin` relative to one at `origin_ref`; ValueError unless within 1e-6 cells of an integer"""
    d = (origin - origin_ref) / cell_size
    r = round(d)
    if abs(d - r) > 1e-6:
        raise ValueError(f"origins differ by {d!r} cells")
    return int(r)
