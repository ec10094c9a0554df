"""The frontier rules of include/tsd_hip.h restated in numpy and plain Python, written from the rules and not from the kernels:
classification by shifted comparisons, components by breadth-first search.  ``frontiers`` returns what tsd_frontiers_dev returns."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
DTYPE = np.dtype([("root_x", "<i4"), ("root_y", "<i4"), ("size", "<u4"), ("reachable", "<i4"), ("sum_x", "<u8"), ("sum_y", "<u8"),
                  ("min_x", "<i4"), ("min_y", "<i4"), ("max_x", "<i4"), ("max_y", "<i4")])
N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
N8 = N4 + ((1, 1), (1, -1), (-1, 1), (-1, -1))


def traversable(m, free_max=0):
    m = np.asarray(m, dtype=np.int8)
    return (m >= 0) & (m <= free_max)


def frontier_cells(m, free_max=0):
    """traversable cells with an unknown edge neighbour inside the map (the border is not unknown)"""
    m = np.asarray(m, dtype=np.int8)
    unk = m < 0
    near = np.zeros(m.shape, dtype=bool)
    near[:, 1:] |= unk[:, :-1]
    near[:, :-1] |= unk[:, 1:]
    near[1:, :] |= unk[:-1, :]
    near[:-1, :] |= unk[1:, :]
    return traversable(m, free_max) & near


def components(mask, neigh):
    """uint32 (H, W): the smallest linear index of each cell's component under ``neigh``, NONE off the mask.  Cells are visited in
    ascending linear index, so the cell a search starts from is its component's root."""
    H, W = mask.shape
    lab = np.full((H, W), NONE, dtype=np.uint32)
    for y0, x0 in zip(*np.nonzero(mask)):
        if lab[y0, x0] != NONE:
            continue
        root = int(y0) * W + int(x0)
        lab[y0, x0] = root
        q = deque([(int(x0), int(y0))])
        while q:
            x, y = q.popleft()
            for dx, dy in neigh:
                nx, ny = x + dx, y + dy
                if 0 <= nx < W and 0 <= ny < H and mask[ny, nx] and lab[ny, nx] == NONE:
                    lab[ny, nx] = root
                    q.append((nx, ny))
    return lab


def used_seeds(m, free_max, seeds):
    m = np.asarray(m, dtype=np.int8)
    H, W = m.shape
    t = traversable(m, free_max)
    return [(int(x), int(y)) for x, y in seeds if 0 <= x < W and 0 <= y < H and t[y, x]]


def frontiers(m, free_max=0, min_size=1, seeds=()):
    """(records in ascending root index, labels (H, W) uint32, seeds_used)"""
    m = np.asarray(m, dtype=np.int8)
    H, W = m.shape
    seeds = list(seeds)
    lab = components(frontier_cells(m, free_max), N8)
    used = used_seeds(m, free_max, seeds)
    seed_roots = set()
    if seeds:
        reg = components(traversable(m, free_max), N4)
        seed_roots = {int(reg[y, x]) for x, y in used}
    ys, xs = np.nonzero(lab != NONE)
    if xs.size == 0:
        return np.zeros(0, dtype=DTYPE), lab, len(used)
    order = np.argsort(lab[ys, xs], kind="stable")    # the cells grouped by root, roots ascending
    ys, xs = ys[order].astype(np.int64), xs[order].astype(np.int64)
    roots, start, size = np.unique(lab[ys, xs], return_index=True, return_counts=True)
    rec = np.zeros(roots.size, dtype=DTYPE)
    rec["root_x"], rec["root_y"], rec["size"] = roots % W, roots // W, size
    rec["sum_x"], rec["sum_y"] = np.add.reduceat(xs, start), np.add.reduceat(ys, start)
    rec["min_x"], rec["min_y"] = np.minimum.reduceat(xs, start), np.minimum.reduceat(ys, start)
    rec["max_x"], rec["max_y"] = np.maximum.reduceat(xs, start), np.maximum.reduceat(ys, start)
    rec["reachable"] = -1
    if seeds:
        hit = np.isin(reg[ys, xs], np.array(sorted(seed_roots), dtype=np.uint32)).astype(np.int32)
        rec["reachable"] = np.maximum.reduceat(hit, start)
    return rec[rec["size"] >= min_size], lab, len(used)
