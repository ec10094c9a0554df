"""The windowed map update (tsd_map_update_begin) restated in numpy, for tests/test_cpu_map_update.py.

Built on map_edges_ref.MapRef (the reference's calcCoords and marking loop in its own serial order).  A windowed update is given the
tile box D that holds every tile which may have changed since the previous frame and does two things:

  * cells pass: the persistent map and the staged map are rewritten for the cells of the tiles of U = D grown by g tiles,
  * mark pass:  the marks of the scanned tiles of U' = U grown by g tiles again are made, unclipped,

with g = ceil((factor + 1) / 32) tiles when inflation is on and 1 when it is off, both boxes clipped to the grid.  Nothing here calls
into oracle/ or the device library.
"""
from __future__ import annotations

import numpy as np

from tests.map_edges_ref import D, MapRef, c_round


def growth(inflate: bool, factor: int) -> int:
    """tiles a mark can land away from the tile that makes it: its cell is at most one past the tile's 32 and the inflated square
    reaches `factor` cells further"""
    return (int(factor) + 1 + D - 1) // D if inflate else 1


def grow(box, by: int, PX: int):
    """an inclusive tile box (x0, y0, x1, y1) grown by `by` tiles on every side, clipped to the grid"""
    x0, y0, x1, y1 = box
    return (max(0, x0 - by), max(0, y0 - by), min(PX - 1, x1 + by), min(PX - 1, y1 + by))


def windows(box, inflate: bool, factor: int, PX: int):
    """-> (U, U') of the changed box D"""
    g = growth(inflate, factor)
    u = grow(box, g, PX)
    return u, grow(u, g, PX)


def cells_of(box):
    """the cell rectangle of a tile box as two slices (rows, columns)"""
    x0, y0, x1, y1 = box
    return slice(y0 * D, (y1 + 1) * D), slice(x0 * D, (x1 + 1) * D)


def tile_in(p: int, box, PX: int) -> bool:
    x0, y0, x1, y1 = box
    return x0 <= p % PX <= x1 and y0 <= p // PX <= y1


def mark(out_flat, coords, N: int, cs: float, inflate: bool, factor: int):
    """ThreadGrid.cpp:93-118 on a flat (N * N) map, as MapRef.occupancy states it: the `unsigned int` bounds wrap (no inflation where
    u < factor or v < factor), a column index past N lands in the next row, writes past the map are dropped.  -> writes with j >= N"""
    size, f, spilled = N * N, int(factor), 0
    for x, y in coords:
        ru, rv = c_round(x / cs), c_round(y / cs)
        if not (0.0 < ru < N and 0.0 < rv < N):
            continue
        u, v = int(ru), int(rv)
        out_flat[v * N + u] = 100
        if not inflate or f <= 0 or u < f or v < f:
            continue
        j = np.arange(u - f, u + f, dtype=np.int64)
        idx = (np.arange(v - f, v + f, dtype=np.int64)[:, None] * N + j[None, :])
        keep = idx < size
        spilled += int((keep & (j[None, :] >= N)).sum())
        out_flat[idx[keep]] = 100
    return spilled


def full_frame(ref: MapRef, init, iw, tsd, inflate: bool, factor: int):
    """the full frame of the grid on ref's persistent map (which it updates): -> (map (N, N), coords, events, spilled)"""
    coords, events = ref.calc_coords(init, iw, tsd)
    out = ref.content.copy()
    spilled = mark(out, coords, ref.N, ref.cs, inflate, factor)
    return out.reshape(ref.N, ref.N), coords, events, spilled


def windowed_update(old_content, old_map, new_content, coords, events, box, inflate: bool, factor: int, PX: int, cs: float):
    """"cells in U, marks from U'" applied to the previous frame.  old_content / old_map: the persistent and the staged map after the
    previous frame; new_content: the persistent map a pass over ALL tiles of the new grid leaves (only its U cells are used);
    coords / events: calcCoords' output for the new grid (events[k][0] is the tile that made coords[k]).
    -> (persistent map, staged map) after the update, both (N, N)"""
    N = old_map.shape[0]
    u, m = windows(box, inflate, factor, PX)
    rows, cols = cells_of(u)
    content = old_content.reshape(N, N).copy()
    staged = old_map.copy()
    content[rows, cols] = new_content.reshape(N, N)[rows, cols]
    staged[rows, cols] = content[rows, cols]
    flat = staged.reshape(-1)
    mark(flat, [c for c, e in zip(coords, events) if tile_in(e[0], m, PX)], N, cs, inflate, factor)
    return content, staged
