"""A third opinion on the published map, written for tests/test_cpu_map_edges.py and tests/test_gpu_map_edges.py.

Plain Python / numpy restatements, in the reference's own serial order, of
  * RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105) with its persistent occupiedGrid,
  * the marking loop of ThreadGrid::eventLoop (ThreadGrid.cpp:93-118) with its wrapping `unsigned int` bounds,
  * TsdGrid::grid2ColorImage (TsdGrid.cpp:429-488) with its `px += stepW` accumulation,
on the canonical tile dump (flags, initWeight, 33 x 33 row-major tsd per tile) that `download_tiles()` / `dump()` hand out.  Nothing
here calls into oracle/ or the device library.  The module also holds what the two test modules share: a builder of hand-made grids,
the case table and the script of the reuse sequence.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

D = 32             # cells per tile side
PT = 33            # pitch of the canonical dump: the tile plus its one-cell halo
TC = PT * PT
U32 = np.uint32
ROW, COL = 0, 1    # axis of a scan


def c_round(x: float) -> float:
    """C's round(): halfway cases away from zero (x - floor(x) is exact in binary floating point)"""
    if x != x or x in (math.inf, -math.inf):
        return x
    f = math.floor(x)
    d = x - f
    if x >= 0.0:
        return float(f + 1) if d >= 0.5 else float(f)
    return float(f) if d <= 0.5 else float(f + 1)


class MapRef:
    """ThreadGrid's state and outputs for one grid: `content` is _occGridContent (-1 at construction, ThreadGrid.cpp:27-28, and
    never cleared afterwards: neither ThreadGrid nor TsdGrid::reset touches it)."""

    def __init__(self, map_size_log2: int, cell_size: float):
        self.N = 1 << map_size_log2
        self.PX = self.N // D
        self.cs = float(cell_size)
        self.content = np.full(self.N * self.N, -1, dtype=np.int8)

    # RayCastAxisAligned2D.cpp:13-105
    def calc_coords(self, init, iw, tsd):
        """-> (coords [(x, y)], events [(tile, py, px, axis)]) in the reference's order; writes self.content"""
        N, PX, cs, content = self.N, self.PX, self.cs, self.content
        cellsPPart, cellsPPX = D * D, D
        coords, events = [], []
        for y in range(1, PX - 1):                       # (unsigned 1 .. partitions-2; no round at all for PX < 3)
            for x in range(1, PX - 1):
                p = y * PX + x
                off = y * cellsPPart * PX + x * cellsPPX
                if init[p]:                              # (an initialised partition is never isEmpty(), TsdGridPartition.h:72)
                    t = np.asarray(tsd[p], dtype=np.float64).reshape(PT, PT).tolist()
                    for py in range(D + 1):
                        prev = t[py][0]
                        content[off + py * N] = 0 if prev > 0.0 else -1
                        for px in range(1, D + 1):
                            v = t[py][px]
                            content[off + py * N + px] = 0 if v > 0.0 else -1
                            if (prev > 0 and v < 0) or (prev < 0 and v > 0):
                                interp = prev / (prev - v)
                                coords.append((px * cs + cs * (interp - 1.0) + (x * D) * cs, py * cs + (y * D) * cs))
                                events.append((p, py, px, ROW))
                            prev = v
                    for px in range(D + 1):
                        prev = t[0][px]
                        for py in range(1, D + 1):
                            v = t[py][px]
                            if (prev > 0 and v < 0) or (prev < 0 and v > 0):
                                interp = prev / (prev - v)
                                coords.append((px * cs + (x * D) * cs, py * cs + cs * (interp - 1.0) + (y * D) * cs))
                                events.append((p, py, px, COL))
                            prev = v
                elif iw[p] > 0.0:                        # isEmpty(): the 32 x 32 interior only
                    for py in range(D):
                        content[off + py * N] = 0
                        for px in range(1, D):
                            content[off + py * N + px] = 0
        return coords, events

    # ThreadGrid.cpp:91-118
    def occupancy(self, init, iw, tsd, inflate: bool, factor: int):
        """-> (map (N, N) int8, n_surface, info).  info: events, coords, marks [(u, v)] of the accepted coordinates, and how many
        inflation writes spilled into the next row (j >= N), how many were dropped (see below), how many marks inflated at all."""
        N, cs = self.N, self.cs
        coords, events = self.calc_coords(init, iw, tsd)
        out = self.content.copy()
        W, f = U32(N), U32(int(factor) & 0xFFFFFFFF)
        size = N * N
        marks, spilled, dropped, inflated = [], 0, 0, 0
        for x, y in coords:
            ru, rv = c_round(x / cs), c_round(y / cs)
            # the accepted range, decided in double: the reference casts first, which is only defined inside this range
            if not (0.0 < ru < N and 0.0 < rv < N):
                continue
            u, v = U32(ru), U32(rv)
            out[int(v * W + u)] = 100
            marks.append((int(u), int(v)))
            if not inflate:
                continue
            with np.errstate(over="ignore"):
                i0, i1, j0, j1 = v - f, v + f, u - f, u + f          # unsigned: v - f wraps for v < f and the loop does not run
                wrote = False
                i = i0
                while i < i1:
                    j = j0
                    while j < j1:
                        idx = int(i * W + j)
                        if idx < size:
                            out[idx] = 100
                            wrote = True
                            spilled += int(j) >= N
                        else:
                            # The reference writes past the end of `data` here (undefined).  Dropping the write is what the
                            # device and the oracle chose (i * N + j < N * N); the tests assert it on both.
                            dropped += 1
                        j = j + U32(1)
                    i = i + U32(1)
                inflated += wrote
        info = dict(events=events, coords=coords, marks=marks, spilled=spilled, dropped=dropped, inflated=inflated)
        return out.reshape(N, N), len(coords), info

    # TsdGrid.cpp:429-488 with coord2Cell (TsdGrid.h:306-340)
    def color_image(self, init, iw, tsd, width: int, height: int):
        N, PX, cs = self.N, self.PX, self.cs
        inv = 1.0 / cs
        max_xy = (float(N) + 0.5) * cs                   # _maxX / _maxY (TsdGrid.cpp:142-144)

        def axis(n):
            step = max_xy / float(n)
            c, v = np.empty(n), 0.0
            for k in range(n):                           # px += stepW
                c[k] = v
                v += step
            i = np.floor(c * inv)
            centre = (i + 0.5) * cs
            i = np.where(c < centre, i - 1.0, i).astype(np.int64)
            return i

        xi, yi = axis(width), axis(height)
        XI, YI = np.meshgrid(xi, yi)                     # (height, width)
        ok = (XI >= 0) & (XI < N) & (YI >= 0) & (YI < N)
        xc, yc = np.where(ok, XI, 0), np.where(ok, YI, 0)
        p = yc // D * PX + xc // D
        lx, ly = xc % D, yc % D
        init_b = np.asarray(init).astype(bool)
        t = np.where(ok & init_b[p], np.asarray(tsd, dtype=np.float64)[p, ly * PT + lx], np.nan)
        empty = ok & ~init_b[p] & (np.asarray(iw)[p] > 0.0)
        img = np.zeros((height, width, 3), dtype=np.uint8)
        pos, neg = t > 0.0, t < 0.0
        with np.errstate(invalid="ignore"):
            vp = np.trunc(np.where(pos, t, 0.0) * 255.0).astype(np.uint8)
            vn = np.trunc((1.0 + np.where(neg, t, 0.0)) * 255.0).astype(np.uint8)
        img[pos, 0] = vp[pos]; img[pos, 1] = 255; img[pos, 2] = vp[pos]
        img[neg, 0] = vn[neg]
        white = ~pos & ~neg & empty
        img[white] = 255
        return img


def raw_sign_changes(init, tsd, tiles=None) -> int:
    """sign changes of the row and column scans of the given tiles (default: all initialised ones), whether calcCoords visits them or not"""
    n = 0
    for p in (range(len(init)) if tiles is None else tiles):
        if not init[p]:
            continue
        t = np.asarray(tsd[p]).reshape(PT, PT)
        with np.errstate(invalid="ignore"):
            a, b = t[:, :-1], t[:, 1:]
            n += int((((a > 0) & (b < 0)) | ((a < 0) & (b > 0))).sum())
            a, b = t[:-1, :], t[1:, :]
            n += int((((a > 0) & (b < 0)) | ((a < 0) & (b > 0))).sum())
    return n


def listed_tiles(map_size_log2: int, init) -> int:
    """how many tiles calcCoords scans: initialised and not on the outer ring (the device's work list holds exactly these)"""
    PX = (1 << map_size_log2) // D
    f = np.asarray(init).reshape(PX, PX).astype(bool)
    return int(f[1:PX - 1, 1:PX - 1].sum()) if PX >= 3 else 0


# ---------------------------------------------------------------------------------------------------------------------------------
class TileGrid:
    """A grid made by hand in the canonical layout.  `set_cell` writes a GLOBAL cell into its owner tile and into the halo copies the
    left / lower / diagonal neighbours keep of it, so that a sign change sits where a case wants it and the 33 x 33 tiles agree."""

    def __init__(self, map_size_log2: int):
        self.map_size_log2 = map_size_log2
        self.N = 1 << map_size_log2
        self.PX = self.N // D
        T = self.PX * self.PX
        self.init = np.zeros(T, dtype=np.uint8)
        self.iw = np.zeros(T)
        self.tsd = np.full((T, TC), np.nan)
        self.w = np.zeros((T, TC))

    def tile(self, X, Y):
        return Y * self.PX + X

    def init_tile(self, p, fill=np.nan):
        self.init[p] = 1
        self.tsd[p, :] = fill
        self.w[p, :] = 0.0 if fill != fill else 1.0
        return self

    def empty_tile(self, p, weight=1.0):
        self.init[p] = 0
        self.iw[p] = weight
        return self

    def set_local(self, p, row, col, value):
        """one entry of one tile's 33 x 33 array, nothing else (this is how a halo is made to disagree with its owner)"""
        assert self.init[p] and 0 <= row <= D and 0 <= col <= D
        self.tsd[p, row * PT + col] = value
        self.w[p, row * PT + col] = 1.0

    def set_cell(self, gx, gy, value):
        X, Y, lx, ly = gx // D, gy // D, gx % D, gy % D
        for dX, dY in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
            if (dX and lx) or (dY and ly):
                continue
            qx, qy = X + dX, Y + dY
            if not (0 <= qx < self.PX and 0 <= qy < self.PX):
                continue
            q = self.tile(qx, qy)
            if self.init[q]:
                self.set_local(q, ly + (D if dY else 0), lx + (D if dX else 0), value)

    def place(self, changes):
        """changes: (tile, row, col, prev_value, cur_value, axis) with row / col in 0..32 of the tile: the pair that the tile's row scan
        (axis ROW: prev at col - 1) or column scan (axis COL: prev at row - 1) compares at (row, col)"""
        for p, row, col, prev, cur, ax in changes:
            X, Y = p % self.PX, p // self.PX
            gx, gy = X * D + col, Y * D + row
            self.set_cell(gx - (ax == ROW), gy - (ax == COL), prev)
            self.set_cell(gx, gy, cur)
        return self

    def fill_from(self, fn, tiles):
        """initialise `tiles` with fn(gx, gy) (arrays) evaluated at the global cell of every entry, halo included: consistent tiles"""
        ly, lx = np.meshgrid(np.arange(PT), np.arange(PT), indexing="ij")
        for p in tiles:
            X, Y = p % self.PX, p // self.PX
            self.init[p] = 1
            self.tsd[p] = fn(X * D + lx, Y * D + ly).reshape(-1)
            self.w[p] = 1.0
        return self

    def arrays(self):
        return self.init.copy(), self.iw.copy(), self.tsd.copy(), self.w.copy()


# ---------------------------------------------------------------------------------------------------------------------------------
FACTORS = (0, 1, 2, 3, 33, None)       # None: the map's own size N


@dataclass
class Case:
    name: str
    map_size_log2: int
    cell_size: float
    grid: TileGrid
    params: list                       # [(inflate, factor)]
    reach: object                      # reach(case, results): asserts that the case gets where it is meant to; results[k] = (map, n, info)
    notes: dict = field(default_factory=dict)


def _inner(g):
    return [g.tile(X, Y) for Y in range(1, g.PX - 1) for X in range(1, g.PX - 1)]


def _stripes(gx, gy):
    return np.where((gy // 5 + gx // 7) % 2 == 0, 0.4, -0.6).astype(np.float64)


def case_tiny(map_size_log2):
    """map_size 5 / 6: one tile / 2 x 2 tiles, every tile on the outer ring: the map stays -1 and nothing is marked"""
    g = TileGrid(map_size_log2)
    g.fill_from(_stripes, range(g.PX * g.PX))

    def reach(case, results):
        init, _, tsd, _ = case.grid.arrays()
        assert raw_sign_changes(init, tsd) > 100, "the tiles hold no sign changes"
        for occ, n, info in results:
            assert n == 0 and not info["marks"], "a tile of the outer ring was scanned"
            assert (occ == -1).all()
    return Case(f"tiny{map_size_log2}", map_size_log2, 0.05, g, [(False, 2), (True, 2), (True, 33)], reach)


def case_border(map_size_log2, inflate, factor):
    """marks on the first and last cells a scanned tile can reach (32 and N - 32 on either axis) plus one in the middle, with every
    inflation factor.  A mark's cell is >= 32 (the outer ring of tiles is never scanned), so `u < factor`, the row spill and the
    clamped top only happen for factors above a tile (33, N); for the smaller factors the case asserts the extreme cells instead."""
    g = TileGrid(map_size_log2)
    N, PX = g.N, g.PX
    fac = N if factor is None else factor
    for p in _inner(g):
        g.init_tile(p)
    lo, hi = 1, PX - 2
    g.place([
        (g.tile(lo, lo), 0, 1, 0.1, -0.9, ROW),          # x = 32.1 cells -> u = 32, v = 32
        (g.tile(hi, lo), 5, D, 0.9, -0.1, ROW),          # cur in the halo column: u = N - 32
        (g.tile(lo, hi), D, 7, 0.9, -0.1, COL),          # cur in the halo row: v = N - 32
        (g.tile(hi, hi), D, D, -0.9, 0.1, ROW),          # the halo row's last pair: u = v = N - 32
        (g.tile(lo, lo), 20, 20, 0.5, -0.5, ROW),        # the middle: u = 52
        (g.tile(hi, hi), 3, 9, -0.25, 0.75, COL),
    ])

    def reach(case, results):
        (occ, n, info), = results
        us = [u for u, _ in info["marks"]]; vs = [v for _, v in info["marks"]]
        assert n == len(info["marks"]) >= 6
        assert min(us) == 32 and min(vs) == 32 and max(us) == N - 32 and max(vs) == N - 32, (us, vs)
        if not inflate:
            assert (occ == 100).sum() == len(set(info["marks"]))
            return
        if fac == 0:
            assert info["inflated"] == 0 and (occ == 100).sum() == len(set(info["marks"]))
        if fac >= 33:
            assert any(u < fac for u in us) and any(v < fac for v in vs)
            assert any(u + fac > N for u in us) and any(v + fac > N for v in vs)
        if fac == 33:
            assert info["inflated"] >= 1 and info["spilled"] > 0 and info["dropped"] > 0, info
            assert occ[N - 1, :].any() and (occ[:, 0] == 100).any()       # the clamped top row is written, the spill reaches column 0
            assert info["inflated"] < len(info["marks"]), "no mark lost its inflation to the wrapped start"
        if fac == N:
            assert info["inflated"] == 0, "a factor of the map's size wraps every start"
        if 1 <= fac <= 3:
            assert info["inflated"] == len(info["marks"]) and info["spilled"] == 0 and info["dropped"] == 0
    return Case(f"border{map_size_log2}-{'inflate' if inflate else 'plain'}-{'N' if factor is None else factor}", map_size_log2, 0.05, g,
                [(inflate, fac)], reach)


def case_seam():
    """sign changes across tile seams: the pair's second cell is the neighbour's halo copy, or both cells lie in the halo column / row"""
    g = TileGrid(7)
    for p in _inner(g):
        g.init_tile(p)
    for gx, gy, v in ((63, 40, 0.3), (64, 40, -0.7), (65, 40, 0.2),          # across the column seam, then back inside the right tile
                      (64, 50, 0.4), (64, 51, -0.6),                          # along the seam: column scan of the halo column
                      (70, 63, -0.2), (70, 64, 0.8), (71, 64, -0.8),          # across and along the row seam
                      (63, 64, 0.5), (64, 64, -0.5), (64, 63, 0.25), (63, 63, -0.35)):   # around the corner cell of four tiles
        g.set_cell(gx, gy, v)

    def reach(case, results):
        ev = results[0][2]["events"]
        assert any((ax == COL and px == D) or (ax == ROW and py == D) for _, py, px, ax in ev), "no change with its prev in a halo cell"
        assert any(ax == ROW and px == D and py < D for _, py, px, ax in ev), "no row change from the interior into the halo column"
        assert any(ax == COL and py == D and px < D for _, py, px, ax in ev), "no column change from the interior into the halo row"
        assert any(py == D and px == D for _, py, px, ax in ev), "the halo's corner cell takes part in no change"
        assert len({p for p, *_ in ev}) == 4
    return Case("seam", 7, 0.05, g, [(False, 2), (True, 2)], reach)


def case_seam_inconsistent():
    """a halo copy that disagrees with its owner: the left tile's scans read ITS copy (a change the owner's value would not give), and
    the map cell of the seam is the owner's (the later writer of the serial tile order)"""
    g = TileGrid(7)
    for p in _inner(g):
        g.init_tile(p)
    left, right = g.tile(1, 1), g.tile(2, 1)
    g.set_cell(63, 40, -0.3)
    g.set_cell(64, 40, -0.5)                  # owner (right tile, column 0) and the left tile's halo copy ...
    g.set_local(left, 8, D, 0.5)              # ... which is then made to disagree
    g.set_cell(65, 41, 0.5)
    g.set_cell(64, 41, 0.5)
    g.set_local(left, 9, D, -0.5)             # and the other way round one row up

    def reach(case, results):
        occ, n, info = results[0]
        assert (left, 8, D, ROW) in info["events"], "the left tile did not scan its own halo copy"
        assert not any(p == right and py == 8 and px == 1 for p, py, px, ax in info["events"])
        assert occ[40, 64] in (-1, 100) and case.grid.tsd[left, 8 * PT + D] > 0, "the seam cell is not the owner's"
        assert occ[41, 64] in (0, 100) and case.grid.tsd[left, 9 * PT + D] < 0
    return Case("seam-inconsistent", 7, 0.05, g, [(False, 2)], reach)


def case_ring_tiles_skipped():
    """initialised tiles on the outer ring are not scanned (the reference's loops run 1 .. partitions-2), the tiles next to them are,
    and those write their halo into the ring tiles' first column / row"""
    g = TileGrid(7)
    ring = [g.tile(0, 1), g.tile(1, 0), g.tile(3, 2), g.tile(2, 3), g.tile(3, 3), g.tile(0, 0)]
    g.fill_from(_stripes, ring)
    g.fill_from(lambda gx, gy: np.where(gx + gy > 150, 0.5, -0.5).astype(np.float64), [g.tile(2, 2)])
    g.init_tile(g.tile(1, 1))
    g.place([(g.tile(1, 1), 3, 3, 0.5, -0.5, ROW)])

    def reach(case, results):
        occ, n, info = results[0]
        init, _, tsd, _ = case.grid.arrays()
        assert raw_sign_changes(init, tsd, ring) > 100
        assert {p for p, *_ in info["events"]} == {g.tile(1, 1), g.tile(2, 2)}
        assert n == raw_sign_changes(init, tsd, [g.tile(1, 1), g.tile(2, 2)])
        assert (occ[0:32, :] == -1).all() and (occ[:, 0:32] == -1).all() and (occ[97:, :] == -1).all() and (occ[:, 97:] == -1).all()
        assert (occ[64:97, 96] != -1).any(), "tile (2, 2) wrote no halo into the ring tile's first column"
    return Case("ring-tiles-skipped", 7, 0.05, g, [(False, 2), (True, 3)], reach)


def case_exact_zero():
    """0.0 / -0.0 on one side of a pair is no sign change (the tests are > and <), a strict pair next to them is"""
    g = TileGrid(7)
    p = g.tile(1, 2)
    g.init_tile(p)
    pairs = [(2, 0.0, -0.5), (4, 0.5, 0.0), (6, -0.0, 0.5), (8, -0.5, -0.0), (10, 0.0, 0.0), (12, 0.5, -0.5)]
    g.place([(p, row, 10, a, b, ROW) for row, a, b in pairs])

    def reach(case, results):
        occ, n, info = results[0]
        assert n == 1 and info["events"] == [(p, 12, 10, ROW)]
        assert sum(1 for _, a, b in pairs if a == 0.0 or b == 0.0) == 5
    return Case("exact-zero", 7, 0.05, g, [(False, 2), (True, 2)], reach)


def case_nan_neighbours():
    """NaN cells and uninitialised neighbours (NaN halo) next to signed cells give no change; NaN cells are -1 in the map"""
    g = TileGrid(7)
    p = g.tile(2, 1)                                        # its right neighbour is a ring tile, its upper one stays uninitialised
    g.init_tile(p)
    for r in range(4, 12):
        for c in range(28, D):                              # a positive block up to the tile's last column: the halo column is NaN
            g.set_cell(2 * D + c, D + r, 0.5)
    for c in range(3, 9):
        g.set_cell(2 * D + c, D + 31, -0.5)                 # a negative run in the last row: the halo row is NaN
    g.place([(p, 20, 20, -0.5, 0.5, COL)])

    def reach(case, results):
        occ, n, info = results[0]
        assert n == 1 and info["events"] == [(p, 20, 20, COL)]
        t = case.grid.tsd[p].reshape(PT, PT)
        assert np.isnan(t[4:12, D]).all() and (t[4:12, D - 1] > 0).all() and np.isnan(t[D, 3:9]).all() and (t[D - 1, 3:9] < 0).all()
        assert (occ[D + 4:D + 12, 2 * D + 28:2 * D + 32] == 0).all() and (occ[D + 4:D + 12, 3 * D] == -1).all()
    return Case("nan-neighbours", 7, 0.05, g, [(False, 2), (True, 1)], reach)


def case_half_cells():
    """interpolations that land exactly on x.5 cells: a cell size that is a power of two makes the arithmetic exact, prev = -cur puts
    the surface half-way; C's round goes away from zero where rint would go to the even cell"""
    g = TileGrid(7)
    p = g.tile(1, 1)
    g.init_tile(p)
    g.place([(p, 3, 4, 0.25, -0.25, ROW), (p, 3, 9, -0.25, 0.25, ROW), (p, 10, 20, 0.5, -0.5, COL), (p, 15, 20, -0.5, 0.5, COL)])

    def reach(case, results):
        occ, n, info = results[0]
        halves = [c / case.cell_size for xy in info["coords"] for c in xy if (c / case.cell_size) % 1.0 == 0.5]
        assert len(halves) == 4
        assert any(math.floor(h) % 2 == 0 for h in halves), "no x.5 with an even floor: rint would agree with round"
        assert any(math.floor(h) % 2 == 1 for h in halves)
        assert (D + 9, D + 3) in info["marks"] and (D + 20, D + 15) in info["marks"]        # 40.5 -> 41 and 46.5 -> 47
    return Case("half-cells", 7, 0.125, g, [(False, 2), (True, 2)], reach)


def case_row_and_column_same_mark():
    """a row scan and a column scan that round to the same cell: one mark, two surface points"""
    g = TileGrid(7)
    p = g.tile(2, 2)
    g.init_tile(p)
    g.set_cell(2 * D + 10, 2 * D + 10, -0.1)
    g.set_cell(2 * D + 9, 2 * D + 10, 0.9)
    g.set_cell(2 * D + 10, 2 * D + 9, 0.9)

    def reach(case, results):
        occ, n, info = results[0]
        assert n == 2 and {ax for *_, ax in info["events"]} == {ROW, COL}
        assert info["marks"][0] == info["marks"][1] == (2 * D + 10, 2 * D + 10)
        assert (occ == 100).sum() == 1
    return Case("row-and-column-same-mark", 7, 0.05, g, [(False, 2)], reach)


def mixed_grid(map_size_log2=7, seed=5):
    """cells of every kind for the images: positive, negative, NaN, an empty tile, untouched tiles, initialised ring tiles"""
    g = TileGrid(map_size_log2)
    rng = np.random.default_rng(seed)

    def noisy(gx, gy):
        v = np.clip(0.9 * np.sin(gx * 0.21) * np.cos(gy * 0.17) + 0.1 * rng.standard_normal(gx.shape), -1.0, 1.0)
        v[(gx * 7 + gy * 3) % 11 == 0] = np.nan
        return v
    tiles = [g.tile(1, 1), g.tile(2, 1), g.tile(2, 2), g.tile(0, 0), g.tile(g.PX - 1, 2), g.tile(1, g.PX - 1)]
    g.fill_from(lambda gx, gy: np.clip(0.9 * np.sin(gx * 0.21) * np.cos(gy * 0.17), -1.0, 1.0), tiles)
    for p in tiles:                                         # per-tile noise and holes (tiles need not agree for an image)
        ly, lx = np.meshgrid(np.arange(PT), np.arange(PT), indexing="ij")
        g.tsd[p] = noisy(lx + 3 * p, ly + 5 * p).reshape(-1)
    g.tsd[g.tile(2, 2), 5 * PT + 5] = 1.0
    g.tsd[g.tile(2, 2), 5 * PT + 6] = -1.0
    g.tsd[g.tile(2, 2), 5 * PT + 7] = 0.0
    g.empty_tile(g.tile(1, 2), 3.0)
    g.empty_tile(g.tile(0, 2), 1.0)
    return g


IMAGE_SIZES = [(1, 1), (1, 9), (9, 1), (256, 5), (257, 5), (512, 3), (255, 2), (259, 259), (128, 128), (100, 77), (3, 300)]   # (width, height)


def table():
    cases = [case_tiny(5), case_tiny(6)]
    for log2 in (7, 9):
        for inflate in (False, True):
            for factor in FACTORS:
                cases.append(case_border(log2, inflate, factor))
    cases += [case_seam(), case_seam_inconsistent(), case_ring_tiles_skipped(), case_exact_zero(), case_nan_neighbours(),
              case_half_cells(), case_row_and_column_same_mark()]
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# The gather of a tile's first row / column / corner cell: which of the four writers (the tile itself, its left, lower and diagonal
# neighbour) the reference's serial tile order leaves standing.  Every combination of present writers, with four sign patterns.
GATHER_SIGNS = [(1, -1, 1, -1), (-1, 1, -1, 1), (1, 1, -1, -1), (-1, -1, 1, 1)]      # (own, left, down, diagonal)


def gather_steps():
    """[(TileGrid, present (own, left, down, diag, own_empty), signs)]: the 2 x 2 inner tiles of a 128 x 128 map; the upper right
    one is `own`.  The neighbours' halo copies hold THEIR sign, whatever own holds: inconsistent on purpose."""
    steps = []
    for mask in range(16):
        for signs in GATHER_SIGNS:
            present = tuple(bool(mask >> k & 1) for k in range(4))
            for own_empty in ((False, True) if not present[0] else (False,)):
                g = TileGrid(7)
                for k, (X, Y) in enumerate(((2, 2), (1, 2), (2, 1), (1, 1))):
                    if present[k]:
                        g.init_tile(g.tile(X, Y), fill=0.5 * signs[k])
                if own_empty:
                    g.empty_tile(g.tile(2, 2), 2.0)
                steps.append((g, present + (own_empty,), signs))
    return steps


def gather_expected_corner(present, signs, before):
    """the map cell (64, 64) by the serial order diag, down, left, own (y outer, x inner): the last present writer's sign"""
    own, left, down, diag, own_empty = present
    v = before
    for k in (3, 2, 1, 0):
        if present[k]:
            v = 0 if signs[k] > 0 else -1
    if own_empty:
        v = 0
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# The reuse sequence: one context, its persistent map and its work list from call to call.
SEQ_LOG2, SEQ_CS = 9, 0.05


def dense_grid():
    g = TileGrid(SEQ_LOG2)
    fn = lambda gx, gy: np.clip(np.sin(gx * 0.045) * np.cos(gy * 0.038) + 0.25, -1.0, 1.0)
    return g.fill_from(fn, _inner(g) + [g.tile(0, 3), g.tile(5, 0), g.tile(g.PX - 1, 7)])


def sparse_grid():
    g = TileGrid(SEQ_LOG2)
    fn = lambda gx, gy: np.clip(np.cos(gx * 0.09 + 1.0) * np.sin(gy * 0.075) - 0.1, -1.0, 1.0)
    g.fill_from(fn, [g.tile(1, 1), g.tile(2, 1), g.tile(9, 6), g.tile(14, 14), g.tile(3, 12)])
    return g.empty_tile(g.tile(8, 8), 2.0)


# (action, inflate, factor): the call after step k is occupancy / occupancy_into / map_frame for k % 3 == 0 / 1 / 2
SEQUENCE = [
    ("dense", False, 2),
    ("sparse", True, 2),         # the grid shrinks: 196 listed tiles -> 5
    ("none", True, 2),           # unchanged grid, same parameters: the identical map
    ("dense", True, 3),
    ("reset", False, 2),         # dense -> reset -> call -> call
    ("none", False, 2),
    ("push", True, 2),
    ("load_text", False, 2),     # the sparse grid as stored after step 1 (its halos are not in the file)
    ("push", True, 3),
    ("dense", True, 1),
    ("sparse", False, 0),
    ("reset", True, 33),
    ("push", True, 2),
    ("none", False, 2),
]


class SequenceReach:
    """what the reuse sequence has to have gone through, from the restatement's own figures"""

    def __init__(self, ref: MapRef):
        self.ref = ref
        self.steps = []

    def record(self, k, action, inflate, factor, init, content_before, occ, n):
        self.steps.append(dict(k=k, action=action, params=(inflate, factor), listed=listed_tiles(SEQ_LOG2, init), before=content_before,
                               after=self.ref.content.copy(), occ=occ.copy(), n=n))

    def assert_reached(self):
        s = self.steps
        assert len(s) >= 8 and {x["action"] for x in s} == {"dense", "sparse", "none", "reset", "push", "load_text"}
        shrinks = [(a["listed"], b["listed"]) for a, b in zip(s, s[1:]) if b["listed"] < a["listed"]]
        assert any(a >= 100 and 0 < b <= 8 for a, b in shrinks), f"the work list never shrank to a few tiles: {shrinks}"
        assert any(b == 0 for _, b in shrinks), "no call on an empty grid behind a full one"
        same = [(a, b) for a, b in zip(s, s[1:]) if b["action"] == "none" and a["params"] == b["params"]]
        assert len(same) >= 2
        for a, b in same:
            assert a["n"] == b["n"] and np.array_equal(a["occ"], b["occ"]) and np.array_equal(a["after"], b["after"]), f"step {b['k']}"
        resets = [(a, b) for a, b in zip(s, s[1:]) if b["action"] == "reset"]
        assert resets
        for a, b in resets:
            # ThreadGrid never clears _occGridContent and TsdGrid::reset does not touch it: the map of an emptied grid is the
            # persistent map as the last extraction left it, without a single mark
            assert b["listed"] == 0 and b["n"] == 0
            assert np.array_equal(b["after"], a["after"]) and np.array_equal(b["occ"].reshape(-1), a["after"])
            assert (a["after"] == 0).sum() > 1000, "nothing in the persistent map that a reset could have wiped"
            assert a["n"] > 0 and (a["occ"] == 100).any() and not (b["occ"] == 100).any()
        assert any(a["action"] == "dense" and b["action"] == "reset" and c["action"] == "none" for a, b, c in zip(s, s[1:], s[2:]))
        assert any(x["action"] == "push" and x["n"] > 0 for x in s) and any(x["action"] == "load_text" and x["n"] > 0 for x in s)
