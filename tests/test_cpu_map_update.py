"""The rule of the windowed map update (tsd_map_update_begin), checked on the numpy restatement of tests/map_update_ref.py
without a GPU: two grids that differ only inside a tile box D give full frames that differ only inside U = D grown by g tiles, and
"cells in U, marks from U'" applied to the old frame gives the new frame exactly.  Every comparison is exact.
"""
import numpy as np
import pytest

from tests import map_edges_ref as R
from tests import map_update_ref as W

CS = 0.05


def _random_tiles(rng, grid, tiles, p_init=0.5, p_empty=0.15, p_neg=0.003):
    """tiles with a few sign changes each (positive cells, a few negative ones, some NaN: at factor 31 a denser grid would be marked
    all over), some empty, some untouched; the halos are independent of the neighbours' edge cells, which is harder on the last-writer
    rule than consistent ones"""
    for p in tiles:
        r = rng.random()
        grid.init[p], grid.iw[p] = 0, 0.0
        grid.tsd[p, :] = np.nan
        if r < p_init:
            v = np.where(rng.random(R.TC) < p_neg, -rng.uniform(0.05, 1.0, R.TC), rng.uniform(0.05, 1.0, R.TC))
            v[rng.random(R.TC) < 0.02] = np.nan
            grid.init[p] = 1
            grid.tsd[p, :] = v
        elif r < p_init + p_empty:
            grid.iw[p] = 1.0


def _boxes(PX):
    """D touching the outer ring, in a corner, a single interior tile, and a box in the middle"""
    return {"ring": (0, 2, 1, 3), "corner": (PX - 2, PX - 2, PX - 1, PX - 1), "single": (PX // 2, PX // 2 - 1, PX // 2, PX // 2 - 1),
            "middle": (1, 1, 2, 3), "right_edge": (PX - 2, 1, PX - 2, 1)}


def _pair(log2, box, seed):
    """(old grid, new grid): random tile grids that differ only inside `box`"""
    rng = np.random.default_rng(seed)
    old = R.TileGrid(log2)
    _random_tiles(rng, old, range(old.PX * old.PX))
    new = R.TileGrid(log2)
    new.init[:], new.iw[:], new.tsd[:] = old.init, old.iw, old.tsd
    inside = [p for p in range(old.PX * old.PX) if W.tile_in(p, box, old.PX)]
    _random_tiles(rng, new, inside, p_init=1.0)         # (every tile of D changes)
    return old, new


PARAMS = [(False, 0), (True, 1), (True, 2), (True, 5), (True, 31)]
_frames = {}


def _frames_of(log2, name, inflate, factor):
    """old frame, then the full frame of the new grid on the same persistent map; computed once per case and left unchanged"""
    key = (log2, name, inflate, factor)
    if key not in _frames:
        PX = (1 << log2) // R.D
        box = _boxes(PX)[name]
        old, new = _pair(log2, box, seed=1000 * log2 + sorted(_boxes(PX)).index(name))
        ref = R.MapRef(log2, CS)
        old_map, _, _, sp0 = W.full_frame(ref, old.init, old.iw, old.tsd, inflate, factor)
        old_content = ref.content.copy()
        new_map, coords, events, sp1 = W.full_frame(ref, new.init, new.iw, new.tsd, inflate, factor)
        for a in (old_map, old_content, new_map):
            a.setflags(write=False)
        _frames[key] = dict(box=box, PX=PX, old_map=old_map, old_content=old_content, new_map=new_map, new_content=ref.content.copy(),
                            coords=coords, events=events, spilled=sp0 + sp1)
    return _frames[key]


def test_fast_marking_equals_the_restatement_of_map_edges_ref():
    """W.mark is MapRef.occupancy's marking loop in numpy slices: same map, wrapping bounds and spills included"""
    old, _ = _pair(7, (1, 1, 2, 2), seed=3)
    edge, _ = _right_edge_mark(7)
    for grid, inflate, factor in [(old, False, 0), (old, True, 1), (old, True, 5), (old, True, 33), (edge, True, 33), (edge, True, 40)]:
        a, b = R.MapRef(7, CS), R.MapRef(7, CS)
        want, n, info = a.occupancy(grid.init, grid.iw, grid.tsd, inflate, factor)
        got, coords, _, spilled = W.full_frame(b, grid.init, grid.iw, grid.tsd, inflate, factor)
        assert n == len(coords) and n > (20 if grid is old else 0)
        assert np.array_equal(got, want), (inflate, factor)
        assert spilled == info["spilled"], (inflate, factor)
        assert grid is old or spilled > 0


@pytest.mark.parametrize("inflate,factor", PARAMS)
@pytest.mark.parametrize("name", ["ring", "corner", "single", "middle", "right_edge"])
@pytest.mark.parametrize("log2", [7, 8])
def test_frames_differ_only_inside_U(log2, name, inflate, factor):
    f = _frames_of(log2, name, inflate, factor)
    u, _ = W.windows(f["box"], inflate, factor, f["PX"])
    rows, cols = W.cells_of(u)
    diff = f["old_map"] != f["new_map"]
    cdiff = (f["old_content"] != f["new_content"]).reshape(diff.shape)
    # (at factor 31 the marks around a single tile can cover its whole neighbourhood before and after: the persistent map still changes)
    assert diff.any() or cdiff.any(), "the two grids give the same maps: the case shows nothing"
    outside = diff.copy()
    outside[rows, cols] = False
    assert not outside.any(), f"{np.count_nonzero(outside)} cells differ outside U = {u}: {np.argwhere(outside)[:5]}"
    cdiff[rows, cols] = False
    assert not cdiff.any(), "the persistent map changed outside U"
    assert f["spilled"] == 0          # (factor <= 31: no mark reaches past its row's end)


@pytest.mark.parametrize("inflate,factor", PARAMS)
@pytest.mark.parametrize("name", ["ring", "corner", "single", "middle", "right_edge"])
@pytest.mark.parametrize("log2", [7, 8])
def test_cells_in_U_marks_from_U2_give_the_new_frame(log2, name, inflate, factor):
    f = _frames_of(log2, name, inflate, factor)
    content, staged = W.windowed_update(f["old_content"], f["old_map"], f["new_content"], f["coords"], f["events"], f["box"],
                                        inflate, factor, f["PX"], CS)
    assert np.array_equal(staged, f["new_map"]), f"{np.count_nonzero(staged != f['new_map'])} cells differ"
    assert np.array_equal(content.reshape(-1), f["new_content"])


def _right_edge_mark(log2):
    """one sign change in the last scanned tile column, in the tile's halo column: the mark with the largest u there is, N - 32"""
    g = R.TileGrid(log2)
    p = g.tile(g.PX - 2, 2)
    g.init_tile(p, fill=0.5)
    g.set_local(p, 16, R.D, -0.5)                # row scan at (16, 32): prev > 0, cur < 0
    return g, p


@pytest.mark.parametrize("factor,spills", [(31, False), (32, False), (33, True)])
def test_spill_at_the_right_edge_leaves_the_window(factor, spills):
    """Why a large factor takes a full frame.  The marking loop's column index is not clipped: with u + factor > N the square's last
    columns land in the NEXT row's first cells, at the other side of the map.  The largest u a scanned tile can mark is N - 32 (tile
    column PX - 2, halo column), so the spill starts at factor 33: the old and the new frame then differ in columns 0 .. factor - 33,
    far outside U whatever the growth.  At factor 32 the square ends in column N - 1 exactly and nothing spills: measured here, one
    tile changed at the right edge of a 256 x 256 map, cells that differ outside U: factor 31: 0, factor 32: 0, factor 33: 67, all in column 0.
    The device's bound (full frame for factor > 31) is therefore conservative by one factor."""
    log2 = 8
    new, p = _right_edge_mark(log2)
    old = R.TileGrid(log2)
    old.init_tile(p, fill=0.5)
    PX, N = old.PX, old.N
    box = (PX - 2, 2, PX - 2, 2)
    ref = R.MapRef(log2, CS)
    old_map, _, _, _ = W.full_frame(ref, old.init, old.iw, old.tsd, True, factor)
    new_map, coords, events, spilled = W.full_frame(ref, new.init, new.iw, new.tsd, True, factor)
    want, _, info = R.MapRef(log2, CS).occupancy(new.init, new.iw, new.tsd, True, factor)
    assert np.array_equal(new_map, want) and info["marks"] and max(u for u, _ in info["marks"]) == N - R.D
    u, _ = W.windows(box, True, factor, PX)
    rows, cols = W.cells_of(u)
    outside = old_map != new_map
    outside[rows, cols] = False
    print(f"factor {factor}: growth {W.growth(True, factor)}, U {u}, spilled writes {spilled}, cells that differ outside U "
          f"{np.count_nonzero(outside)}, their columns {sorted(set(np.argwhere(outside)[:, 1].tolist()))}")
    assert (spilled > 0) == spills
    assert outside.any() == spills
    if spills:
        assert set(np.argwhere(outside)[:, 1].tolist()) == set(range(factor - 32))      # the far side of the map
