"""The frontier rules' restatement (tests/frontier_ref.py) against a second, independent derivation -- label propagation to a fixed
point -- and against hand-drawn maps whose answers are written out here; the ABI's record size through the library."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import frontier_ref as F

NONE = F.NONE
U, O = -1, 100          # unknown, obstacle; 0 = free


def _propagate(mask, diagonals):
    """label = min over the neighbourhood, iterated to a fixed point: each component ends at its smallest linear index"""
    H, W = mask.shape
    big = np.uint64(1) << np.uint64(40)
    lab = np.where(mask, np.arange(H * W, dtype=np.uint64).reshape(H, W), big)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        best = lab.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx or dy) and (diagonals or dx == 0 or dy == 0):
                    best = np.minimum(best, p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        best = np.where(mask, best, big)
        if np.array_equal(best, lab):
            break
        lab = best
    return np.where(mask, lab, NONE).astype(np.uint32)


def _frontier_cells_by_loops(m, free_max):
    H, W = m.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            if not 0 <= m[y, x] <= free_max:
                continue
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < W and 0 <= y + dy < H and m[y + dy, x + dx] < 0:
                    out[y, x] = True
    return out


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (9, 1), (5, 8), (24, 24), (17, 23)])
@pytest.mark.parametrize("p_unknown", [0.1, 0.5, 0.9])
def test_restatement_equals_label_propagation(shape, p_unknown):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + int(p_unknown * 10))
    H, W = shape
    for free_max in (0, 40):
        m = rng.choice(np.array([U, 0, 30, O], dtype=np.int8), size=(H, W), p=[p_unknown] + [(1 - p_unknown) / 3] * 3)
        cells = _frontier_cells_by_loops(m, free_max)
        assert np.array_equal(F.frontier_cells(m, free_max), cells)
        lab = _propagate(cells, True)
        reg = _propagate((m >= 0) & (m <= free_max), False)
        assert np.array_equal(F.components(cells, F.N8), lab)
        assert np.array_equal(F.components(F.traversable(m, free_max), F.N4), reg)
        seeds = [(int(rng.integers(-1, W + 1)), int(rng.integers(-1, H + 1))) for _ in range(3)]
        rec, lab2, used = F.frontiers(m, free_max, 1, seeds)
        assert np.array_equal(lab2, lab)
        good = [(x, y) for x, y in seeds if 0 <= x < W and 0 <= y < H and 0 <= m[y, x] <= free_max]
        assert used == len(good)
        roots = np.unique(lab[lab != NONE])
        assert np.array_equal(rec["root_y"].astype(np.int64) * W + rec["root_x"], roots)
        for r in rec:
            ys, xs = np.nonzero(lab == r["root_y"] * W + r["root_x"])
            assert (r["size"], r["sum_x"], r["sum_y"]) == (xs.size, xs.sum(), ys.sum())
            assert (r["min_x"], r["min_y"], r["max_x"], r["max_y"]) == (xs.min(), ys.min(), xs.max(), ys.max())
            assert r["reachable"] == int(any(reg[y, x] == reg[sy, sx] for y, x in zip(ys, xs) for sx, sy in good))


def _map(rows):
    return np.array(rows, dtype=np.int8)


def test_diagonal_chain_is_one_frontier_but_two_regions():
    m = _map([[0, U, O],
              [U, 0, U],
              [O, U, O]])
    rec, lab, used = F.frontiers(m, seeds=[(0, 0)])
    assert lab.tolist() == [[0, NONE, NONE], [NONE, 0, NONE], [NONE, NONE, NONE]]
    assert rec.tolist() == [(0, 0, 2, 1, 1, 1, 0, 0, 1, 1)] and used == 1
    reg = F.components(F.traversable(m), F.N4)
    assert reg[0, 0] == 0 and reg[1, 1] == 4                      # the diagonal is no passage
    # a frontier is reachable through ANY of its cells: from (1, 1) as well
    assert F.frontiers(m, seeds=[(1, 1)])[0]["reachable"].tolist() == [1]


def test_the_border_is_not_unknown():
    m = np.zeros((4, 5), dtype=np.int8)
    rec, lab, _ = F.frontiers(m)
    assert rec.size == 0 and np.all(lab == NONE)
    m[0, 4] = U
    rec, lab, _ = F.frontiers(m)
    assert sorted(zip(*np.nonzero(lab != NONE))) == [(0, 3), (1, 4)]          # the two edge neighbours, united by the diagonal
    assert rec.tolist() == [(3, 0, 2, -1, 7, 1, 3, 0, 4, 1)]


def test_free_max_step():
    m = _map([[U, 30, 0, 31, U]])
    assert F.frontiers(m, free_max=0)[0].size == 0                            # (0 has no unknown neighbour)
    assert F.frontiers(m, free_max=30)[0].tolist() == [(1, 0, 1, -1, 1, 0, 1, 0, 1, 0)]
    assert F.frontiers(m, free_max=31)[0]["root_x"].tolist() == [1, 3]
    assert F.frontiers(_map([[U, 100, U]]), free_max=99)[0].size == 0


def test_a_seed_on_an_obstacle_is_ignored():
    m = _map([[U, 0, 0, O, 0, U]])
    seeds = [(3, 0), (0, 0), (6, 0), (2, -1)]                                 # obstacle, unknown, outside, outside
    rec, _, used = F.frontiers(m, seeds=seeds)
    assert used == 0 and rec["reachable"].tolist() == [0, 0]
    rec, _, used = F.frontiers(m, seeds=seeds + [(2, 0)])
    assert used == 1 and rec["reachable"].tolist() == [1, 0]
    assert F.frontiers(m)[0]["reachable"].tolist() == [-1, -1]


def test_min_size_drops_records_but_not_labels_and_the_order():
    m = _map([[U, U, U, U, U, U, U],
              [0, 0, 0, O, 0, O, 0],
              [O, O, O, O, O, O, O],
              [0, 0, O, U, U, U, U],
              [U, U, O, 0, 0, 0, 0]])
    rec, lab, _ = F.frontiers(m)
    # ascending root index: (0,1) size 3, (4,1) size 1, (6,1) size 1, (0,3) size 2, (3,4) size 4
    assert list(zip(rec["root_x"].tolist(), rec["root_y"].tolist(), rec["size"].tolist())) == \
        [(0, 1, 3), (4, 1, 1), (6, 1, 1), (0, 3, 2), (3, 4, 4)]
    rec3, lab3, _ = F.frontiers(m, min_size=3)
    assert list(zip(rec3["root_x"].tolist(), rec3["root_y"].tolist(), rec3["size"].tolist())) == [(0, 1, 3), (3, 4, 4)]
    assert np.array_equal(lab3, lab) and lab[1, 4] == 1 * 7 + 4


def test_abi_of_the_frontier_calls(hip_lib):
    for name in ("tsd_frontiers_dev", "tsd_frontiers_frame", "tsd_frontiers_fetch", "tsd_frontiers_dev_ptrs"):
        assert hasattr(hip_lib, name) and name in capi.ABI, name
    assert hip_lib.tsd_abi_sizeof(b"tsd_frontier") == C.sizeof(capi.Frontier) == 48
    assert hip_lib.tsd_abi_sizeof(b"tsd_frontier_params") == C.sizeof(capi.FrontierParams) == 24
    assert capi.FRONTIER_DTYPE == F.DTYPE and capi.Frontier.sum_x.offset == 16 and capi.Frontier.min_x.offset == 32
