"""The route rule's restatement (tests/route_ref.py) against what it must equal on the CPU: a heap Dijkstra over (cost, seed index)
on every map the GPU test uses, the closed form on open maps, the regions of tests/frontier_ref.py, the step equation along every
traced path; and the host parts of the library -- tsd_route_weights against its formula, its refusals, the struct sizes."""
import ctypes as C
import heapq

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import frontier_ref as F
from tests import route_ref as R

CASES = R.cases()
IDS = [c[0] for c in CASES]


def dijkstra(m, seeds, free_max=0, w=None, limit=0):
    """keys by a heap over (d << 4) | i: the textbook algorithm, one pop per settled cell"""
    H, W = m.shape
    wi = R.weight_image(m, free_max, w)
    mv = R.moves(wi)
    lim_key = ((limit or R.MAX_DIST) << 4) | 15
    key = {}
    heap = []
    for i, (x, y) in enumerate(seeds):
        if 0 <= x < W and 0 <= y < H and wi[y, x] > 0 and i < key.get((x, y), 1 << 60):
            key[(x, y)] = i
            heapq.heappush(heap, (i, x, y))
    while heap:
        k, x, y = heapq.heappop(heap)
        if k != key[(x, y)]:
            continue
        for n, (dx, dy) in enumerate(R.OFFS):
            bx, by = x - dx, y - dy                  # (x, y) is neighbour n of b
            if not (0 <= bx < W and 0 <= by < H and mv[n, by, bx]):
                continue
            cand = k + ((R.COST[n] * int(wi[by, bx])) << 4)
            if cand <= lim_key and cand < key.get((bx, by), 1 << 60):
                key[(bx, by)] = cand
                heapq.heappush(heap, (cand, bx, by))
    out = np.full((H, W), R.NONE, dtype=np.uint32)
    for (x, y), k in key.items():
        out[y, x] = k
    return out


@pytest.fixture(scope="module")
def fields():
    """the restatement's result per case, computed once"""
    return {name: R.route(src, p["seeds"], p["free_max"], p["w"], p["limit"]) for name, src, _, p in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_dijkstra(fields, case):
    name, src, _, p = case
    keys, used = fields[name]
    want = dijkstra(src, p["seeds"], p["free_max"], p["w"], p["limit"])
    assert np.array_equal(keys, want), f"{np.count_nonzero(keys != want)} keys differ at {np.argwhere(keys != want)[:4]}"
    assert used == len(F.used_seeds(src, p["free_max"], p["seeds"]))


@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("open_")], ids=lambda c: c[0])
def test_open_map_closed_form(fields, case):
    name, src, _, p = case
    H, W = src.shape
    (sx, sy), = p["seeds"]
    dx, dy = np.abs(np.arange(W)[None, :] - sx), np.abs(np.arange(H)[:, None] - sy)
    want = 7 * np.minimum(dx, dy) + 5 * np.abs(dx - dy)
    assert np.array_equal(fields[name][0], (want << 4).astype(np.uint32))


@pytest.mark.parametrize("case", [c for c in CASES if c[3]["limit"] == 0], ids=lambda c: c[0])
def test_keys_cover_exactly_the_seeds_regions(fields, case):
    name, src, _, p = case
    reg = F.components(F.traversable(src, p["free_max"]), F.N4)
    roots = {int(reg[y, x]) for x, y in F.used_seeds(src, p["free_max"], p["seeds"])}
    want = np.isin(reg, np.array(sorted(roots), dtype=np.uint32)) & (reg != F.NONE)
    assert np.array_equal(fields[name][0] != R.NONE, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_traced_paths_obey_the_step_equation(fields, case):
    name, src, _, p = case
    keys, _ = fields[name]
    H, W = src.shape
    wi = R.weight_image(src, p["free_max"], p["w"])
    reached = np.nonzero(keys.ravel() != R.NONE)[0]
    assert reached.size > 0, "the case has no used seed"
    rng = np.random.default_rng(3)
    picks = [int(c) for c in rng.choice(reached, size=min(24, reached.size), replace=False)] + [int(reached[np.argmax(keys.ravel()[reached] >> 4)])]
    paths, lens = R.trace(keys, wi, picks, W * H)
    seed_cells = {y * W + x for x, y in F.used_seeds(src, p["free_max"], p["seeds"])}
    for path, n in zip(paths, lens):
        assert n == len(path) >= 1 and path[-1] in seed_cells and keys.ravel()[path[-1]] >> 4 == 0
        for b, a in zip(path[:-1], path[1:]):
            ddx, ddy = b % W - a % W, b // W - a // W
            assert max(abs(ddx), abs(ddy)) == 1
            c = 7 if ddx and ddy else 5
            assert int(keys.ravel()[a]) + ((c * int(wi.ravel()[b])) << 4) == int(keys.ravel()[b])
            if ddx and ddy:
                assert wi[b // W, a % W] > 0 and wi[a // W, b % W] > 0
    # a goal without a key, a goal outside the map
    _, lens = R.trace(keys, wi, [W * H, W * H + 7], 4)
    assert lens.tolist() == [0, 0]


def test_named_cells_of_the_drawn_maps(fields):
    """what the drawn maps are drawn for, from the restatement (which the device must equal)"""
    d = lambda name, x, y: int(fields[name][0][y, x]) >> 4 if fields[name][0][y, x] != R.NONE else None
    i = lambda name, x, y: int(fields[name][0][y, x]) & 15
    for name in IDS:
        if name.startswith("corner_"):            # the room across the diagonal is not entered
            keys = fields[name][0]
            anti = "antidiagonal" in name
            assert (keys[:32, (33 if anti else 32):] == R.NONE).all() and (keys[32:, (32 if anti else 33):] == R.NONE).all()
            assert keys[31, 31 if anti else 30] != R.NONE and keys[32, 30 if anti else 31] != R.NONE
    # (the gap is entered straight from (31, 40): the diagonal from (31, 39) would cut the wall)
    assert d("seam_wall_one_gap_64x64", 32, 40) == 7 * 26 + 5 * 9 + 5 and d("seam_wall_one_gap_64x64", 40, 5) is not None
    assert [i("equidistant_column", 16, y) for y in (0, 16, 32)] == [0, 0, 0] and i("equidistant_column", 15, 16) == 1
    assert d("equidistant_column", 16, 16) == 60 and i("equidistant_column", 17, 16) == 0
    assert fields["two_seeds_one_cell"][0][10, 10] == 0 and i("two_seeds_one_cell", 11, 10) == 0 and i("two_seeds_one_cell", 20, 20) == 2
    keys, used = fields["seeds_ignored"]
    assert used == 1 and ((keys[keys != R.NONE] & 15) == 5).all() and keys[3, 3] == R.NONE and keys[4, 4] == R.NONE
    assert fields["sixteen_seeds"][1] == 16 and len(set((fields["sixteen_seeds"][0][fields["sixteen_seeds"][0] != R.NONE] & 15).tolist())) > 8
    assert d("limit_100", 20, 0) == 100 and d("limit_100", 21, 0) is None and d("limit_100", 0, 20) == 100 and d("limit_100", 0, 21) is None
    assert d("limit_100", 14, 1) == 72 and d("limit_100", 14, 14) == 98 and d("limit_100", 15, 15) is None
    assert d("weights_255_1x300", 0, 299) == 381225
    # the detour through the free gap at y = 120 is cheaper than the three band cells at weight 130
    W = 97
    wi = R.weight_image(CASES[IDS.index("cost_band")][1], 50, R.weights(50, 255))
    (path,), _ = R.trace(fields["cost_band"][0], wi, [21 * W + 80], 10 ** 6)
    assert any(c // W == 120 for c in path) and not any(20 <= c // W <= 22 and 47 <= c % W < 50 for c in path)
    assert d("cost_band", 80, 21) < 5 * (70 - 3) + 3 * 5 * 130
    # the sweep over densities is not vacuous
    name = "random_0.05_97x130"
    src, p = CASES[IDS.index(name)][1], CASES[IDS.index(name)][3]
    assert np.count_nonzero(fields[name][0] != R.NONE) > 0.5 * np.count_nonzero(F.traversable(src, p["free_max"]))


def test_goals_are_the_minimum_over_a_frontiers_cells():
    """two frontier cells of one frontier at the same cost: the smaller index; a frontier without a key: none"""
    src = np.zeros((9, 40), dtype=np.int8)
    src[:, 0] = R.U                         # the frontier: column 1
    src[:, 30] = R.O
    src[:, 39] = R.U                        # a second frontier behind the wall: column 38
    rec, lab, _ = F.frontiers(src)
    keys, _ = R.route(src, [(11, 4)])
    g = R.goals(keys, lab, rec)
    assert g["cell"].tolist() == [4 * 40 + 1, R.NONE] and g["dist"].tolist() == [50, R.NONE] and g["seed"].tolist() == [0, -1]
    keys, _ = R.route(src, [(1, 2), (1, 6)])             # both on the frontier at d = 0: the smaller cell, whose key carries seed 0
    g = R.goals(keys, lab, rec)
    assert (g["cell"][0], g["dist"][0], g["seed"][0]) == (2 * 40 + 1, 0, 0)


# ---- the host parts of the library
def test_route_weights_through_the_library(hip_lib):
    _u8p = C.POINTER(C.c_uint8)
    for free_max in (0, 1, 50, 98, 99):
        for max_weight in (1, 2, 98, 99, 200, 255):
            t = np.full(free_max + 2, 0xEE, dtype=np.uint8)
            assert hip_lib.tsd_route_weights(free_max, max_weight, t.ctypes.data_as(_u8p)) == 0
            assert np.array_equal(t[:-1], R.weights(free_max, max_weight)) and t[-1] == 0xEE
            assert np.array_equal(capi.route_weights(free_max, max_weight), t[:-1])
    assert R.weights(98, 255)[98] == 255 and R.weights(99, 255)[0] == 1
    t = np.zeros(128, dtype=np.uint8)
    for free_max, max_weight in ((-1, 1), (100, 1), (0, 0), (0, 256), (0, -3)):
        assert hip_lib.tsd_route_weights(free_max, max_weight, t.ctypes.data_as(_u8p)) == -1, (free_max, max_weight)
    assert hip_lib.tsd_route_weights(0, 1, None) == -1
    with pytest.raises(capi.TsdError):
        capi.route_weights(0, 256)


def test_struct_sizes(hip_lib):
    assert hip_lib.tsd_abi_sizeof(b"tsd_route_params") == C.sizeof(capi.RouteParams) == 2 * 4 + 2 * 8 + 2 * 4
    assert hip_lib.tsd_abi_sizeof(b"tsd_route_info") == C.sizeof(capi.RouteInfo) == 16
    assert hip_lib.tsd_abi_sizeof(b"tsd_route_goal") == C.sizeof(capi.RouteGoal) == capi.ROUTE_GOAL_DTYPE.itemsize == 16
    assert capi.ROUTE_GOAL_DTYPE == R.GOAL_DTYPE and capi.ROUTE_NONE == R.NONE and capi.ROUTE_MAX_DIST == R.MAX_DIST
