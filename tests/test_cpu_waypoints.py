"""The waypoint rule without a GPU: the restatement of tests/waypoint_ref.py (what the device is compared with, byte for byte, in
tests/test_gpu_waypoints.py) against an independent rasteriser of the line, the invariants the rule promises on a converged key
image, the properties of a waypoint list, the named numbers of the free room and of a cluttered map, the diagonal rule against the
views'; the ABI's struct sizes and symbol."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import route_ref as R
from tests import view_ref as V
from tests import waypoint_ref as WP

CASES = R.cases()
IDS = [c[0] for c in CASES]
MAX_LEN = 1 << 20


def sgn(a):
    return (a > 0) - (a < 0)


def half_up(fr):
    """the integer nearest to a non-negative fraction, a half rounded up"""
    n, d = fr.numerator, fr.denominator
    return (2 * n + d) // (2 * d)


def raster(p, q):
    """the line by exact arithmetic: at step j the major axis stands at j, the minor one at j * |d_minor| / N rounded half up"""
    dx, dy = q[0] - p[0], q[1] - p[1]
    N = max(abs(dx), abs(dy))
    return [(p[0] + sgn(dx) * half_up(Fraction(j * abs(dx), N)), p[1] + sgn(dy) * half_up(Fraction(j * abs(dy), N))) for j in range(1, N + 1)]


# ---- the closed form
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1024])
def test_line_closed_form(N):
    minors = sorted({0, 1, N // 3, N // 2, (N + 1) // 2, N - 1, N})        # the axes, shallow and steep lines, the exact diagonal
    p = (2000, 3000)
    seen = set()
    for m in minors:
        for a, b in ((N, m), (m, N)):
            for sx in (1, -1):
                for sy in (1, -1):
                    d = (sx * a, sy * b)
                    if d in seen:
                        continue
                    seen.add(d)
                    q = (p[0] + d[0], p[1] + d[1])
                    cells = WP.line(p, q)
                    assert cells == raster(p, q), (N, d)
                    assert len(cells) == N and cells[-1] == q
                    prev = p
                    for c in cells:
                        assert max(abs(c[0] - prev[0]), abs(c[1] - prev[1])) == 1                    # a neighbour step, never none
                        assert min(p[0], q[0]) <= c[0] <= max(p[0], q[0]) and min(p[1], q[1]) <= c[1] <= max(p[1], q[1])
                        prev = c
    # all eight octants and the four axis directions were among them
    assert len({(sgn(a), sgn(b), abs(a) >= abs(b)) for a, b in seen}) >= (8 if N > 1 else 6)


def test_the_kernels_division_by_a_reciprocal():
    """csrc/waypoint.hip divides by 2N with (n * r) >> 33, r = min(ceil(2^33 / 2N), 2^32 - 1) from a table: exact for every numerator
    2 s m + N of the rule, s and m in 0 .. N, at every N the look-ahead allows"""
    for N in range(1, WP.MAX_LOOKAHEAD + 1):
        r = min(-(-(1 << 33) // (2 * N)), (1 << 32) - 1)
        s = np.arange(N + 1, dtype=np.uint64)
        n = 2 * s[:, None] * s[None, :] + np.uint64(N)
        assert int(n.max()) * r < 1 << 64
        assert np.array_equal((n * np.uint64(r)) >> np.uint64(33), n // np.uint64(2 * N)), N


# ---- the invariants and the properties, on the routes' maps
def _goals(keys, seed=3, n=6):
    flat = keys.ravel()
    reached = np.nonzero(flat != R.NONE)[0]
    far = reached[np.argsort(flat[reached], kind="stable")[-3:]]
    rnd = np.random.default_rng(seed).choice(reached, size=min(n, reached.size), replace=False)
    return [int(c) for c in far] + [int(c) for c in rnd] + [int(reached[np.argmin(flat[reached])]), flat.size + 1]


def _props(keys, wi, cells, lookahead, slack, what, seeds=None):
    """what every waypoint list has; the lists and records"""
    H, W = keys.shape
    ways, info = WP.waypoints(keys, wi, cells, lookahead, slack, MAX_LEN)
    paths, lens = R.trace(keys, wi, cells, MAX_LEN)
    assert np.array_equal(info["len"], lens)
    for g, (way, rec) in enumerate(zip(ways, info)):
        if rec["len"] <= 0:
            assert rec["n_way"] == 0 and way.size == 0 and rec["cost"] == 0
            continue
        assert rec["n_way"] == way.size >= 1 and way[-1] == cells[g] and way[0] == paths[g][-1]
        assert int(keys.ravel()[way[0]]) >> 4 == 0 and rec["dist"] == int(keys.ravel()[cells[g]]) >> 4
        if seeds is not None:                                  # the first waypoint is the cell of the seed the goal's key names
            sx, sy = seeds[int(keys.ravel()[cells[g]]) & 15]
            assert way[0] == sy * W + sx, (what, g)
        # the waypoints are cells of the path, in driving order, at most `lookahead` path cells apart
        at = [paths[g][::-1].index(int(c)) for c in way]
        assert at[0] == 0 and all(0 < b - a <= lookahead for a, b in zip(at, at[1:]))
        total = 0
        for a, b in zip(way, way[1:]):
            pa, pb = (int(a) % W, int(a) // W), (int(b) % W, int(b) // W)
            ok, c = WP.segment(wi, pa, pb)
            d_ab = (int(keys.ravel()[b]) >> 4) - (int(keys.ravel()[a]) >> 4)
            assert ok and d_ab <= c <= d_ab + slack, (what, g, pa, pb, c, d_ab)       # (never cheaper than the field: a converged image)
            total += c
        assert total == rec["cost"] and rec["dist"] <= total <= rec["dist"] + (way.size - 1) * slack, (what, g)
    return ways, info


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invariants(case):
    name, src, _, p = case
    rng = np.random.default_rng(len(name))
    for unit in (True, False):
        w = None if unit else (p["w"] if p["w"] is not None else rng.integers(1, 256, size=p["free_max"] + 1).astype(np.uint8))
        keys, _ = R.route(src, p["seeds"], p["free_max"], w, p["limit"])
        wi = R.weight_image(src, p["free_max"], w)
        cells = _goals(keys)
        for lookahead, slack in ((8, 0), (128, 0), (128, 200), (128, 1 << 20)):
            ways, info = _props(keys, wi, cells, lookahead, slack, name, p["seeds"])
            has = info["len"] > 0
            if slack == 0 or unit:
                assert (info["cost"][has] == info["dist"][has]).all(), (name, unit, lookahead, slack)      # every segment an equally cheap way
        # lookahead 1: the trace, reversed
        ways, info = WP.waypoints(keys, wi, cells, 1, 0, MAX_LEN)
        paths, _ = R.trace(keys, wi, cells, MAX_LEN)
        assert [w_.tolist() for w_ in ways] == [path[::-1] for path in paths]
        # a path longer than max_len is not straightened; its length is reported in full
        cut, cinfo = WP.waypoints(keys, wi, cells, 8, 0, 2)
        assert np.array_equal(cinfo["len"], info["len"]) and (cinfo["n_way"][info["len"] > 2] == 0).all()
        assert all(c.tolist() == w_.tolist() for c, w_, n in zip(cut, ways, info["len"]) if 0 < n <= 2)


# ---- named numbers
def test_the_free_room():
    src = np.zeros((64, 96), dtype=np.int8)
    keys, _ = R.route(src, [(3, 3)])
    wi = R.weight_image(src)
    goal = [50 * 96 + 90]
    for lookahead, n_way in ((1, 88), (8, 12), (64, 3), (1024, 2)):
        (way,), info = WP.waypoints(keys, wi, goal, lookahead, 0, 4096)
        assert tuple(info[0]) == (88, n_way, 529, 529), (lookahead, info)
        assert way.size == n_way and way[0] == 3 * 96 + 3 and way[-1] == goal[0]


def test_a_cluttered_map_with_weights():
    """random_map(97, 130, 0.15) with random weights, two seeds: paths of about 120 cells take about 55 waypoints without slack and
    about 30 where the slack never binds; the count is not monotone in the slack by law, so the ordering is asserted on the goals
    where the restatement shows it, and those are most"""
    shown = 0
    for seed in (7, 8):
        src = R.random_map(97, 130, 0.15, seed)
        w = R.random_weights(seed)
        keys, _ = R.route(src, [(5, 5), (90, 120)], 50, w)
        wi = R.weight_image(src, 50, w)
        flat = keys.ravel()
        reached = np.nonzero(flat != R.NONE)[0]
        top = reached[np.argsort(flat[reached], kind="stable")[-5:]]
        n = {slack: _props(keys, wi, top, 128, slack, f"seed {seed}")[1]["n_way"] for slack in (0, 200, 100000)}
        lens = R.trace(keys, wi, top, MAX_LEN)[1]
        assert (lens > 60).all() and (n[0] > lens // 4).all() and (n[100000] < n[0]).all(), (lens, n)
        order = (n[0] >= n[200]) & (n[200] >= n[100000])
        shown += int(order.sum())
    assert shown >= 8, shown


# ---- the diagonal rule
def test_one_blocked_corner_refuses_a_diagonal_step():
    src = np.zeros((5, 5), dtype=np.int8)
    wi = R.weight_image(src)
    assert WP.segment(wi, (1, 1), (3, 3)) == (True, 14)
    for corner in ((2, 1), (1, 2), (3, 2), (2, 3)):
        blocked = src.copy()
        blocked[corner[1], corner[0]] = R.O
        assert not WP.segment(R.weight_image(blocked), (1, 1), (3, 3))[0], corner
        assert not WP.segment(R.weight_image(blocked), (3, 3), (1, 1))[0], corner
        assert V.view(blocked, 1 * 5 + 1, 3)[3, 3], corner      # the views' rule lets the ray through: only two corners make a wall
    # ... and so the waypoints go round the corner the route goes round
    blocked = src.copy()
    blocked[1, 2] = R.O
    keys, _ = R.route(blocked, [(1, 1)])
    (way,), info = WP.waypoints(keys, R.weight_image(blocked), [3 * 5 + 3], 8, 0, 64)
    assert info["n_way"][0] > 2 and info["cost"][0] == info["dist"][0]
    # a straight step has no corners to ask
    wall = src.copy()
    wall[0, 2] = wall[2, 2] = R.O
    assert WP.segment(R.weight_image(wall), (1, 1), (3, 1)) == (True, 10)


def test_segment_cost_and_bound():
    src = np.array([[0, 10, 20, 30]], dtype=np.int8)
    wi = R.weight_image(src, 50, np.arange(1, 52, dtype=np.uint8))
    assert WP.segment(wi, (0, 0), (3, 0)) == (True, 5 * (11 + 21 + 31))
    assert WP.segment(wi, (0, 0), (3, 0), 5 * 63)[0] and not WP.segment(wi, (0, 0), (3, 0), 5 * 63 - 1)[0]


# ---- the ABI
def test_struct_sizes(hip_lib):
    assert hip_lib.tsd_abi_sizeof(b"tsd_waypoint_params") == C.sizeof(capi.WaypointParams) == 16
    assert hip_lib.tsd_abi_sizeof(b"tsd_waypoint_info") == C.sizeof(capi.WaypointInfo) == capi.WAYPOINT_INFO_DTYPE.itemsize == 16
    assert capi.WAYPOINT_INFO_DTYPE == WP.INFO_DTYPE and capi.WAYPOINT_MAX_LOOKAHEAD == WP.MAX_LOOKAHEAD == 1024


def test_the_library_has_the_waypoint_entry(hip_lib):
    assert "tsd_route_waypoints" in capi.ABI and getattr(hip_lib, "tsd_route_waypoints") is not None
    from ohm_tsd_slam_amd import facade
    for name in ("tsd_node_explore_waypoints", "tsd_fleet_explore_waypoints"):
        assert name in facade.HOST_ABI, name
