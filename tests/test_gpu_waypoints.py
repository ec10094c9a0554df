"""Waypoints on the device (csrc/waypoint.hip; tsd_route_waypoints, the facade's explore_waypoints) against the restatement of
tests/waypoint_ref.py: every comparison is byte for byte -- the waypoints, every field of the records, and the words of a
sentinel-filled output the call must not write."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import frontier_ref as F
from tests import route_ref as R
from tests import waypoint_ref as WP

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [c[0] for c in CASES]
SENTINEL = 0xA5A5A5A5
PAIRS = [(1, 0), (8, 0), (64, 0), (65, 0), (128, 200), (128, 1 << 20)]          # (lookahead, slack)
LONG = [c[0] for c in CASES if c[0].startswith("open_") or c[0] in ("serpentine", "weights_255_1x300")]   # where lookahead 1024 runs
MAX_LEN = 4096


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def fields():
    """per case the restatement's keys, the weight image and the goal cells, computed once and left unchanged"""
    out = {}
    for name, src, _, p in CASES:
        keys, _ = R.route(src, p["seeds"], p["free_max"], p["w"], p["limit"])
        keys.setflags(write=False)
        out[name] = (keys, R.weight_image(src, p["free_max"], p["w"]), _goal_cells(keys))
    return out


def _goal_cells(keys, seed=5):
    """the 8 reached cells with the largest keys, 8 seeded random reached cells, a seed's own cell, one cell without a key (where
    the map has one) and one index outside the map"""
    flat = keys.ravel()
    reached = np.nonzero(flat != R.NONE)[0]
    assert reached.size
    far = reached[np.argsort(flat[reached], kind="stable")[-8:]]
    rnd = np.random.default_rng(seed).choice(reached, size=min(8, reached.size), replace=False)
    cells = list(far) + list(rnd) + [int(reached[np.argmin(flat[reached])])]
    none = np.nonzero(flat == R.NONE)[0]
    if none.size:
        cells.append(int(none[none.size // 2]))
    cells.append(flat.size + 7)
    return np.array(cells, dtype=np.uint32)


def _upload(grid, src, stride):
    H_, W = src.shape
    padded = np.full((H_, stride), -1, dtype=np.int8)
    padded[:, :W] = src
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    return buf


def _route(grid, src, stride=None, **kw):
    """the route result of `src` on the context (the map is released: the waypoints work on what the route call kept)"""
    H_, W = src.shape
    stride = W if stride is None else stride
    buf = _upload(grid, src, stride)
    try:
        return grid.route_of(buf.ptr, W, H_, stride, **kw)
    finally:
        buf.free()


def _route_case(grid, case):
    name, src, stride, p = case
    return _route(grid, src, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"], max_rounds=p["max_rounds"])


def _raw(grid, cells, lookahead, slack, max_len=MAX_LEN, max_way=256, way=None, info=None):
    """one tsd_route_waypoints call into sentinel-filled outputs: (rc, way (n, max_way) uint32, info)"""
    cells = np.ascontiguousarray(cells, dtype=np.uint32).ravel()
    if way is None:
        way = np.full((cells.size, max(max_way, 1)), SENTINEL, dtype=np.uint32)
        info = np.frombuffer(np.full(4 * cells.size, SENTINEL, dtype=np.uint32).tobytes(), dtype=capi.WAYPOINT_INFO_DTYPE).copy()
    prm = capi.WaypointParams(lookahead, slack, max_len, max_way)
    rc = grid.lib.tsd_route_waypoints(grid.h, cells.ctypes.data, cells.size, C.byref(prm), way.ctypes.data, info.ctypes.data)
    return rc, way, info


def _same(got, want, max_way, what):
    """the call's outputs against the restatement's: the records, the waypoints written and the sentinel behind them"""
    rc, way, info = got
    want_ways, want_info = want
    assert rc == 0, what
    assert info.tobytes() == want_info.tobytes(), (what, info[info != want_info][:4], want_info[info != want_info][:4])
    for g, w in enumerate(want_ways):
        k = min(len(w), max_way)
        assert np.array_equal(way[g, :k], w[:k]), (what, g, way[g, :k][:8], w[:8])
        assert (way[g, k:] == SENTINEL).all(), (what, g, "words beyond the waypoints were written")


def _check(grid, keys, wi, cells, lookahead, slack, what, max_len=MAX_LEN, max_way=256):
    want = WP.waypoints(keys, wi, cells, lookahead, slack, max_len)
    _same(_raw(grid, cells, lookahead, slack, max_len, max_way), want, max_way, what)
    return want


# ---- every drawn and random map
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"lookahead{p[0]}_slack{p[1]}")
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_waypoints_equal_the_restatement(grid, fields, case, pair):
    keys, wi, cells = fields[case[0]]
    _route_case(grid, case)
    _, info = _check(grid, keys, wi, cells, pair[0], pair[1], case[0])
    print(f"{case[0]} {pair}: len {info['len'].tolist()} n_way {info['n_way'].tolist()}")


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in LONG], ids=LONG)
def test_the_longest_lookahead(grid, fields, case):
    keys, wi, cells = fields[case[0]]
    _route_case(grid, case)
    _, info = _check(grid, keys, wi, cells, 1024, 0, case[0])
    if case[0].startswith("open_"):
        assert (info["n_way"][:8] == 2).all()               # (an open map: the goal is in sight of the seed)


def test_named_numbers(grid):
    """a free 96 x 64 map, seed (3, 3), goal (90, 50): 88 cells, d = 529"""
    src = np.zeros((64, 96), dtype=np.int8)
    _route(grid, src, seeds=[(3, 3)])
    goal = [50 * 96 + 90]
    for lookahead, n_way in ((1, 88), (8, 12), (64, 3), (1024, 2)):
        rc, way, info = _raw(grid, goal, lookahead, 0)
        assert rc == 0 and tuple(info[0]) == (88, n_way, 529, 529), (lookahead, info)
        assert way[0, 0] == 3 * 96 + 3 and way[0, n_way - 1] == goal[0]
    (path,), _ = grid.route_paths(goal)
    (way,), _ = grid.route_waypoints(goal, lookahead=1)
    assert np.array_equal(way, path[::-1])                     # lookahead 1: the trace in driving order


# ---- segment lengths at the wave's edge
ROOM, CENTRE = 263, 131
DISTS = {63: 8, 64: 29, 65: 17, 128: 40, 129: 55}            # the distance and the minor offset: no goal lies on another goal's line


def _octant_goals():
    """per octant and distance D the goal at Chebyshev distance D: [(octant, D, (x, y))]"""
    out = []
    for o in range(8):
        for D, minor in DISTS.items():
            major = D
            dx, dy = (major, minor) if o & 1 else (minor, major)
            out.append((o, D, (CENTRE + (dx if o & 2 else -dx), CENTRE + (dy if o & 4 else -dy))))
    return out


def _room_check(grid, src, goals, what):
    seed = (CENTRE, CENTRE)
    keys, _ = R.route(src, [seed])
    _route(grid, src, seeds=[seed])
    cells = [y * ROOM + x for _, _, (x, y) in goals]
    return _check(grid, keys, R.weight_image(src), cells, 1024, 0, what)


def test_segments_at_the_wave_edge():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        goals = _octant_goals()
        free = np.zeros((ROOM, ROOM), dtype=np.int8)
        ways, info = _room_check(g, free, goals, "free room")
        assert (info["n_way"] == 2).all() and all(len(WP.line((CENTRE, CENTRE), q)) == D for _, D, q in goals)
        # one blocking cell on every goal's line at step 64, 65, N - 1 (where the line has such a step before its end) ...
        for step in (64, 65, -1):
            src, hit = free.copy(), []
            for k, (_, D, q) in enumerate(goals):
                s = D - 1 if step < 0 else step
                if 1 <= s <= D - 1:
                    x, y = WP.line((CENTRE, CENTRE), q)[s - 1]
                    assert (x, y) not in [t[2] for t in goals]
                    src[y, x] = R.O
                    hit.append(k)
            assert len(hit) >= 16
            ways, info = _room_check(g, src, goals, f"a block at step {step}")
            assert (info["n_way"][hit] > 2).all() and (info["len"][hit] > 0).all(), (step, info[hit])
        # ... and at step 1, octant by octant: the eight first steps together would wall the seed in
        for o in range(8):
            mine = [t for t in goals if t[0] == o]
            src = free.copy()
            for _, _, q in mine:
                x, y = WP.line((CENTRE, CENTRE), q)[0]
                src[y, x] = R.O
            ways, info = _room_check(g, src, mine, f"a block at step 1, octant {o}")
            assert (info["n_way"] > 2).all() and (info["len"] > 0).all(), (o, info)
    finally:
        g.close()


# ---- the window's edge
@pytest.mark.parametrize("L", [8, 64])
def test_window_edge_on_a_corridor(grid, L):
    src = np.zeros((1, L + 8), dtype=np.int8)
    keys, _ = R.route(src, [(0, 0)])
    _route(grid, src, seeds=[(0, 0)])
    cells = [L - 1, L, L + 1]                                  # len = L, L + 1, L + 2
    _, info = _check(grid, keys, R.weight_image(src), cells, L, 0, f"corridor {L}")
    assert info["len"].tolist() == [L, L + 1, L + 2] and info["n_way"].tolist() == [2, 2, 3]


# ---- cuts
def test_cuts(grid, fields):
    case = next(c for c in CASES if c[0] == "random_0.15_97x130")
    keys, wi, cells = fields[case[0]]
    _route_case(grid, case)
    want = WP.waypoints(keys, wi, cells, 8, 0, MAX_LEN)
    assert want[1]["n_way"].max() > 3
    _same(_raw(grid, cells, 8, 0, MAX_LEN, 3), want, 3, "max_way 3")              # the full n_way, three words written
    _same(_raw(grid, cells, 8, 0, MAX_LEN, 1), want, 1, "max_way 1")
    short = int(np.median(want[1]["len"][want[1]["len"] > 0]))
    cut = WP.waypoints(keys, wi, cells, 8, 0, short)
    assert ((cut[1]["len"] > short) & (cut[1]["n_way"] == 0)).any() and (cut[1]["n_way"] > 0).any()
    assert np.array_equal(cut[1]["len"], want[1]["len"])
    _same(_raw(grid, cells, 8, 0, short), cut, 256, "max_len")


# ---- n_goals
def test_one_goal_and_the_most_goals(grid):
    src = np.zeros((64, 64), dtype=np.int8)
    src[30:34, 40] = R.O
    keys, _ = R.route(src, [(21, 21)])
    wi = R.weight_image(src)
    _route(grid, src, seeds=[(21, 21)])
    _check(grid, keys, wi, [63 * 64 + 63], 64, 0, "one goal")
    cells = np.arange(64 * 64, dtype=np.uint32)
    assert cells.size == capi.ROUTE_MAX_GOALS
    _check(grid, keys, wi, cells, 64, 0, "4096 goals", max_len=256, max_way=8)


# ---- a key image that did not converge
def test_an_image_that_did_not_converge(grid, fields):
    case = next(c for c in CASES if c[0] == "serpentine")
    _, src, stride, p = case
    _, wi, _ = fields["serpentine"]
    part, info = _route(grid, src, stride, seeds=p["seeds"], max_rounds=1)
    assert info["converged"] == 0
    cells = _goal_cells(part)
    ways, winfo = _check(grid, part, wi, cells, 64, 0, "one round")
    assert (winfo["n_way"][winfo["len"] <= 0] == 0).all() and (winfo["n_way"] > 0).any()
    # a key raised by hand in the middle of the corridor: the walk finds no neighbour that matches there (len -1)
    keys_dev = grid.route_dev_ptrs()[0]
    torn = part.copy()
    reached = np.nonzero(torn.ravel() != R.NONE)[0]
    order = reached[np.argsort(torn.ravel()[reached], kind="stable")]
    mid, far = int(order[order.size // 2]), int(order[-1])
    torn.ravel()[mid] += 16
    grid._check(grid.lib.tsd_dev_copy(grid.h, keys_dev, torn.ctypes.data, torn.nbytes, 1), "tsd_dev_copy")
    ways, winfo = _check(grid, torn, wi, [far, mid, int(order[order.size // 4])], 64, 0, "a torn image")
    assert winfo["len"].tolist()[:2] == [-1, -1] and winfo["n_way"].tolist()[:2] == [0, 0] and winfo["n_way"][2] > 0


# ---- both ends of the route's schedule
def test_both_ends_of_the_schedule(grid, fields):
    case = next(c for c in CASES if c[0] == "random_0.05_64x64")
    keys, wi, cells = fields[case[0]]
    want = WP.waypoints(keys, wi, cells, 128, 200, MAX_LEN)
    for sweeps in (1, 0):
        grid.set_route_sweeps(sweeps)
        try:
            name, src, stride, p = case
            _route(grid, src, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"], max_rounds=1 << 16)
        finally:
            grid.set_route_sweeps(0)
        _same(_raw(grid, cells, 128, 200), want, 256, f"sweeps {sweeps}")


# ---- refusals, and the call after them
def test_refusals_leave_everything_in_place(grid, fields):
    case = next(c for c in CASES if c[0] == "random_0.05_64x64")
    keys, wi, cells = fields[case[0]]
    _route_case(grid, case)
    lib, h = grid.lib, grid.h
    c2 = np.ascontiguousarray(cells[:2])
    way = np.full((2, 4), SENTINEL, dtype=np.uint32)
    info = np.frombuffer(np.full(8, SENTINEL, dtype=np.uint32).tobytes(), dtype=capi.WAYPOINT_INFO_DTYPE).copy()

    def call(cells_=c2.ctypes.data, n=2, prm=(8, 0, 64, 4), way_=way.ctypes.data, info_=info.ctypes.data):
        p = None if prm is None else C.byref(capi.WaypointParams(*prm))
        return lib.tsd_route_waypoints(h, cells_, n, p, way_, info_)

    bad = {"goal_cells is NULL": dict(cells_=None), "params is NULL": dict(prm=None), "way_host is NULL": dict(way_=None),
           "info_host is NULL": dict(info_=None), "n_goals is outside": dict(n=0), "n_goals is outside 1": dict(n=4097),
           "lookahead is outside": dict(prm=(0, 0, 64, 4)), "lookahead is outside 1": dict(prm=(1025, 0, 64, 4)),
           "max_len is below 1": dict(prm=(8, 0, 0, 4)), "max_way is below 1": dict(prm=(8, 0, 64, 0)),
           "n_goals * max_len": dict(prm=(8, 0, (1 << 23) + 1, 4)), "n_goals * max_way": dict(prm=(8, 0, 64, (1 << 23) + 1))}
    for why, kw in bad.items():
        assert call(**kw) == -1 and why.encode() in lib.tsd_last_error(h), (why, lib.tsd_last_error(h))
        assert b"tsd_route_waypoints" in lib.tsd_last_error(h)
    assert (way == SENTINEL).all() and (info.view(np.uint32) == SENTINEL).all()
    assert np.array_equal(grid.route_keys(), keys)            # the route result is still there, and a valid call works on it
    _check(grid, keys, wi, cells, 8, 0, "after the refusals")
    fresh = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        prm = capi.WaypointParams(8, 0, 64, 4)
        assert fresh.lib.tsd_route_waypoints(fresh.h, c2.ctypes.data, 2, C.byref(prm), way.ctypes.data, info.ctypes.data) == -1
        assert b"no route result" in fresh.lib.tsd_last_error(fresh.h)
    finally:
        fresh.close()


# ---- a repeated call
def test_a_repeated_call_gives_the_same_bytes(grid, fields):
    case = next(c for c in CASES if c[0] == "random_0.15_97x130")
    keys, wi, cells = fields[case[0]]
    _route_case(grid, case)
    rc, way, info = _raw(grid, cells, 64, 200)
    first = (way.copy(), info.copy())
    way[:] = SENTINEL
    info.view(np.uint32)[:] = SENTINEL
    rc2, way, info = _raw(grid, cells, 64, 200, way=way, info=info)
    assert rc == rc2 == 0 and way.tobytes() == first[0].tobytes() and info.tobytes() == first[1].tobytes()
    _same((rc2, way, info), WP.waypoints(keys, wi, cells, 64, 200, MAX_LEN), 256, "the second call")


# ---- the facade: SlamNode.explore_waypoints, SlamFleet.explore_waypoints
def _metres(cells, width, m):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([((cells % width) + 0.5) * m["resolution"] + m["origin_position"][0],
                     ((cells // width) + 0.5) * m["resolution"] + m["origin_position"][1]], axis=-1).reshape(-1, 2)


def _check_waypoints(out, plan, m, seeds, min_size, lookahead_m, slack=0, max_way=256):
    data = m["data"]
    W = data.shape[1]
    rec, lab, _ = F.frontiers(data, 0, min_size, seeds)
    keys, _ = R.route(data, seeds)
    goals = R.goals(keys, lab, rec)
    assert plan["goals"].tobytes() == goals.tobytes()
    cells_want = min(max(int(np.floor(lookahead_m / m["resolution"] + 0.5)), 1), capi.WAYPOINT_MAX_LOOKAHEAD)
    assert out["lookahead_cells"] == cells_want
    ways, info = WP.waypoints(keys, R.weight_image(data), goals["cell"], cells_want, slack, MAX_LEN)
    assert out["info"].tobytes() == info.tobytes() and (info["n_way"] > 1).any()
    for got, w in zip(out["waypoints"], ways):
        assert got.shape == (min(len(w), max_way), 2) and np.array_equal(got, _metres(w[:max_way], W, m))
    none = goals["cell"] == R.NONE
    assert (info["len"][none] == 0).all() and (info["n_way"][none] == 0).all()
    return info


def _node(**over):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over.update(occ_grid_time_interval=1000.0)
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    return gc, geo, scans, over


def test_node_explore_waypoints():
    gc, geo, scans, over = _node(frontier_min_size=3)
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        with pytest.raises(capi.TsdError):
            node.explore_waypoints(2.0)                        # no plan yet
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m = node.map_msg()
        pose = node.pose_msg()["position"]
        seed = tuple(int(np.floor((pose[a] - m["origin_position"][a]) / m["resolution"])) for a in (0, 1))
        plan = node.explore_plan()
        for lookahead_m, slack, max_way in ((3.0, 0, 256), (0.01, 0, 256), (1e6, 0, 256), (3.0, 0, 2)):
            out = node.explore_waypoints(lookahead_m, slack, max_way)
            info = _check_waypoints(out, plan, m, [seed], 3, lookahead_m, slack, max_way)
        # the plan's paths and the straightened ones start and end alike
        for path, way in zip(plan["paths"], node.explore_waypoints(3.0)["waypoints"]):
            assert len(way) == 0 or (np.array_equal(way[0], path[0]) and np.array_equal(way[-1], path[-1]) and len(way) <= len(path))
        node.publish_map()
        with pytest.raises(capi.TsdError):
            node.explore_waypoints(3.0)                        # the plan is of the map published before
        node.explore_plan()
        node.explore_waypoints(3.0)
    finally:
        node.close()


def test_fleet_explore_waypoints():
    gc, geo, scans, over = _node(frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        with pytest.raises(capi.TsdError):
            fleet.explore_waypoints(3.0)                       # no plan yet
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        seeds = []
        for n in nodes:
            pose = n.pose_msg()["position"]
            seeds.append(tuple(int(np.floor((pose[a] - m["origin_position"][a]) / m["resolution"])) for a in (0, 1)))
        plan = fleet.explore_plan(min_size=2)
        _check_waypoints(fleet.explore_waypoints(3.0), plan, m, seeds, 2, 3.0)
        _check_waypoints(fleet.explore_waypoints(0.5, 0, 4), plan, m, seeds, 2, 0.5, 0, 4)
        fleet.publish_merged_map()
        with pytest.raises(capi.TsdError):
            fleet.explore_waypoints(3.0)                       # the plan is of the merged map published before
    finally:
        fleet.close()
        for n in nodes:
            n.close()
