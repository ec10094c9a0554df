"""Routes on the device (csrc/route.hip; tsd_route_dev / _frame / _goals / _trace / _dev_ptrs, the facade's explore_plan) against the
restatement of tests/route_ref.py: every comparison is byte for byte -- the key image, the goals, the paths.  The maps are those of
tests/test_cpu_route.py, where the restatement is checked against a heap Dijkstra and the drawn maps' named cells are asserted."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import frontier_ref as F
from tests import helpers as H
from tests import route_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [c[0] for c in CASES]
SENTINEL = 0xA5A5A5A5
U, O = R.U, R.O
MANY_ROUNDS = 1 << 16          # for the one-sweep schedule, whose rounds are as many as the longest path has cells


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def fields():
    """the restatement's (keys, seeds_used) per case, computed once and left unchanged"""
    out = {name: R.route(src, p["seeds"], p["free_max"], p["w"], p["limit"]) for name, src, _, p in CASES}
    for keys, _ in out.values():
        keys.setflags(write=False)
    return out


def _upload(grid, src, stride):
    """the map as `height` rows of `stride` bytes on the device; the padding holds -1s"""
    H_, W = src.shape
    padded = np.full((H_, stride), -1, dtype=np.int8)
    padded[:, :W] = src
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    return buf


def _call(grid, src, stride=None, **kw):
    """one call with the key image prefilled: a first call puts the context's key image in place for this size, the sentinel is
    written over it, and the second call must write every cell (and allocate nothing: the image stays where it is).  The map is
    released before the result is used."""
    H_, W = src.shape
    stride = W if stride is None else stride
    buf = _upload(grid, src, stride)
    try:
        grid.route_of(buf.ptr, W, H_, stride, **kw)
        keys_dev = grid.route_dev_ptrs()[0]
        fill = np.full(W * H_, SENTINEL, dtype=np.uint32)
        grid._check(grid.lib.tsd_dev_copy(grid.h, keys_dev, fill.ctypes.data, fill.nbytes, 1), "tsd_dev_copy")
        keys, info = grid.route_of(buf.ptr, W, H_, stride, **kw)
        assert grid.route_dev_ptrs() == (keys_dev, W, H_), "a repeated call at the same size moved the key image"
    finally:
        buf.free()
    return keys, info


def _check(grid, src, stride, want, p, max_rounds=None, what=""):
    want_keys, want_used = want
    keys, info = _call(grid, src, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"],
                       max_rounds=p["max_rounds"] if max_rounds is None else max_rounds)
    assert not (keys == SENTINEL).any(), f"{what}: {np.count_nonzero(keys == SENTINEL)} keys were not written"
    assert np.array_equal(keys, want_keys), f"{what}: {np.count_nonzero(keys != want_keys)} keys differ at {np.argwhere(keys != want_keys)[:4]}"
    assert info["converged"] == 1 and info["seeds_used"] == want_used, (what, info)
    assert info["reached"] == np.count_nonzero(want_keys != R.NONE), (what, info)
    return keys, info


# ---- every drawn and random map, at both ends of the schedule
@pytest.mark.parametrize("sweeps", [0, 1], ids=["default_sweeps", "one_sweep"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_keys_equal_the_restatement(grid, fields, case, sweeps):
    name, src, stride, p = case
    grid.set_route_sweeps(sweeps)
    try:
        _, info = _check(grid, src, stride, fields[name], p, max_rounds=MANY_ROUNDS if sweeps else None, what=name)
    finally:
        grid.set_route_sweeps(0)
    print(f"{name}: {info}, tile visits and host waits {grid.route_counts()}")


@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("open_")], ids=lambda c: c[0])
def test_open_map_closed_form(grid, case):
    name, src, stride, p = case
    H_, W = src.shape
    (sx, sy), = p["seeds"]
    keys, _ = _call(grid, src, stride, seeds=p["seeds"])
    dx, dy = np.abs(np.arange(W)[None, :] - sx), np.abs(np.arange(H_)[:, None] - sy)
    assert np.array_equal(keys, ((7 * np.minimum(dx, dy) + 5 * np.abs(dx - dy)) << 4).astype(np.uint32))


def test_named_cells_on_the_device(grid):
    """the cells the drawn maps are drawn for, read from the device's image"""
    by = {c[0]: c for c in CASES}

    def run(name):
        _, src, stride, p = by[name]
        return _call(grid, src, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"])[0]

    k = run("limit_100")
    assert k[0, 20] == 100 << 4 and k[0, 21] == R.NONE and k[20, 0] == 100 << 4 and k[21, 0] == R.NONE and k[14, 14] == 98 << 4
    assert k[15, 15] == R.NONE
    assert run("weights_255_1x300")[299, 0] == 381225 << 4
    k = run("equidistant_column")
    assert (k[:, 16] & 15 == 0).all() and k[16, 16] == 60 << 4 and k[16, 15] & 15 == 1
    k = run("two_seeds_one_cell")
    assert k[10, 10] == 0 and k[20, 20] == 2
    k = run("seeds_ignored")
    assert k[30, 30] == 5 and ((k[k != R.NONE] & 15) == 5).all()
    for name in ("corner_diagonal_64x64", "corner_antidiagonal_64x64"):
        k = run(name)
        anti = "anti" in name
        assert (k[:32, (33 if anti else 32):] == R.NONE).all() and (k[32:, (32 if anti else 33):] == R.NONE).all()


@pytest.mark.parametrize("sweeps", [0, 1], ids=["default_sweeps", "one_sweep"])
def test_serpentine_out_of_rounds(grid, fields, sweeps):
    """max_rounds = 4: not converged, every key an upper bound of the rule's, the seed's cell exact"""
    _, src, stride, p = CASES[IDS.index("serpentine")]
    want = fields["serpentine"][0]
    grid.set_route_sweeps(sweeps)
    try:
        keys, info = _call(grid, src, stride, seeds=p["seeds"], max_rounds=4)
    finally:
        grid.set_route_sweeps(0)
    assert info["converged"] == 0 and info["rounds"] == 4 and info["seeds_used"] == 1
    assert not (keys == SENTINEL).any() and (keys >= want).all() and (keys != want).any()
    assert keys[16, 8] == want[16, 8] == 0
    assert info["reached"] == np.count_nonzero(keys != R.NONE) < np.count_nonzero(want != R.NONE)
    # the default cap of a 256 x 256 map is 16 * (8 + 8) + 64 = 320 rounds
    _, info = _call(grid, src, stride, seeds=p["seeds"])
    assert info["rounds"] <= 320 and (info["converged"] == 1 or info["rounds"] == 320)


# ---- one context, many calls
def test_repeated_calls_keep_the_scratch(grid):
    large, small = R.random_map(256, 256, 0.15, 5), R.random_map(33, 33, 0.15, 6)
    w = R.random_weights(9)
    out = []
    for src in (large, small, large):
        H_, W = src.shape
        seeds = [(W // 2, H_ // 2), (3, 3), (W - 2, 1)]
        keys, info = _check(grid, src, W, R.route(src, seeds, 50, w), dict(seeds=seeds, free_max=50, w=w, limit=0, max_rounds=0))
        out.append((keys, grid.route_dev_ptrs()[0]))
        assert np.array_equal(grid.route_keys(), keys)
    assert np.array_equal(out[0][0], out[2][0])
    assert out[0][1] == out[1][1] == out[2][1], "the scratch of the large call was not kept"


def test_argument_errors_leave_the_previous_result(grid):
    src = R.corner_wall(64, 64, False)
    buf = _upload(grid, src, 64)
    try:
        keys, _ = grid.route_of(buf.ptr, 64, 64, 64, seeds=[(5, 5)])
        lib, h = grid.lib, grid.h
        info = capi.RouteInfo(-7, -7, -7, 7)
        xy = (C.c_int32 * 2)(5, 5)
        w0 = (C.c_uint8 * 3)(1, 0, 1)

        def prm(free_max=0, n_seeds=1, seeds=xy, weights=None, limit=0, max_rounds=0):
            return C.byref(capi.RouteParams(free_max, n_seeds, seeds, weights, limit, max_rounds))

        def dev(ptr=buf.ptr, W=64, H_=64, stride=64, p=None, i=C.byref(info)):
            return lib.tsd_route_dev(h, C.c_void_p(ptr), W, H_, stride, prm() if p is None else p, i)

        assert dev(ptr=0) == -1 and b"null map" in lib.tsd_last_error(h)
        assert lib.tsd_route_dev(h, C.c_void_p(buf.ptr), 64, 64, 64, None, C.byref(info)) == -1
        assert dev(i=None) == -1
        for W, H_ in ((0, 64), (64, 0), (-1, 64), (32769, 1), (1, 32769)):
            assert dev(W=W, H_=H_, stride=max(W, 64)) == -1, (W, H_)
        assert dev(stride=63) == -1
        bad = (prm(free_max=-1), prm(free_max=100), prm(free_max=2, weights=w0), prm(limit=capi.ROUTE_MAX_DIST + 1), prm(n_seeds=0),
               prm(n_seeds=17), prm(seeds=None), prm(max_rounds=-1), prm(max_rounds=(1 << 20) + 1))
        for k, b in enumerate(bad):
            assert dev(p=b) == -1, k
            assert lib.tsd_route_frame(h, 0, b, C.byref(info)) == -1, k
        assert lib.tsd_route_frame(h, 0, prm(), C.byref(info)) == -1 and b"no completed frame" in lib.tsd_last_error(h)
        assert lib.tsd_route_frame(h, 1, prm(), C.byref(info)) == -1 and lib.tsd_route_frame(h, 2, prm(), C.byref(info)) == -1
        cells = (C.c_uint32 * 2)(0, 1)
        paths, lens = (C.c_uint32 * 64)(), (C.c_int32 * 2)()
        for args in ((None, 2, 4, paths, lens), (cells, 0, 4, paths, lens), (cells, 4097, 4, paths, lens), (cells, 2, 0, paths, lens),
                     (cells, 2, (1 << 23) + 1, paths, lens), (cells, 2, 4, None, lens), (cells, 2, 4, paths, None)):
            assert lib.tsd_route_trace(h, *args) == -1, args[1:3]
        assert (info.seeds_used, info.rounds, info.converged, info.reached) == (-7, -7, -7, 7)
        # the result of the last good call is still there
        assert np.array_equal(grid.route_keys(), keys) and grid.route_dev_ptrs()[1:] == (64, 64)
        assert lib.tsd_route_trace(h, cells, 2, 4, paths, lens) == 0 and list(lens) == [6, 6]      # (five moves from (5, 5) to either)
        # goals: a frontier result of another size, then one of the same size
        other = _upload(grid, np.zeros((16, 16), dtype=np.int8), 16)
        try:
            grid.frontiers_of(other.ptr, 16, 16, 16)
            n = C.c_int(-7)
            assert lib.tsd_route_goals(h, C.byref(n)) == -1 and b"differ in size" in lib.tsd_last_error(h) and n.value == -7
        finally:
            other.free()
        grid.frontiers_of(buf.ptr, 64, 64, 64)
        assert lib.tsd_route_goals(h, None) == -1
        assert grid.route_goals().size == 0                  # (no unknown cell: no frontier)
        assert lib.tsd_route_goals_fetch(h, 0, 1, None) == -1 and lib.tsd_route_goals_fetch(h, 0, 0, None) == 0
        assert dev(p=prm(free_max=99, limit=capi.ROUTE_MAX_DIST, max_rounds=1 << 20)) == 0 and info.converged == 1 and info.seeds_used == 1
    finally:
        buf.free()


def test_no_result_before_the_first_call():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        with pytest.raises(capi.TsdError):
            g.route_dev_ptrs()
        n = C.c_int(0)
        cells, paths, lens = (C.c_uint32 * 1)(0), (C.c_uint32 * 4)(), (C.c_int32 * 1)()
        assert g.lib.tsd_route_goals(g.h, C.byref(n)) == -1 and b"no route result" in g.lib.tsd_last_error(g.h)
        assert g.lib.tsd_route_goals_fetch(g.h, 0, 0, None) == -1
        assert g.lib.tsd_route_trace(g.h, cells, 1, 4, paths, lens) == -1 and b"no route result" in g.lib.tsd_last_error(g.h)
        # a route result, but no frontier result on this context
        buf = _upload(g, np.zeros((8, 8), dtype=np.int8), 8)
        try:
            g.route_of(buf.ptr, 8, 8, 8, seeds=[(1, 1)])
        finally:
            buf.free()
        assert g.lib.tsd_route_goals(g.h, C.byref(n)) == -1 and b"no frontier result" in g.lib.tsd_last_error(g.h)
        assert g.lib.tsd_route_trace(g.h, cells, 1, 4, paths, lens) == 0 and lens[0] == 2 and list(paths[:2]) == [0, 9]
    finally:
        g.close()


# ---- goals and paths
def _two_rooms_with_pockets():
    """96 x 64: two rooms split by a wall at x = 48, an unknown column at either end (a frontier of 64 cells in each room); in the left
    room an unknown cell at (20, 60) (a frontier of 4 cells, more than 250 away from the seed) and one at (40, 12) under an obstacle
    at (40, 11): its frontier's cells (39, 12) and (41, 12) cost the same from the seed at (40, 10), (40, 13) costs more"""
    src = np.zeros((64, 96), dtype=np.int8)
    src[:, 0] = U
    src[:, 95] = U
    src[:, 48] = O
    src[60, 20] = U
    src[12, 40] = U
    src[11, 40] = O
    return src


@pytest.mark.parametrize("min_size", [1, 9])
def test_goals_of_the_frontiers(grid, min_size):
    src = _two_rooms_with_pockets()
    W = 96
    seeds = [(40, 10), (60, 10)]
    buf = _upload(grid, src, 104)
    try:
        rec, lab, _ = grid.frontiers_of(buf.ptr, W, 64, 104, min_size=min_size, seeds=seeds)
        keys, info = grid.route_of(buf.ptr, W, 64, 104, seeds=seeds, limit=250)
    finally:
        buf.free()
    goals = grid.route_goals()
    want_rec, want_lab, _ = F.frontiers(src, 0, min_size, seeds)
    want_keys, _ = R.route(src, seeds, limit=250)
    want = R.goals(want_keys, want_lab, want_rec)
    assert rec.tobytes() == want_rec.tobytes() and np.array_equal(keys, want_keys) and info["converged"] == 1
    assert goals.dtype == want.dtype and goals.tobytes() == want.tobytes()
    roots = [(int(r["root_x"]), int(r["root_y"])) for r in rec]
    by_root = {r: g for r, g in zip(roots, goals)}
    assert tuple(by_root[(1, 0)]) == (10 * W + 1, 195, 0, 0)                    # the left room's frontier: seed 0, straight west
    assert tuple(by_root[(94, 0)]) == (10 * W + 94, 170, 1, 0)                  # only the second seed reaches the right room
    if min_size == 1:
        assert roots == [(1, 0), (94, 0), (39, 12), (20, 59)]
        assert tuple(by_root[(39, 12)]) == (12 * W + 39, 15, 0, 0)              # the tie: the smaller index of (39, 12) and (41, 12)
        assert want_keys[12, 39] == want_keys[12, 41] == 15 << 4
        assert tuple(by_root[(20, 59)]) == (R.NONE, R.NONE, -1, 0)              # beyond the limit
    else:
        assert roots == [(1, 0), (94, 0)]
    # paths for all goals at once, and for a goal without a key (inside the wall) and one outside the map
    cells = np.concatenate([goals["cell"], np.array([5 * W + 48, W * 64], dtype=np.uint32)])
    paths, lens = grid.route_paths(cells, 4096)
    want_paths, want_lens = R.trace(want_keys, R.weight_image(src), cells, 4096)
    assert np.array_equal(lens, want_lens) and lens[-2:].tolist() == [0, 0] and lens[0] == 40
    for p, q in zip(paths, want_paths):
        assert p.tolist() == q
    assert paths[0][0] == 10 * W + 1 and paths[0][-1] == 10 * W + 40
    # a cut at max_len = 3: the lengths in full, the three cells nearest to the goal
    cut, lens3 = grid.route_paths(cells, 3)
    assert np.array_equal(lens3, want_lens)
    for p, q in zip(cut, want_paths):
        assert p.tolist() == q[:3]


def test_the_longest_serpentine_path(grid, fields):
    _, src, stride, p = CASES[IDS.index("serpentine")]
    want = fields["serpentine"][0]
    keys, _ = _call(grid, src, stride, seeds=p["seeds"], max_rounds=1024)
    far = int(np.argmax(np.where(want != R.NONE, want, 0)))
    (path,), lens = grid.route_paths([far], 4096)
    (want_path,), want_lens = R.trace(want, R.weight_image(src), [far], 4096)
    assert lens[0] == want_lens[0] == np.count_nonzero(src == 0) and path.tolist() == want_path and path[-1] == 16 * 256 + 8
    # on an image that did not converge the walk may find no neighbour that matches: the same answer as the restatement's
    buf = _upload(grid, src, stride)
    try:
        grid.set_route_sweeps(3)
        part, info = grid.route_of(buf.ptr, 256, 256, stride, seeds=p["seeds"], max_rounds=2)
    finally:
        grid.set_route_sweeps(0)
        buf.free()
    assert info["converged"] == 0
    goals = [far, int(np.argmax(np.where(part != R.NONE, part, 0))), 16 * 256 + 8]
    got, lens = grid.route_paths(goals, 64)
    want_paths, want_lens = R.trace(part, R.weight_image(src), goals, 64)
    assert np.array_equal(lens, want_lens) and lens[0] == 0 and lens[2] == 1 and [g.tolist() for g in got] == want_paths


# ---- the frame forms: a pushed grid
GC = synth.GridConfig(8, 0.1)
GEO = synth.ScanGeometry.full_circle_360()
SHORT_RANGE = 3.0


def _push(oracle, dg, world, pose3):
    x, y, yaw = pose3
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, GEO), SHORT_RANGE, GEO.angle_increment)
    dg.push(synth.pose_matrix(x, y, yaw), data, mask, GEO.angle_increment, GEO.angle_min, SHORT_RANGE, H.MIN_RANGE, H.LOW_REFL,
            want_stats=False)


def test_routes_of_a_frame_and_its_refusals(oracle):
    world = synth.World("room", GC)
    dg = capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)
    try:
        for source in ("map", "costmap"):
            with pytest.raises(capi.TsdError):
                dg.route(source, seeds=[(5, 5)])             # no frame yet
            assert dg.last_rc == -1
        poses = [(world.cx - world.hx + 2.0 + 0.3 * k, world.cy - world.hy + 1.5, 0.1 + 0.02 * k) for k in range(6)]
        for pose in poses:
            _push(oracle, dg, world, pose)
        dg.map_frame_begin(False, 2, image=False)
        with pytest.raises(capi.TsdError):
            dg.route("map", seeds=[(5, 5)])                  # a frame in flight
        assert dg.last_rc == -1
        occ, _, _ = dg.map_frame_wait()
        assert (occ == 0).sum() > 100 and (occ == -1).sum() > 100
        ys, xs = np.nonzero(occ == 0)                        # the free cell nearest to the robot, and an unknown corner
        k = np.argmin((xs - poses[0][0] / GC.cell_size) ** 2 + (ys - poses[0][1] / GC.cell_size) ** 2)
        seeds = [(0, 0), (int(xs[k]), int(ys[k]))]
        with pytest.raises(capi.TsdError):
            dg.route("costmap", seeds=seeds)                 # a frame, but no cost map yet
        keys, info = dg.route("map", seeds=seeds)
        want, used = R.route(occ, seeds)
        assert np.array_equal(keys, want) and info["converged"] == 1 and info["seeds_used"] == used == 1
        assert info["reached"] == np.count_nonzero(want != R.NONE) > 100
        # the goals of the frame's frontiers, and the paths to them
        rec, lab, _ = dg.frontiers(min_size=4, seeds=seeds)
        goals = dg.route_goals()
        want_goals = R.goals(want, lab, rec)
        assert goals.tobytes() == want_goals.tobytes() and (goals["seed"] == 1).any()
        reach = goals["cell"][goals["cell"] != R.NONE]
        paths, lens = dg.route_paths(reach, 512)
        want_paths, want_lens = R.trace(want, R.weight_image(occ), reach, 512)
        assert np.array_equal(lens, want_lens) and [p.tolist() for p in paths] == want_paths
        # the cost map of the same frame
        dg.costmap_begin(6)
        for source in ("map", "costmap"):
            with pytest.raises(capi.TsdError):
                dg.route(source, seeds=seeds)                # a cost map in flight
        cost, _ = dg.costmap_wait()
        w = dg.route_weights(98, 40)
        keys, info = dg.route("costmap", seeds=seeds, free_max=98, weights=w)
        want, used = R.route(cost, seeds, 98, w)
        assert np.array_equal(keys, want) and info["converged"] == 1 and info["seeds_used"] == used == 1
        assert (cost != occ).any() and np.count_nonzero(want != R.NONE) > 100
    finally:
        dg.close()


# ---- the facade: SlamNode.explore_plan, SlamFleet.explore_plan
def _metres(cells, width, m):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([((cells % width) + 0.5) * m["resolution"] + m["origin_position"][0],
                     ((cells // width) + 0.5) * m["resolution"] + m["origin_position"][1]], axis=-1)


def _check_plan(out, data, m, seeds, min_size, free_max=0, w=None, max_len=4096):
    """an explore_plan result against the restatement on the published map `data` (the frontiers' map: m["data"])"""
    W = data.shape[1]
    want_rec, want_lab, used = F.frontiers(m["data"], 0, min_size, seeds)
    want_keys, _ = R.route(data, seeds, free_max, w)
    want_goals = R.goals(want_keys, want_lab, want_rec)
    assert out["seeds"] == seeds and out["seeds_used"] == used
    assert out["records"].tobytes() == want_rec.tobytes() and out["goals"].tobytes() == want_goals.tobytes()
    assert out["route"]["converged"] == 1 and out["route"]["reached"] == np.count_nonzero(want_keys != R.NONE)
    has = want_goals["cell"] != R.NONE
    assert has.any() and np.array_equal(out["goal_xy"][has], _metres(want_goals["cell"][has], W, m)) and np.isnan(out["goal_xy"][~has]).all()
    want_paths, want_lens = R.trace(want_keys, R.weight_image(data, free_max, w), want_goals["cell"], max_len)
    assert np.array_equal(out["path_lens"], want_lens)
    for got, cells in zip(out["paths"], want_paths):
        assert got.shape == (len(cells), 2) and np.array_equal(got, _metres(cells[::-1], W, m).reshape(-1, 2))
    return want_goals


def _node(**over):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over.update(occ_grid_time_interval=1000.0)
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    return gc, geo, scans, over


def test_node_explore_plan():
    gc, geo, scans, over = _node(publish_costmap=True, frontier_min_size=3)
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        with pytest.raises(capi.TsdError):
            node.explore_plan()                            # no map published yet
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m = node.map_msg()
        pose = node.pose_msg()["position"]
        seed = tuple(int(np.floor((pose[a] - m["origin_position"][a]) / m["resolution"])) for a in (0, 1))
        goals = _check_plan(node.explore_plan(), m["data"], m, [seed], 3)
        assert (goals["seed"] == 0).any()
        _check_plan(node.explore_plan(min_size=1, max_len=5), m["data"], m, [seed], 1, max_len=5)
        cost = node.costmap_msg()["data"]
        _check_plan(node.explore_plan(source="costmap", max_weight=30), cost, m, [seed], 3, 98, R.weights(98, 30))
        assert node.frontiers()["records"].tobytes() == F.frontiers(m["data"], 0, 3, [seed])[0].tobytes()
    finally:
        node.close()


def test_fleet_explore_plan_assigns_the_nearer_member():
    """two nodes in the same room, their grids 24 / -16 cells apart: on the merged map every reachable frontier goes to the member
    the restatement finds nearer"""
    gc, geo, scans, over = _node(publish_frontiers=True, frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        with pytest.raises(capi.TsdError):
            fleet.explore_plan()                           # no merged map yet
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        seeds = []
        for n in nodes:
            pose = n.pose_msg()["position"]
            seeds.append(tuple(int(np.floor((pose[a] - m["origin_position"][a]) / m["resolution"])) for a in (0, 1)))
        for min_size in (1, 5):
            goals = _check_plan(fleet.explore_plan(min_size=min_size), m["data"], m, seeds, min_size)
            assert (goals["seed"] >= 0).any()
        # node 0's own plan in between, on the same context at its own (smaller) size
        nodes[0].publish_map()
        own = nodes[0].map_msg()
        pose = nodes[0].pose_msg()["position"]
        seed = tuple(int(np.floor((pose[a] - own["origin_position"][a]) / own["resolution"])) for a in (0, 1))
        _check_plan(nodes[0].explore_plan(), own["data"], own, [seed], 2)
        _check_plan(fleet.explore_plan(), m["data"], m, seeds, 1)
    finally:
        fleet.close()
        for n in nodes:
            n.close()
