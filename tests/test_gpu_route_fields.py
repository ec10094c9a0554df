"""Fields on the device (csrc/route.hip with a layer per seed; tsd_route_fields_*, tsd_view_assign_fields) against the restatement of
tests/route_fields_ref.py: every comparison is byte for byte -- the layers, the goal matrix, the paths, the waypoints, the
assignment and the claims image it leaves.  The maps are those of the route and view tests plus the few drawn here."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, synth
from tests import frontier_ref as F
from tests import helpers as H
from tests import route_fields_ref as RF
from tests import route_ref as R
from tests import view_ref as V
from tests import waypoint_ref as WP

pytestmark = pytest.mark.gpu

U, O = R.U, R.O
SENTINEL = 0xA5A5A5A5
MANY_ROUNDS = 1 << 16          # for the one-sweep schedule, whose rounds are as many as the longest path has cells


def _corner_seeds():
    """both seeds at the corner four tiles share, one on either side of it"""
    return "tile_corner_64x64", np.zeros((64, 64), dtype=np.int8), 64, dict(seeds=[(31, 31), (32, 32)], free_max=0, w=None, limit=0, max_rounds=0)


def _serpentine_and_a_cell():
    """the serpentine with a second seed shut in a one-cell room: layer 1 ends in round 1, layer 0 goes on through every tile"""
    src = R.serpentine()
    assert (src[99:102, 99:102] == U).all()
    src[100, 100] = 0
    return "serpentine_and_a_cell", src, 256, dict(seeds=[(8, 16), (100, 100)], free_max=0, w=None, limit=0, max_rounds=1024)


CASES = R.cases() + [_corner_seeds(), _serpentine_and_a_cell()]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def want_fields():
    """the restatement's (keys, used) per case, computed once and left unchanged"""
    out = {name: RF.fields(src, p["seeds"], p["free_max"], p["w"], p["limit"]) for name, src, _, p in CASES}
    for keys, _ in out.values():
        keys.setflags(write=False)
    return out


def _upload(grid, src, stride=None):
    """the map as `height` rows of `stride` bytes on the device; the padding holds -1s"""
    H_, W = src.shape
    stride = W if stride is None else stride
    padded = np.full((H_, stride), -1, dtype=np.int8)
    padded[:, :W] = src
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    return buf


def _call(grid, src, stride=None, **kw):
    """one fields call with every layer prefilled: a first call puts the key images in place for this size and seed count, the
    sentinel is written over all of them, and the second call must write every cell of every layer and move no buffer"""
    H_, W = src.shape
    stride = W if stride is None else stride
    L = len(kw["seeds"])
    buf = _upload(grid, src, stride)
    try:
        grid.route_fields_of(buf.ptr, W, H_, stride, **kw)
        ptrs = grid.route_fields_dev_ptrs()
        assert ptrs[1:] == (W, H_, L)
        fill = np.full(L * W * H_, SENTINEL, dtype=np.uint32)
        grid._check(grid.lib.tsd_dev_copy(grid.h, ptrs[0], fill.ctypes.data, fill.nbytes, 1), "tsd_dev_copy")
        keys, info = grid.route_fields_of(buf.ptr, W, H_, stride, **kw)
        assert grid.route_fields_dev_ptrs() == ptrs, "a repeated call at the same size moved the key images"
    finally:
        buf.free()
    return keys, info


def _check_info(info, keys, used, what):
    L = keys.shape[0]
    assert info["layers"] == L and info["seeds_used"] == sum(used), (what, info)
    assert info["used"] == list(used) + [0] * (16 - L), (what, info)
    assert info["reached"] == [int(np.count_nonzero(keys[r] != R.NONE)) for r in range(L)] + [0] * (16 - L), (what, info)


# ---- 1., 2. every layer of every drawn and random map, at both ends of the schedule
@pytest.mark.parametrize("sweeps", [0, 1], ids=["default_sweeps", "one_sweep"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layers_equal_the_restatement(grid, want_fields, case, sweeps):
    name, src, stride, p = case
    want, used = want_fields[name]
    grid.set_route_sweeps(sweeps)
    try:
        keys, info = _call(grid, src, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"],
                           max_rounds=MANY_ROUNDS if sweeps else p["max_rounds"])
    finally:
        grid.set_route_sweeps(0)
    print(f"{name}: {info}, tile visits and host waits {grid.route_fields_counts()}")
    assert keys.shape == want.shape
    assert not (keys == SENTINEL).any(), f"{name}: {np.count_nonzero(keys == SENTINEL)} keys were not written"
    for r in range(want.shape[0]):
        assert np.array_equal(keys[r], want[r]), f"{name}: layer {r}: {np.count_nonzero(keys[r] != want[r])} keys differ at {np.argwhere(keys[r] != want[r])[:4]}"
        if not used[r]:
            assert (keys[r] == R.NONE).all()
    assert info["converged"] == 1
    _check_info(info, want, used, name)


def test_a_layer_that_ends_early_does_not_end_the_call(grid, want_fields):
    """the shut-in seed's layer has nothing to do after its first round; the shared word keeps the rounds going for the other"""
    name, src, stride, p = CASES[IDS.index("serpentine_and_a_cell")]
    keys, info = _call(grid, src, stride, seeds=p["seeds"], max_rounds=1024)
    assert info["reached"][:2] == [int(np.count_nonzero(R.serpentine() == 0)), 1] and info["rounds"] > 8 and info["converged"] == 1
    assert keys[1, 100, 100] == 1 and np.count_nonzero(keys[1] != R.NONE) == 1 and keys[0, 100, 100] == R.NONE


# ---- 3. the device's own identity, and the two results side by side
@pytest.mark.parametrize("name", ["sixteen_seeds", "two_seeds_one_cell", "seeds_ignored", "random_0.15_97x130"])
def test_minimum_over_the_layers_is_the_route_image_and_neither_touches_the_other(grid, name):
    _, src, stride, p = CASES[IDS.index(name)]
    H_, W = src.shape
    kw = dict(seeds=p["seeds"], free_max=p["free_max"], weights=p["w"], limit=p["limit"])
    buf = _upload(grid, src, stride)
    try:
        joint, jinfo = grid.route_of(buf.ptr, W, H_, stride, **kw)
        keys, info = grid.route_fields_of(buf.ptr, W, H_, stride, **kw)
        assert np.array_equal(keys.min(axis=0), joint) and info["seeds_used"] == jinfo["seeds_used"]
        assert np.array_equal(grid.route_keys(), joint), "the fields call changed the route result"
        assert grid.route_dev_ptrs()[0] != grid.route_fields_dev_ptrs()[0]
        # another route call, with one seed: the fields stay
        one, _ = grid.route_of(buf.ptr, W, H_, stride, **dict(kw, seeds=p["seeds"][-1:]))
        assert np.array_equal(grid.route_fields_keys(), keys), "a route call changed the fields result"
        assert grid.route_fields_dev_ptrs()[1:] == (W, H_, len(p["seeds"]))
        has = one != R.NONE
        assert np.array_equal(one[has] >> 4, keys[-1][has] >> 4) and np.array_equal(has, keys[-1] != R.NONE)
    finally:
        buf.free()


# ---- 4. out of rounds
@pytest.mark.parametrize("sweeps", [0, 1], ids=["default_sweeps", "one_sweep"])
def test_serpentine_out_of_rounds(grid, want_fields, sweeps):
    name, src, stride, p = CASES[IDS.index("serpentine_and_a_cell")]
    want, _ = want_fields[name]
    grid.set_route_sweeps(sweeps)
    try:
        keys, info = _call(grid, src, stride, seeds=p["seeds"], max_rounds=4)
    finally:
        grid.set_route_sweeps(0)
    assert info["converged"] == 0 and info["rounds"] == 4 and info["seeds_used"] == 2 and info["layers"] == 2
    assert not (keys == SENTINEL).any() and (keys >= want).all() and (keys[0] != want[0]).any()
    assert keys[0, 16, 8] == want[0, 16, 8] == 0 and keys[1, 100, 100] == want[1, 100, 100] == 1
    assert np.array_equal(keys[1], want[1])
    assert info["reached"][:2] == [int(np.count_nonzero(keys[0] != R.NONE)), 1]


# ---- 5. one context, many calls
def test_repeated_calls_keep_the_scratch(grid):
    large, small = R.random_map(256, 256, 0.15, 5), R.random_map(33, 33, 0.15, 6)
    w = R.random_weights(9)
    ptrs = []
    for src, n in ((large, 3), (small, 3), (large, 2), (large, 3)):
        H_, W = src.shape
        seeds = [(W // 2, H_ // 2), (3, 3), (W - 2, 1)][:n]
        keys, info = _call(grid, src, W, seeds=seeds, free_max=50, weights=w)
        want, used = RF.fields(src, seeds, 50, w)
        assert np.array_equal(keys, want) and info["converged"] == 1
        _check_info(info, want, used, (W, n))
        ptrs.append(grid.route_fields_dev_ptrs()[0])
    assert len(set(ptrs)) == 1, "the scratch of the largest call was not kept"


def test_argument_errors_leave_the_previous_result(grid):
    src = R.corner_wall(64, 64, False)
    buf = _upload(grid, src, 64)
    try:
        keys, _ = grid.route_fields_of(buf.ptr, 64, 64, 64, seeds=[(5, 5), (40, 40)])
        lib, h = grid.lib, grid.h
        info = capi.RouteFieldsInfo()
        info.layers = info.rounds = -7
        xy = (C.c_int32 * 2)(5, 5)
        w0 = (C.c_uint8 * 3)(1, 0, 1)

        def prm(free_max=0, n_seeds=1, seeds=xy, weights=None, limit=0, max_rounds=0):
            return C.byref(capi.RouteParams(free_max, n_seeds, seeds, weights, limit, max_rounds))

        def dev(ptr=buf.ptr, W=64, H_=64, stride=64, p=None, i=C.byref(info)):
            return lib.tsd_route_fields_dev(h, C.c_void_p(ptr), W, H_, stride, prm() if p is None else p, i)

        assert dev(ptr=0) == -1 and b"tsd_route_fields_dev" in lib.tsd_last_error(h)
        assert lib.tsd_route_fields_dev(h, C.c_void_p(buf.ptr), 64, 64, 64, None, C.byref(info)) == -1
        assert dev(i=None) == -1
        for W, H_ in ((0, 64), (64, 0), (-1, 64), (32769, 1), (1, 32769)):
            assert dev(W=W, H_=H_, stride=max(W, 64)) == -1, (W, H_)
        assert dev(stride=63) == -1
        bad = (prm(free_max=-1), prm(free_max=100), prm(free_max=2, weights=w0), prm(limit=capi.ROUTE_MAX_DIST + 1), prm(n_seeds=0),
               prm(n_seeds=17), prm(seeds=None), prm(max_rounds=-1), prm(max_rounds=(1 << 20) + 1))
        for k, b in enumerate(bad):
            assert dev(p=b) == -1, k
            assert lib.tsd_route_fields_frame(h, 0, b, C.byref(info)) == -1, k
        assert lib.tsd_route_fields_frame(h, 0, prm(), C.byref(info)) == -1 and b"no completed frame" in lib.tsd_last_error(h)
        assert lib.tsd_route_fields_frame(h, 2, prm(), C.byref(info)) == -1
        assert (info.layers, info.rounds) == (-7, -7)
        assert np.array_equal(grid.route_fields_keys(), keys) and grid.route_fields_dev_ptrs()[1:] == (64, 64, 2)
    finally:
        buf.free()


# ---- 6. the goal matrix
def _unreached(m):
    """`m` with a clear cell in the unknown room at (50, 10): a frontier of one cell that no robot reaches"""
    m = m.copy()
    assert (m[9:12, 49:52] == U).all()
    m[10, 50] = 0
    return m


def _goal_maps():
    convoy, cseeds, _, _ = RF.convoy()
    rooms, rseeds, _ = V.two_rooms()
    out = [("convoy", convoy, cseeds, 0, 1), ("two_rooms", rooms, rseeds, 0, 1), ("convoy_unreached", _unreached(convoy), cseeds, 0, 1),
           ("convoy_min_size_2", _unreached(convoy), cseeds, 0, 2)]
    by = {c[0]: c for c in R.cases()}
    _, src, _, p = by["random_0.05_97x130"]
    out.append(("random_3_seeds", src, p["seeds"][:3], 50, 1))
    out.append(("random_3_seeds_min_size_3", src, p["seeds"][:3], 50, 3))
    _, src, _, p = by["sixteen_seeds"]
    out.append(("random_16_seeds", src, p["seeds"], 50, 2))
    return out


GOAL_MAPS = _goal_maps()


@pytest.mark.parametrize("case", GOAL_MAPS, ids=[c[0] for c in GOAL_MAPS])
def test_goal_matrix(grid, case):
    name, src, seeds, free_max, min_size = case
    H_, W = src.shape
    buf = _upload(grid, src, W + 7)
    try:
        rec, lab, _ = grid.frontiers_of(buf.ptr, W, H_, W + 7, free_max=free_max, min_size=min_size, seeds=seeds)
        keys, info = grid.route_fields_of(buf.ptr, W, H_, W + 7, seeds=seeds, free_max=free_max)
    finally:
        buf.free()
    got = grid.route_fields_goals()
    want_rec, want_lab, _ = F.frontiers(src, free_max, min_size, seeds)
    want_keys, _ = RF.fields(src, seeds, free_max)
    want = RF.goal_matrix(want_keys, want_lab, want_rec)
    assert rec.tobytes() == want_rec.tobytes() and np.array_equal(keys, want_keys)
    assert got.shape == want.shape == (len(seeds), rec.size) and got.dtype == want.dtype and rec.size > 0
    assert got.tobytes() == want.tobytes(), f"{name}: {np.argwhere(got != want)[:4]}"
    for r in range(len(seeds)):
        assert set(got[r]["seed"].tolist()) <= {r, -1}
    if name == "convoy":
        assert got["cell"].tolist() == [[2318, 2328, 2360]] * 2 and got["dist"].tolist() == [[34, 84, 244], [74, 124, 284]]
    if name == "convoy_unreached":
        assert rec.size == 4 and (got["cell"] == R.NONE).any(axis=0).tolist() == [True, False, False, False]
    if "min_size" in name:
        assert rec.size < F.frontiers(src, free_max, 1, seeds)[0].size, "min_size dropped no root: the case tests nothing"
    # a row at a time and in parts, like tsd_route_goals_fetch
    part = np.zeros(1, dtype=capi.ROUTE_GOAL_DTYPE)
    assert grid.lib.tsd_route_fields_goals_fetch(grid.h, len(seeds) - 1, rec.size - 1, 1, part.ctypes.data) == 0
    assert part[0].tobytes() == want[-1, -1].tobytes()
    assert grid.lib.tsd_route_fields_goals_fetch(grid.h, len(seeds), 0, 1, part.ctypes.data) == -1
    assert grid.lib.tsd_route_fields_goals_fetch(grid.h, -1, 0, 1, part.ctypes.data) == -1
    assert grid.lib.tsd_route_fields_goals_fetch(grid.h, 0, rec.size, 1, part.ctypes.data) == -1


def test_goal_matrix_refusals():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        n = C.c_int(-7)
        part = np.zeros(1, dtype=capi.ROUTE_GOAL_DTYPE)
        with pytest.raises(capi.TsdError):
            g.route_fields_dev_ptrs()
        with pytest.raises(capi.TsdError):
            g.route_fields_counts()
        assert g.lib.tsd_route_fields_goals(g.h, C.byref(n)) == -1 and b"tsd_route_fields_goals: no route result" in g.lib.tsd_last_error(g.h)
        m, seeds, _, _ = RF.convoy()
        buf = _upload(g, m)
        try:
            # a route result is no fields result
            g.route_of(buf.ptr, 64, 48, 64, seeds=seeds)
            assert g.lib.tsd_route_fields_goals(g.h, C.byref(n)) == -1 and b"no route result" in g.lib.tsd_last_error(g.h)
            g.route_fields_of(buf.ptr, 64, 48, 64, seeds=seeds)
            assert g.lib.tsd_route_fields_goals(g.h, C.byref(n)) == -1 and b"no frontier result" in g.lib.tsd_last_error(g.h)
            assert g.lib.tsd_route_fields_goals_fetch(g.h, 0, 0, 0, part.ctypes.data) == -1
            other = _upload(g, np.zeros((16, 16), dtype=np.int8))
            try:
                g.frontiers_of(other.ptr, 16, 16, 16)
            finally:
                other.free()
            assert g.lib.tsd_route_fields_goals(g.h, C.byref(n)) == -1 and b"differ in size" in g.lib.tsd_last_error(g.h) and n.value == -7
            assert g.lib.tsd_route_fields_goals(g.h, None) == -1
            g.frontiers_of(buf.ptr, 64, 48, 64)
            assert g.route_fields_goals().shape == (2, 3)
        finally:
            buf.free()
    finally:
        g.close()


# ---- 7. paths and waypoints on mixed layers
def _mixed_goals(keys, seeds, per_layer, rng):
    """per layer its seed's own cell and `per_layer` cells with a key, all layers interleaved"""
    L, H_, W = keys.shape
    cells, layers = [], []
    for r in range(L):
        flat = np.nonzero(keys[r].ravel() != R.NONE)[0]
        if flat.size == 0:
            continue
        pick = [seeds[r][1] * W + seeds[r][0]] + [int(c) for c in rng.choice(flat, size=per_layer, replace=False)]
        cells += pick
        layers += [r] * len(pick)
    order = rng.permutation(len(cells))
    return np.array(cells, dtype=np.uint32)[order], np.array(layers, dtype=np.uint8)[order]


def test_paths_and_waypoints_on_mixed_layers(grid, want_fields):
    name, src, stride, p = CASES[IDS.index("sixteen_seeds")]
    H_, W = src.shape
    want, _ = want_fields[name]
    wi = R.weight_image(src, p["free_max"], p["w"])
    buf = _upload(grid, src, stride)
    try:
        keys, _ = grid.route_fields_of(buf.ptr, W, H_, stride, seeds=p["seeds"], free_max=p["free_max"], weights=p["w"])
    finally:
        buf.free()
    assert np.array_equal(keys, want)
    cells, layers = _mixed_goals(want, p["seeds"], 2, np.random.default_rng(7))
    assert set(layers.tolist()) == set(range(16)) and cells.size == 48
    # an obstacle has no key on any layer; a cell outside the map
    blocked = int(np.nonzero(wi.ravel() == 0)[0][0])
    cells = np.concatenate([cells, np.array([blocked, W * H_], dtype=np.uint32)])
    layers = np.concatenate([layers, np.array([15, 3], dtype=np.uint8)])
    paths, lens = grid.route_fields_paths(cells, layers, 4096)
    want_paths, want_lens = RF.trace(want, wi, cells, layers, 4096)
    assert np.array_equal(lens, want_lens) and lens[-2:].tolist() == [0, 0] and (lens[:-2] >= 1).all() and (lens == 1).sum() >= 16
    for g, (a, b) in enumerate(zip(paths, want_paths)):
        assert a.tolist() == b, g
        if lens[g] > 0:
            assert a[-1] == p["seeds"][layers[g]][1] * W + p["seeds"][layers[g]][0], "a path ends on its own layer's seed"
    # the same cells on the layer after: other paths to another seed
    shifted = ((layers.astype(np.int64) + 1) % 16).astype(np.uint8)
    paths2, lens2 = grid.route_fields_paths(cells, shifted, 4096)
    want_paths2, want_lens2 = RF.trace(want, wi, cells, shifted, 4096)
    assert np.array_equal(lens2, want_lens2) and [a.tolist() for a in paths2] == want_paths2 and not np.array_equal(lens, lens2)
    # a cut at max_len = 3
    cut, lens3 = grid.route_fields_paths(cells, layers, 3)
    assert np.array_equal(lens3, want_lens) and [a.tolist() for a in cut] == [q[:3] for q in want_paths]
    # the waypoints of the same goals
    for lookahead, slack in ((24, 0), (8, 300)):
        ways, info = grid.route_fields_waypoints(cells, layers, lookahead=lookahead, slack=slack, max_len=4096, max_way=256)
        want_ways, want_info = RF.waypoints(want, wi, cells, layers, lookahead, slack, 4096)
        assert info.tobytes() == want_info.tobytes(), (lookahead, slack, np.argwhere(info != want_info)[:4])
        assert [a.tolist() for a in ways] == [b.tolist() for b in want_ways]
        assert (info["n_way"][:-2] >= 1).all() and (info["n_way"] == 1).sum() >= 16 and (info["n_way"] > 2).any()


def test_a_goal_without_a_key_on_its_layer(grid, want_fields):
    """the shut-in cell has a key on layer 1 only, the corridor on layer 0 only"""
    name, src, stride, p = CASES[IDS.index("serpentine_and_a_cell")]
    want, _ = want_fields[name]
    keys, _ = _call(grid, src, stride, seeds=p["seeds"], max_rounds=1024)
    assert np.array_equal(keys, want)
    room, corridor = 100 * 256 + 100, 16 * 256 + 40
    cells, layers = [room, room, corridor, corridor], [0, 1, 0, 1]
    paths, lens = grid.route_fields_paths(cells, layers, 64)
    assert lens.tolist() == [0, 1, 33, 0] and paths[1].tolist() == [room] and paths[2][-1] == 16 * 256 + 8
    ways, info = grid.route_fields_waypoints(cells, layers, lookahead=64, max_len=64, max_way=8)
    want_ways, want_info = RF.waypoints(want, R.weight_image(src), cells, layers, 64, 0, 64)
    assert info.tobytes() == want_info.tobytes() and [a.tolist() for a in ways] == [b.tolist() for b in want_ways]
    assert info["len"].tolist() == [0, 1, 33, 0] and info["n_way"].tolist() == [0, 1, 2, 0]
    assert info["dist"].tolist() == [R.NONE, 0, 160, R.NONE]


def test_trace_refusals_leave_the_outputs(grid):
    src = np.zeros((33, 33), dtype=np.int8)
    buf = _upload(grid, src)
    try:
        grid.route_fields_of(buf.ptr, 33, 33, 33, seeds=[(1, 1), (30, 30), (5, 20)])
    finally:
        buf.free()
    lib, h = grid.lib, grid.h
    cells = (C.c_uint32 * 2)(0, 40)
    ok, bad = (C.c_uint8 * 2)(0, 2), (C.c_uint8 * 2)(0, 3)
    paths, lens = (C.c_uint32 * 8)(*([7] * 8)), (C.c_int32 * 2)(-7, -7)
    way, info = (C.c_uint32 * 8)(*([7] * 8)), np.full(2, -7, dtype=WP.INFO_DTYPE)
    prm = capi.WaypointParams(16, 0, 64, 4)
    for layers, who in ((bad, b"layer"), (None, b"goal_layers is NULL")):
        assert lib.tsd_route_fields_trace(h, cells, layers, 2, 4, paths, lens) == -1
        assert b"tsd_route_fields_trace" in lib.tsd_last_error(h) and who in lib.tsd_last_error(h)
        assert lib.tsd_route_fields_waypoints(h, cells, layers, 2, C.byref(prm), way, info.ctypes.data) == -1
        assert b"tsd_route_fields_waypoints" in lib.tsd_last_error(h) and who in lib.tsd_last_error(h)
    for args in ((None, ok, 2, 4, paths, lens), (cells, ok, 0, 4, paths, lens), (cells, ok, 4097, 4, paths, lens), (cells, ok, 2, 0, paths, lens),
                 (cells, ok, 2, 4, None, lens), (cells, ok, 2, 4, paths, None)):
        assert lib.tsd_route_fields_trace(h, *args) == -1, args[2:4]
    assert list(paths) == [7] * 8 and list(lens) == [-7, -7] and list(way) == [7] * 8 and (info["len"] == -7).all()
    assert lib.tsd_route_fields_trace(h, cells, ok, 2, 4, paths, lens) == 0 and list(lens) == [2, 20]
    assert lib.tsd_route_fields_waypoints(h, cells, ok, 2, C.byref(prm), way, info.ctypes.data) == 0 and info["len"].tolist() == [2, 20]
    # without a fields result
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        assert g.lib.tsd_route_fields_trace(g.h, cells, ok, 2, 4, paths, lens) == -1 and b"no route result" in g.lib.tsd_last_error(g.h)
        assert g.lib.tsd_route_fields_waypoints(g.h, cells, ok, 2, C.byref(prm), way, info.ctypes.data) == -1
    finally:
        g.close()


# ---- 8. the assignment across robots
def _plan(m, seeds, free_max=0, min_size=1):
    rec, lab, _ = F.frontiers(m, free_max, min_size, seeds)
    keys, _ = RF.fields(m, seeds, free_max)
    return RF.goal_matrix(keys, lab, rec)


def _assign_cases():
    """[(name, map, goal matrix, R, gain_weight, free_max, unknown_depth)]"""
    out = []
    m, seeds, _, matrix = RF.convoy()
    out.append(("convoy", m, matrix, 10, 1, 0, 0))
    out.append(("convoy_four_robots_three_frontiers", m, _plan(m, seeds + [(20, 43), (60, 41)]), 10, 1, 0, 0))
    rooms, rseeds, _ = V.two_rooms()
    out.append(("two_rooms", rooms, _plan(rooms, rseeds), 10, 1, 0, 0))
    out.append(("two_rooms_gain_weight_40_depth_2", rooms, _plan(rooms, rseeds), 12, 40, 0, 2))
    _, src, _, p = {c[0]: c for c in R.cases()}["sixteen_seeds"]
    for n, min_size in ((2, 3), (3, 3), (16, 4)):
        out.append((f"random_97x130_{n}_robots", src, _plan(src, p["seeds"][:n], 50, min_size), 6, 25, 50, 1))
    out.append(("no_frontiers", m, np.zeros((2, 0), dtype=R.GOAL_DTYPE), 10, 1, 0, 0))
    known = np.zeros((33, 33), dtype=np.int8)
    every_gain_0 = np.zeros((2, 2), dtype=R.GOAL_DTYPE)
    every_gain_0[0] = [(40, 10, 0, 0), (50, 20, 0, 0)]
    every_gain_0[1] = [(40, 30, 1, 0), (50, 5, 1, 0)]
    out.append(("every_gain_0", known, every_gain_0, 5, 3, 0, 0))
    return out


ASSIGN = _assign_cases()


@pytest.fixture(scope="module")
def want_assign():
    return {name: RF.assign_fields(m, goals, R_, gw, free_max, depth) for name, m, goals, R_, gw, free_max, depth in ASSIGN}


@pytest.mark.parametrize("case", ASSIGN, ids=[c[0] for c in ASSIGN])
def test_view_assign_fields(grid, want_assign, case):
    name, m, goals, R_, gw, free_max, depth = case
    H_, W = m.shape
    want_of, want_picked, want_rounds, want_claims = want_assign[name]
    buf = _upload(grid, m, W + 5)
    try:
        grid.view_claims_reset(W, H_)
        grid.view_claim_of(buf.ptr, W, H_, W + 5, [0, W * H_ // 2 + W // 2], R_, free_max)      # stale claims: the call resets them
        goal_of, picked, rounds = grid.view_assign_fields_of(buf.ptr, W, H_, W + 5, goals, R_, gw, free_max, depth)
        claims = grid.view_claims()
        print(f"{name}: {goals.shape} goals, goal_of_robot {goal_of.tolist()}, rounds {rounds}")
        assert goal_of.tolist() == want_of.tolist() and rounds == want_rounds
        assert picked.tobytes() == want_picked.tobytes()
        assert claims.shape == (H_, W) and np.array_equal(claims, want_claims)
        n_robots, n_frontiers = goals.shape
        assert rounds <= min(n_robots, n_frontiers)
        given = goal_of[goal_of >= 0]
        assert len(set(given.tolist())) == given.size, "a frontier was given twice"
        if name == "convoy":
            assert goal_of.tolist() == [0, 1] and rounds == 2
            # the joint field on the same context: the rear robot is offered nothing
            grid.frontiers_of(buf.ptr, W, H_, W + 5, seeds=[(12, 42), (4, 42)])
            grid.route_of(buf.ptr, W, H_, W + 5, seeds=[(12, 42), (4, 42)])
            joint_of, _, joint_rounds = grid.view_assign_of(buf.ptr, W, H_, W + 5, grid.route_goals(), 2, R_, gw)
            assert joint_of.tolist() == [0, -1] and joint_rounds == 1
            # and the device's own matrix is the one the restatement assigned from
            grid.route_fields_of(buf.ptr, W, H_, W + 5, seeds=[(12, 42), (4, 42)])
            assert grid.route_fields_goals().tobytes() == goals.tobytes()
        if name == "convoy_four_robots_three_frontiers":
            assert (goal_of >= 0).sum() == 3 and (goal_of == -1).sum() == 1
        if name in ("no_frontiers", "every_gain_0"):
            assert (goal_of == -1).all() and not claims.any() and rounds == (0 if name == "no_frontiers" else 1)
            assert (picked["cell"] == R.NONE).all()
        if name.startswith("random"):
            assert (goal_of >= 0).sum() >= min(2, n_robots) and n_frontiers >= 2
    finally:
        buf.free()


def test_view_assign_fields_refusals_leave_the_claims(grid):
    m, _, _, matrix = RF.convoy()
    H_, W = m.shape
    buf = _upload(grid, m)
    try:
        grid.view_assign_fields_of(buf.ptr, W, H_, W, matrix, 10, 1)
        before = grid.view_claims()
        assert before.any()
        lib, h = grid.lib, grid.h
        goal_of, rounds = (C.c_int32 * 17)(*([-7] * 17)), C.c_int(-7)

        def call(ptr=buf.ptr, W_=W, stride=W, prm=None, goals=matrix.ctypes.data, n_f=3, n_r=2, of=goal_of, rounds_=C.byref(rounds)):
            prm = capi.ViewParams(0, 10, 0, 0) if prm is None else prm
            return lib.tsd_view_assign_fields(h, C.c_void_p(ptr), W_, H_, stride, C.byref(prm), goals, n_f, n_r, 1, of, None, rounds_)

        for k, kw in enumerate((dict(W_=0), dict(stride=W - 1), dict(prm=capi.ViewParams(0, 0, 0, 0)), dict(prm=capi.ViewParams(0, 512, 0, 0)),
                                dict(prm=capi.ViewParams(100, 10, 0, 0)), dict(prm=capi.ViewParams(0, 10, -1, 0)), dict(goals=None),
                                dict(n_f=-1), dict(n_f=4097), dict(n_r=0), dict(n_r=17), dict(of=None), dict(rounds_=None))):
            assert call(**kw) == -1, k
            assert b"tsd_view_assign_fields" in lib.tsd_last_error(h), k
        assert list(goal_of) == [-7] * 17 and rounds.value == -7
        assert np.array_equal(grid.view_claims(), before)
        assert call() == 0 and list(goal_of)[:2] == [0, 1] and rounds.value == 2
    finally:
        buf.free()


# ---- 9. the frame forms: a pushed grid
GC = synth.GridConfig(8, 0.1)
GEO = synth.ScanGeometry.full_circle_360()
SHORT_RANGE = 3.0


def _push(oracle, dg, world, pose3):
    x, y, yaw = pose3
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, GEO), SHORT_RANGE, GEO.angle_increment)
    dg.push(synth.pose_matrix(x, y, yaw), data, mask, GEO.angle_increment, GEO.angle_min, SHORT_RANGE, H.MIN_RANGE, H.LOW_REFL,
            want_stats=False)


def test_fields_of_a_frame_and_its_refusals(oracle):
    world = synth.World("room", GC)
    dg = capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)
    try:
        for source in ("map", "costmap"):
            with pytest.raises(capi.TsdError):
                dg.route_fields(source, seeds=[(5, 5)])      # no frame yet
            assert dg.last_rc == -1
        poses = [(world.cx - world.hx + 2.0 + 0.3 * k, world.cy - world.hy + 1.5, 0.1 + 0.02 * k) for k in range(6)]
        for pose in poses:
            _push(oracle, dg, world, pose)
        dg.map_frame_begin(False, 2, image=False)
        with pytest.raises(capi.TsdError):
            dg.route_fields("map", seeds=[(5, 5)])           # a frame in flight
        assert dg.last_rc == -1
        occ, _, _ = dg.map_frame_wait()
        ys, xs = np.nonzero(occ == 0)
        assert xs.size > 100 and (occ == -1).sum() > 100
        d2 = (xs - poses[0][0] / GC.cell_size) ** 2 + (ys - poses[0][1] / GC.cell_size) ** 2
        near, far = int(np.argmin(d2)), int(np.argmax(d2))
        seeds = [(int(xs[near]), int(ys[near])), (0, 0), (int(xs[far]), int(ys[far]))]      # (0, 0): an unknown corner
        with pytest.raises(capi.TsdError):
            dg.route_fields("costmap", seeds=seeds)          # a frame, but no cost map yet
        keys, info = dg.route_fields("map", seeds=seeds)
        want, used = RF.fields(occ, seeds)
        assert np.array_equal(keys, want) and info["converged"] == 1 and used == [1, 0, 1]
        _check_info(info, want, used, "map")
        assert info["reached"][0] > 100 and info["reached"][1] == 0
        # the matrix of the frame's frontiers, the paths of both robots to the same cells
        rec, lab, _ = dg.frontiers(min_size=4, seeds=seeds)
        goals = dg.route_fields_goals()
        assert goals.tobytes() == RF.goal_matrix(want, lab, rec).tobytes() and (goals[1]["cell"] == R.NONE).all()
        both = np.nonzero((goals[0]["cell"] != R.NONE) & (goals[2]["cell"] != R.NONE))[0]
        assert both.size > 0
        cells = np.concatenate([goals[0]["cell"][both], goals[2]["cell"][both]])
        layers = np.array([0] * both.size + [2] * both.size, dtype=np.uint8)
        paths, lens = dg.route_fields_paths(cells, layers, 512)
        want_paths, want_lens = RF.trace(want, R.weight_image(occ), cells, layers, 512)
        assert np.array_equal(lens, want_lens) and [a.tolist() for a in paths] == want_paths
        # the cost map of the same frame
        dg.costmap_begin(6)
        for source in ("map", "costmap"):
            with pytest.raises(capi.TsdError):
                dg.route_fields(source, seeds=seeds)         # a cost map in flight
        cost, _ = dg.costmap_wait()
        w = dg.route_weights(98, 40)
        keys, info = dg.route_fields("costmap", seeds=seeds, free_max=98, weights=w)
        want, used = RF.fields(cost, seeds, 98, w)
        assert np.array_equal(keys, want) and info["converged"] == 1
        _check_info(info, want, used, "costmap")
        assert (cost != occ).any() and info["reached"][0] > 100
    finally:
        dg.close()


# ---- 10. the facade: SlamFleet.explore_dispatch
def _node(**over):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over.update(occ_grid_time_interval=1000.0)
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    return gc, geo, scans, over


def _metres(cells, width, origin, res):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([((cells % width) + 0.5) * res + origin[0], ((cells // width) + 0.5) * res + origin[1]], axis=-1).reshape(-1, 2)


def test_fleet_explore_dispatch():
    """two nodes in the same room, their grids 24 / -16 cells apart: every piece of the dispatch against the restatement on the
    merged map and against the lower calls on the context that carried it"""
    from ohm_tsd_slam_amd import facade
    gc, geo, scans, over = _node(frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        with pytest.raises(capi.TsdError):
            fleet.explore_dispatch(1.0, 1, 1.0)            # no merged map yet
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        data, W = m["data"], m["width"]
        seeds = []
        for n in nodes:
            pose = n.pose_msg()["position"]
            seeds.append(tuple(int(np.floor((pose[a] - m["origin_position"][a]) / m["resolution"])) for a in (0, 1)))
        out = fleet.explore_dispatch(view_radius_m=1.0, gain_weight=3, lookahead_m=1.5, slack=0, unknown_depth=2, min_size=3, max_len=2048,
                                     max_way=64)
        R_, look = out["radius_cells"], out["lookahead_cells"]
        assert R_ == int(round(1.0 / m["resolution"])) and look == int(round(1.5 / m["resolution"]))
        assert out["frontiers"]["seeds"] == seeds and out["resolution"] == m["resolution"]
        assert np.array_equal(out["origin"], m["origin_position"][:2])
        # against the restatement on the published map
        want_rec, want_lab, used = F.frontiers(data, 0, 3, seeds)
        keys, used_by = RF.fields(data, seeds)
        matrix = RF.goal_matrix(keys, want_lab, want_rec)
        want_of, want_picked, want_rounds, _ = RF.assign_fields(data, matrix, R_, 3, 0, 2)
        assert out["frontiers"]["records"].tobytes() == want_rec.tobytes() and out["frontiers"]["seeds_used"] == used == 2
        assert out["goals"].shape == (2, want_rec.size) and out["goals"].tobytes() == matrix.tobytes()
        assert out["goal_of_robot"].tolist() == want_of.tolist() and out["rounds"] == want_rounds
        assert out["picked"].tobytes() == want_picked.tobytes()
        assert (want_of >= 0).all() and want_of[0] != want_of[1], "the scene gives both nodes a frontier: the case tests nothing otherwise"
        assert out["fields"]["layers"] == 2 and out["fields"]["converged"] == 1 and out["fields"]["used"][:2] == used_by
        layers = [r for r in range(2) if want_of[r] >= 0]
        cells = [int(matrix[r, want_of[r]]["cell"]) for r in layers]
        for r in range(2):
            assert out["goal"][r].tobytes() == matrix[r, want_of[r]].tobytes()
        want_ways, want_info = RF.waypoints(keys, R.weight_image(data), cells, layers, look, 0, 2048)
        for k, r in enumerate(layers):
            assert out["waypoint_info"][r].tobytes() == want_info[k].tobytes()
            assert out["waypoint_cells"][r].tolist() == want_ways[k].tolist()
            assert np.array_equal(out["waypoints"][r], _metres(want_ways[k], W, m["origin_position"], m["resolution"]))
            assert out["waypoint_cells"][r][0] == seeds[r][1] * W + seeds[r][0] and out["waypoint_cells"][r][-1] == cells[k]
        # against the lower calls: member 0's context carried the call and still holds the frontier and the fields result
        g = nodes[0].grid()
        assert g.route_fields_goals().tobytes() == out["goals"].tobytes()
        ways, info = g.route_fields_waypoints(cells, layers, lookahead=look, slack=0, max_len=2048, max_way=64)
        for k, r in enumerate(layers):
            assert info[k].tobytes() == out["waypoint_info"][r].tobytes() and ways[k].tolist() == out["waypoint_cells"][r].tolist()
        # a result of a merged map that has been published over is not handed out
        counts, finfo = (C.c_int * 6)(), capi.RouteFieldsInfo()
        seeds_out, origin_cs = np.zeros(32, dtype=np.int32), np.zeros(3)
        lib = fleet.lib
        assert lib.tsd_fleet_explore_dispatch(fleet.h, 3, 1.0, 3, 2, 1.5, 0, 2048, 64, counts, C.byref(finfo), seeds_out.ctypes.data,
                                              origin_cs.ctypes.data_as(C.POINTER(C.c_double))) == 0
        goal_of = np.full(2, -7, dtype=np.int32)
        assert lib.tsd_fleet_explore_dispatch_fetch(fleet.h, None, None, goal_of.ctypes.data, None, None, None) == 0
        assert goal_of.tolist() == want_of.tolist()
        fleet.publish_merged_map()
        goal_of[:] = -7
        assert lib.tsd_fleet_explore_dispatch_fetch(fleet.h, None, None, goal_of.ctypes.data, None, None, None) == -1
        assert goal_of.tolist() == [-7, -7]
        again = fleet.explore_dispatch(1.0, 3, 1.5, unknown_depth=2, min_size=3, max_len=2048, max_way=64)
        assert again["goal_of_robot"].tolist() == want_of.tolist()
        # refusals of the arguments
        for kw in (dict(unknown_depth=-1), dict(max_len=0), dict(max_way=0)):
            with pytest.raises(capi.TsdError):
                fleet.explore_dispatch(1.0, 3, 1.5, **kw)
    finally:
        fleet.close()
        for n in nodes:
            n.close()
