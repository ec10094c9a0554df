"""Views on the device (csrc/view.hip; tsd_view_gains / _claim / _claims_reset / _claims_dev_ptr / _assign, the facade's explore_gains
and explore_assign) against the restatement of tests/view_ref.py: every comparison is byte for byte -- the records, the claims image,
the assignment.  The maps are those of tests/test_cpu_view.py, where the restatement is checked against a scalar ray-by-ray statement
of the rule and the named numbers of the room and the diagonal wall are asserted."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, facade, synth
from tests import frontier_ref as F
from tests import helpers as H
from tests import route_ref as R
from tests import view_ref as V

pytestmark = pytest.mark.gpu

CASES = V.cases()
IDS = [c[0] for c in CASES]
U, O = V.U, V.O


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def wants():
    """the restatement's records per case, computed once and left unchanged"""
    out = {name: V.gains(m, p["cells"], p["R"], p["free_max"], p["unknown_depth"]) for name, m, _, p in CASES}
    for rec in out.values():
        rec.setflags(write=False)
    return out


def _upload(grid, src, stride=None):
    """the map as `height` rows of `stride` bytes on the device; the padding holds -1s (read, they would count as unknown cells)"""
    H_, W = src.shape
    stride = W if stride is None else stride
    padded = np.full((H_, stride), -1, dtype=np.int8)
    padded[:, :W] = src
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    return buf


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert got.tobytes() == want.tobytes(), f"{what}: {bad.size} records differ, first {bad[:3]}: {got[bad[:3]]} for {want[bad[:3]]}"


# ---- every drawn and random map
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gains_equal_the_restatement(grid, wants, case):
    name, m, stride, p = case
    H_, W = m.shape
    buf = _upload(grid, m, stride)
    try:
        got = grid.view_gains_of(buf.ptr, W, H_, stride, p["cells"], p["R"], p["free_max"], p["unknown_depth"])
    finally:
        buf.free()
    _same(got, wants[name], name)
    cells = np.array(p["cells"], dtype=np.uint32)
    for c in np.unique(cells):                            # the same cell twice in one call: equal records
        assert len({bytes(r) for r in got[cells == c]}) == 1, (name, c)
    for k in np.nonzero(cells >= W * H_)[0]:
        assert tuple(got[k]) == (cells[k], 0, 0, 0)


@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("open_")], ids=lambda c: c[0])
def test_open_map_closed_form(grid, case):
    """all unknown but the candidate: the whole disc is seen, clipped at the map's border"""
    name, m, stride, p = case
    H_, W = m.shape
    c = p["cells"][-1]
    buf = _upload(grid, m, stride)
    try:
        got = grid.view_gains_of(buf.ptr, W, H_, stride, [c], p["R"])[0]
    finally:
        buf.free()
    n = V.disc_cells(W, H_, c % W, c // W, p["R"])
    assert tuple(got) == (c, n - 1, n - 1, n), (name, got, n)


def test_named_numbers_on_the_device(grid):
    """the room, its door and the diagonal wall"""
    c = 10 * 21 + 10
    for door, depth, want in ((False, 0, (c, 0, 0, 81)), (True, 0, (c, 7, 7, 89)), (True, 2, (c, 2, 2, 84))):
        buf = _upload(grid, V.room(door))
        try:
            assert tuple(grid.view_gains_of(buf.ptr, 21, 21, 21, [c], 20, 0, depth)[0]) == want
        finally:
            buf.free()
    for anti in (True, False):
        m = V.diagonal_wall(41, anti)
        c = 5 * 41 + (5 if anti else 35)
        buf = _upload(grid, m)
        try:
            rec = grid.view_gains_of(buf.ptr, 41, 41, 41, [c], 31)[0]
        finally:
            buf.free()
        yy, xx = np.nonzero(V.view(m, c, 31))
        side = (xx + yy < 40) if anti else (xx > yy)
        assert side.all() and rec["visible"] == xx.size and rec["gain"] == 0


@pytest.mark.parametrize("n", [1, V.MAX_CELLS])
def test_one_and_the_most_candidates(grid, n):
    m = R.random_map(97, 130, 0.05, 12)
    rng = np.random.default_rng(n)
    cells = rng.integers(0, 97 * 130 + 10, size=n).astype(np.uint32)
    buf = _upload(grid, m)
    try:
        got = grid.view_gains_of(buf.ptr, 97, 130, 97, cells, 2, 50, 1)
    finally:
        buf.free()
    _same(got, V.gains(m, cells, 2, 50, 1), f"n = {n}")


# ---- claims
FOG = CASES[IDS.index("fog_97x130_R64_depth0")][1]


@pytest.mark.parametrize("shape", ["97x130", "64x64_stride_72"])
def test_claims_equal_the_restatement(grid, shape):
    if shape == "97x130":
        m, stride, Rr, depth = FOG, 97, 33, 3
        first, second = [65 * 97 + 50, 60 * 97 + 40, 0], [66 * 97 + 58, 129 * 97 + 96, 97 * 130, 65 * 97 + 50]
    else:
        m, stride, Rr, depth = R.random_map(64, 64, 0.05, 21), 72, 16, 0
        m[m == 0] = U
        first, second = [20 * 64 + 20, 63], [24 * 64 + 28, 40 * 64 + 40]
    H_, W = m.shape
    probe = first + second + [10 * W + 10, (H_ - 1) * W]
    buf = _upload(grid, m, stride)
    try:
        grid.view_claims_reset(W, H_)
        ptr = grid.view_claims_dev_ptr()
        assert ptr[1:] == (W, H_) and not grid.view_claims().any()
        want = np.zeros((H_, W), dtype=np.uint8)
        _same(grid.view_gains_of(buf.ptr, W, H_, stride, probe, Rr, 50, depth, use_claims=True), V.gains(m, probe, Rr, 50, depth, want), "no claims yet")
        grid.view_claim_of(buf.ptr, W, H_, stride, first, Rr, 50, depth)
        V.claim(m, want, first, Rr, 50, depth)
        assert want.any() and np.array_equal(grid.view_claims(), want)
        grid.view_claim_of(buf.ptr, W, H_, stride, first[::-1], Rr, 50, depth)                  # a second claim changes nothing
        assert np.array_equal(grid.view_claims(), want)
        got = grid.view_gains_of(buf.ptr, W, H_, stride, probe, Rr, 50, depth, use_claims=True)
        _same(got, V.gains(m, probe, Rr, 50, depth, want), "claimed once")
        assert got[0]["gain"] == 0 and got[0]["unknown"] > 0 and (got["gain"] < got["unknown"]).sum() >= 3
        _same(grid.view_gains_of(buf.ptr, W, H_, stride, probe, Rr, 50, depth), V.gains(m, probe, Rr, 50, depth), "claims not in use")
        grid.view_claim_of(buf.ptr, W, H_, stride, second, Rr, 50, depth)                       # overlapping views
        V.claim(m, want, second, Rr, 50, depth)
        assert np.array_equal(grid.view_claims(), want)
        _same(grid.view_gains_of(buf.ptr, W, H_, stride, probe, Rr, 50, depth, use_claims=True), V.gains(m, probe, Rr, 50, depth, want), "claimed twice")
        grid.view_claims_reset(W, H_)
        assert grid.view_claims_dev_ptr() == ptr and not grid.view_claims().any()
    finally:
        buf.free()


# ---- the assignment
def _device_goals(grid, buf, W, H_, stride, seeds, free_max, min_size=1):
    grid.frontiers_of(buf.ptr, W, H_, stride, free_max=free_max, min_size=min_size, seeds=seeds)
    grid.route_of(buf.ptr, W, H_, stride, seeds=seeds, free_max=free_max)
    return grid.route_goals()


def _check_assign(grid, buf, m, stride, goals, n_robots, Rr, weight, free_max=0, depth=0):
    H_, W = m.shape
    got = grid.view_assign_of(buf.ptr, W, H_, stride, goals, n_robots, Rr, weight, free_max, depth)
    want_of, want_picked, want_rounds, want_claims = V.assign(m, goals, n_robots, Rr, weight, free_max, depth)
    assert np.array_equal(got[0], want_of) and got[2] == want_rounds, (got, want_of, want_rounds)
    _same(got[1], want_picked, "picked")
    assert np.array_equal(grid.view_claims(), want_claims)
    return got


def test_assign_two_rooms(grid):
    m, seeds, want_goals = V.two_rooms()
    H_, W = m.shape
    buf = _upload(grid, m, 72)
    try:
        goals = _device_goals(grid, buf, W, H_, 72, seeds, 0)
        assert goals.tobytes() == want_goals.tobytes()
        of, picked, rounds = _check_assign(grid, buf, m, 72, goals, 2, 12, 10)
        assert of.tolist() == [0, 2] and rounds == 2                       # the second robot is sent to the other room
        of, _, _ = _check_assign(grid, buf, m, 72, goals, 2, 12, 0)
        assert of.tolist() == [0, 1]                                       # by distance alone: both look into the first room
        _check_assign(grid, buf, m, 72, goals, 2, 12, 10, depth=2)
        of, picked, rounds = _check_assign(grid, buf, m, 72, goals, 1, 12, 10)     # one robot: robot 1's goals are not remaining
        assert of.tolist() == [0] and rounds == 1
        of, picked, rounds = _check_assign(grid, buf, m, 72, goals[:0], 2, 12, 10)
        assert of.tolist() == [-1, -1] and rounds == 0 and (picked["cell"] == V.NONE).all()
    finally:
        buf.free()


def test_assign_random_map_four_seeds(grid):
    m = R.random_map(97, 130, 0.03, 31)
    rng = np.random.default_rng(32)
    m[rng.random(m.shape) < 0.10] = U
    m[:, 60:] = np.where(rng.random((130, 37)) < 0.7, U, m[:, 60:])
    ys, xs = np.nonzero((m >= 0) & (m <= 50))
    pick = rng.choice(xs.size, size=4, replace=False)
    seeds = [(int(xs[i]), int(ys[i])) for i in pick]
    buf = _upload(grid, m)
    try:
        goals = _device_goals(grid, buf, 97, 130, 97, seeds, 50, min_size=2)
        usable = goals[(goals["cell"] != R.NONE)]
        assert usable.size >= 4 and np.unique(usable["seed"]).size >= 2
        for weight, depth in ((0, 0), (3, 0), (50, 3)):
            of, picked, rounds = _check_assign(grid, buf, m, 97, goals, 4, 20, weight, 50, depth)
            assert (of >= 0).sum() >= 2 and rounds >= 2
        _check_assign(grid, buf, m, 97, goals, 2, 20, 3, 50)                # seeds 2 and 3 are no robots of this call
    finally:
        buf.free()


# ---- one context, many calls
def test_repeated_calls_keep_the_scratch(grid):
    large, small = R.random_map(256, 256, 0.02, 5), R.random_map(33, 33, 0.02, 6)
    large[large < 30], small[small < 30] = U, U
    grid.view_claims_reset(256, 256)
    ptr = grid.view_claims_dev_ptr()[0]
    out = []
    for m in (large, small, large):
        H_, W = m.shape
        cells = [(H_ // 2) * W + W // 2, 3 * W + 3, W * H_ - 2]
        buf = _upload(grid, m)
        try:
            grid.view_claims_reset(W, H_)
            assert grid.view_claims_dev_ptr() == (ptr, W, H_), "the claims image of the large call was not kept"
            grid.view_claim_of(buf.ptr, W, H_, W, cells[:1], 33, 50)
            got = grid.view_gains_of(buf.ptr, W, H_, W, cells, 33, 50, use_claims=True)
        finally:
            buf.free()
        want_claims = V.claim(m, np.zeros(m.shape, dtype=np.uint8), cells[:1], 33, 50)
        _same(got, V.gains(m, cells, 33, 50, 0, want_claims))
        assert np.array_equal(grid.view_claims(), want_claims)
        out.append(got)
    assert out[0].tobytes() == out[2].tobytes()


def test_argument_errors_leave_the_claims(grid):
    m = V.room(True)
    buf = _upload(grid, m)
    try:
        grid.view_claims_reset(21, 21)
        grid.view_claim_of(buf.ptr, 21, 21, 21, [10 * 21 + 10], 20)
        ptr, claims = grid.view_claims_dev_ptr(), grid.view_claims()
        assert claims.sum() == 7
        lib, h = grid.lib, grid.h
        cells = (C.c_uint32 * 2)(220, 0)
        many = (C.c_uint32 * 4097)()
        out = (capi.ViewGain * 4097)()
        out[0].visible = 77
        goal = np.zeros(1, dtype=capi.ROUTE_GOAL_DTYPE)
        goal[0] = (220, 5, 0, 0)
        of, rounds = (C.c_int32 * 2)(-7, -7), C.c_int(-7)

        def prm(free_max=0, radius=20, depth=0, use=0):
            return C.byref(capi.ViewParams(free_max, radius, depth, use))

        def gains(ptr_=buf.ptr, W=21, H_=21, stride=21, p=None, c=cells, n=2, o=out):
            return lib.tsd_view_gains(h, C.c_void_p(ptr_), W, H_, stride, prm() if p is None else p, c, n, o)

        def claim(ptr_=buf.ptr, W=21, H_=21, stride=21, p=None, c=cells, n=2):
            return lib.tsd_view_claim(h, C.c_void_p(ptr_), W, H_, stride, prm() if p is None else p, c, n)

        def assign(ptr_=buf.ptr, W=21, H_=21, stride=21, p=None, g=goal.ctypes.data, n=1, robots=1, o=of, r=C.byref(rounds)):
            return lib.tsd_view_assign(h, C.c_void_p(ptr_), W, H_, stride, prm() if p is None else p, g, n, robots, 1, o, None, r)

        assert lib.tsd_view_gains(h, C.c_void_p(buf.ptr), 21, 21, 21, None, cells, 2, out) == -1 and b"params is NULL" in lib.tsd_last_error(h)
        assert lib.tsd_view_claim(h, C.c_void_p(buf.ptr), 21, 21, 21, None, cells, 2) == -1
        assert gains(c=None) == -1 and gains(o=None) == -1 and claim(c=None) == -1
        for n in (0, -1, 4097):
            assert gains(c=many, n=n) == -1 and claim(c=many, n=n) == -1, n
        bad = (prm(radius=0), prm(radius=512), prm(radius=-3), prm(free_max=-1), prm(free_max=100), prm(depth=-1))
        for k, b in enumerate(bad):
            assert gains(p=b) == -1 and claim(p=b) == -1 and assign(p=b) == -1, k
            assert lib.tsd_view_gains(h, None, 0, 0, 0, b, cells, 2, out) == -1, k
        for W, H_ in ((0, 21), (21, 0), (-1, 21), (32769, 1), (1, 32769)):
            assert gains(W=W, H_=H_, stride=max(W, 21)) == -1 and claim(W=W, H_=H_, stride=max(W, 21)) == -1, (W, H_)
            assert assign(W=W, H_=H_, stride=max(W, 21)) == -1 and lib.tsd_view_claims_reset(h, W, H_) == -1, (W, H_)
        assert gains(stride=20) == -1 and claim(stride=20) == -1 and assign(stride=20) == -1
        # claims in use, or a claim, on a map of another size than the image
        assert gains(W=20, H_=21, p=prm(use=1)) == -1 and b"claims image" in lib.tsd_last_error(h)
        assert gains(W=21, H_=20, p=prm(use=1)) == -1 and claim(W=20) == -1 and claim(H_=20) == -1
        # the assignment's own arguments
        assert assign(g=None) == -1 and assign(n=-1) == -1 and assign(n=4097) == -1 and assign(robots=0) == -1 and assign(robots=17) == -1
        assert assign(o=None) == -1 and assign(r=None) == -1
        # the frame forms without a frame
        assert lib.tsd_view_gains(h, None, 0, 0, 0, prm(), cells, 2, out) == -1 and b"no completed frame" in lib.tsd_last_error(h)
        assert lib.tsd_view_claim(h, None, 0, 0, 0, prm(), cells, 2) == -1 and assign(ptr_=None) == -1
        assert out[0].visible == 77 and list(of) == [-7, -7] and rounds.value == -7
        assert grid.view_claims_dev_ptr() == ptr and np.array_equal(grid.view_claims(), claims)
        assert gains(p=prm(use=1)) == 0 and (out[0].cell, out[0].gain, out[0].unknown, out[0].visible) == (220, 0, 7, 89)
        assert gains(p=prm(free_max=99, radius=511, depth=1 << 30)) == 0
    finally:
        buf.free()


def test_no_claims_before_the_first_reset():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        with pytest.raises(capi.TsdError):
            g.view_claims_dev_ptr()
        buf = _upload(g, V.room(True))
        try:
            with pytest.raises(capi.TsdError):
                g.view_claim_of(buf.ptr, 21, 21, 21, [220], 20)
            with pytest.raises(capi.TsdError):
                g.view_gains_of(buf.ptr, 21, 21, 21, [220], 20, use_claims=True)
            assert tuple(g.view_gains_of(buf.ptr, 21, 21, 21, [220], 20)[0]) == (220, 7, 7, 89)
            with pytest.raises(capi.TsdError):
                g.view_claims_dev_ptr()
        finally:
            buf.free()
    finally:
        g.close()


# ---- the frame forms: a pushed grid
GC = synth.GridConfig(8, 0.1)
GEO = synth.ScanGeometry.full_circle_360()
SHORT_RANGE = 3.0


def _push(oracle, dg, world, pose3):
    x, y, yaw = pose3
    data, mask = oracle.ingest_f32(world.scan(x, y, yaw, GEO), SHORT_RANGE, GEO.angle_increment)
    dg.push(synth.pose_matrix(x, y, yaw), data, mask, GEO.angle_increment, GEO.angle_min, SHORT_RANGE, H.MIN_RANGE, H.LOW_REFL,
            want_stats=False)


def test_views_of_a_frame_and_their_refusals(oracle):
    world = synth.World("room", GC)
    dg = capi.TsdGridDevice(GC.map_size_log2, GC.cell_size, GC.max_trunc)
    try:
        with pytest.raises(capi.TsdError):
            dg.view_gains([5], 10)                           # no frame yet
        assert dg.last_rc == -1
        poses = [(world.cx - world.hx + 2.0 + 0.3 * k, world.cy - world.hy + 1.5, 0.1 + 0.02 * k) for k in range(6)]
        for pose in poses:
            _push(oracle, dg, world, pose)
        dg.map_frame_begin(False, 2, image=False)
        N = 1 << GC.map_size_log2
        dg.view_claims_reset(N, N)
        for call in (lambda: dg.view_gains([5], 10), lambda: dg.view_claim([5], 10),
                     lambda: dg.view_assign(np.zeros(0, dtype=capi.ROUTE_GOAL_DTYPE), 1, 10, 1)):
            with pytest.raises(capi.TsdError):
                call()                                       # a frame in flight
            assert dg.last_rc == -1
        occ, _, _ = dg.map_frame_wait()
        assert occ.shape == (N, N) and (occ == 0).sum() > 100 and (occ == -1).sum() > 100
        ys, xs = np.nonzero(occ == 0)
        k = np.argmin((xs - poses[0][0] / GC.cell_size) ** 2 + (ys - poses[0][1] / GC.cell_size) ** 2)
        seeds = [(int(xs[k]), int(ys[k])), (int(xs[k]) + 3, int(ys[k]))]
        dg.frontiers(min_size=4, seeds=seeds)
        dg.route("map", seeds=seeds)
        goals = dg.route_goals()
        cells = goals["cell"][goals["cell"] != R.NONE]
        assert cells.size >= 1
        for radius, depth in ((35, 0), (35, 2), (140, 0)):
            got = dg.view_gains(cells, radius, 0, depth)
            _same(got, V.gains(occ, cells, radius, 0, depth), f"frame, R = {radius}")
        assert got["gain"].max() > 10
        of, picked, rounds = dg.view_assign(goals, 2, 35, 4)
        want_of, want_picked, want_rounds, want_claims = V.assign(occ, goals, 2, 35, 4)
        assert np.array_equal(of, want_of) and rounds == want_rounds and (of >= 0).any()
        _same(picked, want_picked, "picked")
        assert np.array_equal(dg.view_claims(), want_claims)
        dg.view_claim(cells[:1], 140)
        V.claim(occ, want_claims, cells[:1], 140)
        assert np.array_equal(dg.view_claims(), want_claims)
        _same(dg.view_gains(cells, 140, use_claims=True), V.gains(occ, cells, 140, 0, 0, want_claims), "frame, claims")
        dg.costmap_begin(6)
        with pytest.raises(capi.TsdError):
            dg.view_gains(cells, 35)                         # a cost map in flight
        dg.costmap_wait()
    finally:
        dg.close()


# ---- the facade: SlamNode.explore_gains, SlamFleet.explore_assign
def _node(**over):
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over.update(occ_grid_time_interval=1000.0)
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    return gc, geo, scans, over


def _radius_cells(radius_m, m):
    return min(V.MAX_RADIUS, max(1, int(np.floor(radius_m / m["resolution"] + 0.5))))


def test_node_explore_gains():
    gc, geo, scans, over = _node(frontier_min_size=3)
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        with pytest.raises(capi.TsdError):
            node.explore_gains(2.0)                        # no plan yet
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m = node.map_msg()
        plan = node.explore_plan()
        goals = plan["goals"]
        assert goals.size >= 1 and (goals["cell"] != R.NONE).any()
        for radius_m, depth in ((2.0, 0), (3.5, 3), (1000.0, 0), (0.0, 0)):
            got = node.explore_gains(radius_m, depth)
            Rc = _radius_cells(radius_m, m)
            assert node.view_radius_cells == Rc
            _same(got, V.gains(m["data"], goals["cell"], Rc, 0, depth), f"radius {radius_m} m")
        assert got.size == goals.size and node.explore_gains(3.5)["gain"].max() > 0
        node.publish_map()                                 # the plan is of the map published before
        with pytest.raises(capi.TsdError):
            node.explore_gains(2.0)
        node.explore_plan()
        node.explore_gains(2.0)
    finally:
        node.close()


def test_fleet_explore_assign():
    """two nodes in the same room, their grids 24 / -16 cells apart: the assignment on the merged map equals the restatement's, fed
    with the plan's goals"""
    gc, geo, scans, over = _node(frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        with pytest.raises(capi.TsdError):
            fleet.explore_assign(2.0, 4)                   # no plan yet
        goals = fleet.explore_plan(min_size=2)["goals"]
        assert (goals["seed"] >= 0).any()
        for radius_m, weight, depth in ((2.0, 4, 0), (2.0, 0, 0), (3.5, 50, 2)):
            out = fleet.explore_assign(radius_m, weight, depth)
            Rc = _radius_cells(radius_m, m)
            want_of, want_picked, want_rounds, _ = V.assign(m["data"], goals, 2, Rc, weight, 0, depth)
            assert out["radius_cells"] == Rc and out["rounds"] == want_rounds and np.array_equal(out["goal_of_robot"], want_of)
            _same(out["picked"], want_picked, "picked")
        assert (out["goal_of_robot"] >= 0).any()
        fleet.publish_merged_map()
        with pytest.raises(capi.TsdError):
            fleet.explore_assign(2.0, 4)                   # the plan is of the merged map published before
    finally:
        fleet.close()
        for n in nodes:
            n.close()
