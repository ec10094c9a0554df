"""The live layer on the device (csrc/drive.hip; tsd_drive_live_* and reason 7 of the three rollouts) against the restatement of
tests/drive_live_ref.py: every comparison is byte for byte -- the layer's words, the choice records, the scores and `why` of every
sample, the tracks, and the words of sentinel-filled outputs a call must not write."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_live_ref as LR
from tests import drive_ref as DR
from tests import route_fields_ref as RF
from tests import route_ref as RR
from tests import test_gpu_drive as GD
from tests import test_gpu_drive_fleet as GF

pytestmark = pytest.mark.gpu

H = DR.H
CELL = 65536
S64, S16, TAIL, T64 = GD.S64, GD.S16, GD.TAIL, GF.T64
S32 = 0xA5A5A5A5


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cases():
    out = DR.cases()
    out["lanes_300x24"] = _lanes()
    return out


def _lanes():
    """300 x 24, free but for two cells: rows a robot at x = 2 drives along at one cell per step, up to 256 steps"""
    m = np.zeros((24, 300), dtype=np.int8)
    m[19, 12] = RR.O                                          # beside row 18: a body point one cell to the left meets it at k = 10
    m[21, 20] = RR.O                                          # on row 21: the centre enters it at k = 18
    goals = [(298, 1), (1, 22)]
    keys, fields = RR.route(m, goals)[0], RF.fields(m, goals)[0]
    for a in (keys, fields):
        a.setflags(write=False)
    return dict(map=m, wi=RR.weight_image(m), keys=keys, fields=fields, goals=goals, free_max=0, w=None, limit=0)


# ---- the layer
def _set_raw(grid, pts, r, W, Hh, skip=None, null=(), n=None, n_skip=None):
    """one tsd_drive_live_set: (rc, n_kept -- -77 where the call left it alone)"""
    p = np.ascontiguousarray(pts if pts is not None else [], dtype=np.int32).reshape(-1, 2)
    s = np.ascontiguousarray(skip if skip is not None else [], dtype=np.int32).reshape(-1, 3)
    prm = capi.DriveLiveParams(int(r), s.shape[0] if n_skip is None else n_skip,
                               None if "skip" in null or not s.shape[0] else s.ctypes.data_as(C.POINTER(C.c_int32)))
    kept = C.c_int(-77)
    rc = grid.lib.tsd_drive_live_set(grid.h, None if "params" in null else C.byref(prm), None if "points" in null or not p.shape[0] else p.ctypes.data,
                                     p.shape[0] if n is None else n, W, Hh, None if "kept" in null else C.byref(kept))
    return rc, kept.value


def _fetch(grid, W, Hh):
    """the layer's words through tsd_drive_live_fetch into a sentinel-filled buffer: uint32 (Hh, stride_words)"""
    sw = LR.stride_words(W)
    buf = np.full(sw * Hh + TAIL, S32, dtype=np.uint32)
    w, h, s = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = grid.lib.tsd_drive_live_fetch(grid.h, buf.ctypes.data, sw * Hh, C.byref(w), C.byref(h), C.byref(s))
    assert rc == 0 and (w.value, h.value, s.value) == (W, Hh, sw), grid.lib.tsd_last_error(grid.h)
    assert (buf[sw * Hh:] == S32).all(), "words beyond the layer were written"
    return buf[:sw * Hh].reshape(Hh, sw)


def _check_stamp(grid, pts, r, W, Hh, skip=None, what=""):
    want, n = LR.stamp(pts, r, W, Hh, skip)
    rc, kept = _set_raw(grid, pts, r, W, Hh, skip)
    assert rc == 0, (what, grid.lib.tsd_last_error(grid.h))
    got = _fetch(grid, W, Hh)
    assert got.tobytes() == LR.pack(want).tobytes(), (what, "bits", np.argwhere(LR.unpack(got, W) != want)[:4])
    assert kept == n, (what, kept, n)
    return want


@pytest.mark.parametrize("size", LR.STAMP_MAPS, ids=lambda s: "%dx%d" % s)
def test_stamp_equals_the_restatement(grid, size):
    """corners, word edges, the map's borders from outside, far points and duplicates at every radius, set after set on one image:
    each set has to remove what the one before it wrote"""
    W, Hh = size
    for r in (0, 1, 2, 63, 64, 1):
        pts = LR.stamp_points(W, Hh, r)
        want = _check_stamp(grid, pts, r, W, Hh, what=f"{size} r {r}")
        assert want[0, 0] and want[Hh - 1, W - 1]
        if r == 63:                                           # the far end alone, then nothing at all
            _check_stamp(grid, [(W - 1, Hh - 1), (W + 5, 0)], r, W, Hh, what=f"{size} the far end")
            assert not _check_stamp(grid, [(W + r, 0), (-r - 1, 0), (0, Hh + r), (0, -r - 1)], r, W, Hh, what=f"{size} outside by r + 1").any()
            assert _check_stamp(grid, [(-r, 0), (W - 1 + r, Hh - 1)], r, W, Hh, what=f"{size} outside by r").sum() == (1 if W * Hh == 1 else 2)


def test_point_counts_and_duplicates(grid):
    rng = np.random.default_rng(20)
    W, Hh = 97, 64
    assert not _check_stamp(grid, [], 5, W, Hh, what="n = 0").any()
    assert _check_stamp(grid, [(50, 30)], 2, W, Hh, what="n = 1").sum() == 13
    many = np.stack([rng.integers(-70, W + 70, 32768), rng.integers(-70, Hh + 70, 32768)], axis=1)
    many[::7] = many[0]                                       # duplicates
    _check_stamp(grid, many, 2, W, Hh, what="n = 32768, r 2")
    _check_stamp(grid, many[:9], 2, W, Hh, what="fewer points: no old bit")
    sparse = np.stack([rng.integers(0, 4096, 32768), rng.integers(-3, 67, 32768)], axis=1)
    _check_stamp(grid, sparse[:2000], 64, 4096, 64, what="4096 x 64, r 64")
    _check_stamp(grid, sparse, 1, 4096, 64, what="4096 x 64, n = 32768")
    _check_stamp(grid, [(4095, 63), (4000, 0)], 64, 4096, 64, what="4096 x 64: the far end alone")
    rc, kept = _set_raw(grid, many, 2, W, Hh, n=32769)
    assert rc == -1 and kept == -77


def test_skip_discs(grid):
    W, Hh = 45, 37
    pts = [(10, 10), (13, 14), (13, 15), (20, 20), (20, 20), (40, 3), (-2, 5)]
    rim = [(10, 10, 5), (20, 20, 0)]                          # (13, 14) on the rim: dropped; ro = 0 drops the point at its centre
    want = _check_stamp(grid, pts, 2, W, Hh, rim, "the rim")
    assert want[15, 13] and not want[10, 10] and not want[20, 20] and want[5, 0]
    sixteen = [(x, 3 * x % 37, x % 4) for x in range(0, 48, 3)]
    assert len(sixteen) == 16
    rng = np.random.default_rng(21)
    many = np.stack([rng.integers(-5, W + 5, 3000), rng.integers(-5, Hh + 5, 3000)], axis=1)
    _check_stamp(grid, many, 1, W, Hh, sixteen, "16 discs")
    every = [(p[0], p[1], 0) for p in pts[:6]] + [(-2, 5, 1 << 15)]
    assert not _check_stamp(grid, pts, 3, W, Hh, every, "every point dropped").any()
    far = [(1 << 30, 1 << 30), (-(1 << 30), 7), (5, 5)]
    _check_stamp(grid, far, 4, W, Hh, [((1 << 30) - 3, (1 << 30) - 4, 5), (-(1 << 30), -(1 << 30), 1 << 15)], "far discs and points")


def test_clear_set_again_and_the_block_is_kept(grid):
    W, Hh = 97, 64
    pts = LR.stamp_points(W, Hh, 3)
    _check_stamp(grid, pts, 3, W, Hh, what="first")
    p, w, h, s = C.c_void_p(), C.c_int(0), C.c_int(0), C.c_int(0)
    assert grid.lib.tsd_drive_live_dev_ptr(grid.h, C.byref(p), C.byref(w), C.byref(h), C.byref(s)) == 0 and (w.value, h.value, s.value) == (W, Hh, 4)
    first = p.value
    assert np.array_equal(grid.drive_live(), LR.stamp(pts, 3, W, Hh)[0])
    grid.drive_live_clear()
    grid.drive_live_clear()                                   # legal without a layer
    assert grid.drive_live() is None
    buf = np.full(8, S32, dtype=np.uint32)
    assert grid.lib.tsd_drive_live_fetch(grid.h, buf.ctypes.data, 8, None, None, None) == -1 and (buf == S32).all()
    assert grid.lib.tsd_drive_live_dev_ptr(grid.h, C.byref(p), None, None, None) == -1
    _check_stamp(grid, pts[:5], 1, W, Hh, what="after the clear")
    _check_stamp(grid, pts, 3, 33, 7, what="a smaller image in the same block")
    _check_stamp(grid, pts, 3, W, Hh, what="the first shape again")
    assert grid.lib.tsd_drive_live_dev_ptr(grid.h, C.byref(p), None, None, None) == 0 and p.value == first
    assert grid.drive_live_set(pts, 3, size=(W, Hh)) == len(pts)


def test_live_refusals_leave_the_layer_in_place(grid):
    W, Hh = 45, 37
    pts = [(10, 10), (44, 36), (0, 0)]
    want = _check_stamp(grid, pts, 2, W, Hh, what="before")
    far = 1 << 30
    bad = [dict(null=("params",)), dict(null=("points",)), dict(skip=[(1, 1, 1)], null=("skip",), n_skip=1), dict(n=-1), dict(n=32769), dict(r=-1), dict(r=65),
           dict(n_skip=-1), dict(n_skip=17), dict(W=0), dict(Hh=0), dict(W=32769), dict(Hh=32769), dict(pts=[(far + 1, 0)]), dict(pts=[(0, -far - 1)]),
           dict(skip=[(far + 1, 0, 1)]), dict(skip=[(0, 0, -1)]), dict(skip=[(0, 0, (1 << 15) + 1)])]
    for kw in bad:
        a = dict(dict(pts=pts, r=2, W=W, Hh=Hh), **kw)
        rc, kept = _set_raw(grid, a.pop("pts"), a.pop("r"), a.pop("W"), a.pop("Hh"), **a)
        assert rc == -1 and kept == -77 and b"tsd_drive_live_set" in grid.lib.tsd_last_error(grid.h), (kw, grid.lib.tsd_last_error(grid.h))
        assert _fetch(grid, W, Hh).tobytes() == LR.pack(want).tobytes(), kw
    buf = np.full(2 * Hh, S32, dtype=np.uint32)
    assert grid.lib.tsd_drive_live_fetch(grid.h, buf.ctypes.data, 2 * Hh - 1, None, None, None) == -1 and (buf == S32).all()
    assert _set_raw(grid, [(far, -far)], 64, W, Hh, [(far, far, 1 << 15)], null=("kept",))[0] == 0      # the values at their limits pass
    grid.drive_live_clear()


# ---- the rollouts
def _check(grid, c, form, live, poses, steps, step_q16, turn, what="", **kw):
    """GD._check against the restatement with the layer ``live`` (bool image or None), which the context must hold already"""
    keys = c["keys"] if form == "route" else c["fields"]
    want = LR.rollout_all(keys, c["wi"], live, poses, steps, step_q16, turn, **kw)
    rc, choice, sc, wh = GD._raw(grid, form, poses, steps, step_q16, turn, **kw)
    n = want[1].size
    assert rc == 0, (what, grid.lib.tsd_last_error(grid.h))
    assert wh[:n].tobytes() == want[2].tobytes(), (what, "why", np.argwhere(wh[:n].reshape(want[2].shape) != want[2])[:4])
    assert sc[:n].tobytes() == want[1].tobytes(), (what, "scores", np.argwhere(sc[:n].reshape(want[1].shape) != want[1])[:4])
    assert choice.tobytes() == want[0].tobytes(), (what, choice, want[0])
    assert (sc[n:] == S64).all() and (wh[n:] == S16).all(), (what, "words beyond the samples were written")
    return want


def _live(grid, c, pts, r, skip=None):
    Hh, W = c["wi"].shape
    return _check_stamp(grid, pts, r, W, Hh, skip, "the rollout's layer")


LANES = (3, 6, 9, 12, 15)


@pytest.mark.parametrize("form", ["route", "fields"])
@pytest.mark.parametrize("T", [1, 64, 65, 256])
def test_reason_7_at_the_round_edges(grid, cases, form, T):
    """a robot per row at x = 2, one cell per step: the live cell of row i is entered at k = 1, 63, 64, 65 and T"""
    c = cases["lanes_300x24"]
    GD._load(grid, c, route=form == "route", fields=form == "fields")
    ks = [1, 63, 64, 65, T]
    live = _live(grid, c, [(2 + k, y) for k, y in zip(ks, LANES)], 0)
    poses = [(2, y, 32768, 32768, 0, 0) for y in LANES] + [(2, 1, 32768, 32768, 0, 0)]
    want = _check(grid, c, form, live, poses, T, [65536, 32768], [0], f"lanes T {T}")
    assert want[2][:5, 0, 0].tolist() == [(7 << 12) | k if k <= T else 0 for k in ks] and want[2][5, 0, 0] == 0
    assert want[2][0, 1, 0] == (7 << 12) | 1                             # half a cell from the middle of a cell: the next one at k = 1 too
    assert (want[0]["admissible"] > 0).any()
    grid.drive_live_clear()


def test_reason_7_on_the_centre_and_on_body_points_0_and_63(grid, cases):
    c = cases["lanes_300x24"]
    GD._load(grid, c, fields=False)
    poses = [(2, y, 32768, 32768, 0, 0) for y in LANES[:3]]
    # the centre of row 3 at k = 30; two cells left of row 6 at k = 40 and of row 9 at k = 70: only the point at (0, 2) gets there
    live = _live(grid, c, [(32, 3), (42, 8), (72, 11)], 0)
    for at in (0, 63):
        body = [(0, 0)] * 64
        body[at] = (0, 2 * CELL)
        want = _check(grid, c, "route", live, poses, 100, [65536], [0], f"body point {at}", body=body)
        assert want[2][:, 0, 0].tolist() == [(7 << 12) | 30, (7 << 12) | 40, (7 << 12) | 70]
    want = _check(grid, c, "route", live, poses, 100, [65536], [0], "no body")
    assert want[2][:, 0, 0].tolist() == [(7 << 12) | 30, 0, 0]
    grid.drive_live_clear()


def test_reason_7_behind_4_and_ahead_of_2(grid, cases):
    c = cases["lanes_300x24"]
    GD._load(grid, c, fields=False)
    poses = [(2, 18, 32768, 32768, 0, 0), (2, 21, 32768, 32768, 0, 0)]
    beside = [(0, CELL)]                                      # row 18: the point meets (12, 19), w == 0, at k = 10; row 21: the centre (20, 21) at k = 18
    for pts, why in (([(12, 18), (20, 21)], [(4 << 12) | 10, (2 << 12) | 18]),          # at the same step 4 and 2 go first
                     ([(11, 18), (19, 21)], [(7 << 12) | 9, (7 << 12) | 17]),           # a step earlier 7 wins
                     ([(13, 18), (21, 21)], [(4 << 12) | 10, (2 << 12) | 18]),          # a step later it is never reached
                     ([(11, 19), (19, 22)], [(7 << 12) | 9, (7 << 12) | 17])):          # ... on the body point as on the centre
        live = _live(grid, c, pts, 0)
        want = _check(grid, c, "route", live, poses, 40, [65536], [0], f"orders {pts}", body=beside)
        assert want[2][:, 0, 0].tolist() == why, pts
    grid.drive_live_clear()


def test_every_sample_refused_by_7_and_freed_by_a_skip_disc(grid, cases):
    c = cases["open_45x37"]
    GD._load(grid, c)
    poses = [(20, 20, 32768, 32768, 0, 0), (30, 8, 0, 0, H // 3, 1)]
    prm = (10, GD._speeds(3), GD._turns(5, 40))
    pts = [(20, 20), (21, 20), (30, 8), (5, 30)]
    live = _live(grid, c, pts, 2)
    want = _check(grid, c, "fields", live, poses, *prm, "on live cells")
    assert (want[2] == (7 << 12) | 1).all() and (want[0]["speed"] == -1).all() and (want[0]["admissible"] == 0).all() and (want[1] == DR.DRIVE_NONE).all()
    live = _live(grid, c, pts, 2, skip=[(20, 20, 1), (30, 8, 0)])
    want = _check(grid, c, "fields", live, poses, *prm, "the robots' own discs skipped")
    assert (want[0]["speed"] >= 0).all() and live[30, 5] and not live[20, 20]
    grid.drive_live_clear()


@pytest.mark.parametrize("shape", [(20, 4, 5, 13, 40), (65, 64, 2, 3, 5), (256, 1, 3, 5, 2)], ids=lambda s: "T%d_B%d_V%d_W%d" % s[:4])
@pytest.mark.parametrize("name,form", [("door_96x64", "route"), ("random_67x50", "fields")])
def test_rollout_with_a_layer_equals_the_restatement(grid, cases, name, form, shape):
    """the shapes of test_gpu_drive.py with a layer of scattered discs: scores, `why`, the choice and k_drive_pick's record"""
    T, B, V, Wn, unit = shape
    c = cases[name]
    GD._load(grid, c, route=form == "route", fields=form == "fields")
    Hh, W = c["wi"].shape
    rng = np.random.default_rng(T)
    pts = np.stack([rng.integers(-2, W + 2, 60), rng.integers(-2, Hh + 2, 60)], axis=1)
    live = _live(grid, c, pts, 1)
    poses = GD._poses(c, 1 if form == "route" else c["fields"].shape[0])
    kw = dict(body=GD._body(B, 20000 if name.startswith("random") else 98304) if B else None, weights=(3, 2, 1, 5), nose_q16=3 * 65536 + 77, nose_miss=123)
    want = _check(grid, c, form, live, poses, T, GD._speeds(V), GD._turns(Wn, unit), f"{name} {shape}", **kw)
    reasons = sorted(set((want[2] >> 12).ravel().tolist()))
    print(f"{name} {form} {shape}: reasons {reasons}, admissible {want[0]['admissible'].tolist()}, blocked {LR.blocked_live(want[2]).tolist()}")
    assert 7 in reasons and (want[0]["admissible"] > 0).any()
    # the layer cleared and the call repeated: the bytes of the rule without it
    grid.drive_live_clear()
    GD._check(grid, c, form, poses, T, GD._speeds(V), GD._turns(Wn, unit), f"{name} {shape} cleared", **kw)


def test_sixteen_robots_on_mixed_layers_with_a_layer(grid, cases):
    c = cases["open_45x37"]
    GD._load(grid, c)
    cells = GD._free_cells(c, 16, 5)
    poses = [(x, y, (977 * k) % 65536, (313 * k) % 65536, (257 * k) % H, k % 3) for k, (x, y) in enumerate(cells)]
    kw = dict(body=GD._body(5, 30000), weights=(2, 1, 1, 3), nose_q16=2 * 65536, nose_miss=50)
    prm = (20, GD._speeds(4), GD._turns(7, 30))
    rng = np.random.default_rng(16)
    pts = np.stack([rng.integers(0, 45, 30), rng.integers(0, 37, 30)], axis=1)
    live = _live(grid, c, pts, 1, skip=[(x, y, 2) for x, y in cells])
    all16 = _check(grid, c, "fields", live, poses, *prm, "16 robots", **kw)
    assert (LR.blocked_live(all16[2]) > 0).sum() >= 8 and (all16[0]["admissible"][0::3] > 0).all()
    _check(grid, c, "route", live, poses, *prm, "the route form", **kw)
    for r in (0, 7, 15):                                      # each robot equal to its own single call
        one = _check(grid, c, "fields", live, [poses[r]], *prm, f"robot {r} alone", **kw)
        assert one[0][0].tobytes() == all16[0][r].tobytes()
    grid.drive_live_clear()


def test_a_layer_of_another_size_refuses_and_writes_nothing(grid, cases):
    c = cases["open_45x37"]
    GD._load(grid, c)
    poses = [(5, 5, 0, 0, 0, 0), (6, 5, 0, 0, 0, 1)]
    prm = (8, [65536, 0], [0, 7])
    block = None
    for W, Hh in ((46, 37), (45, 36), (37, 45)):
        assert _set_raw(grid, [(5, 5)], 1, W, Hh)[0] == 0
        for form, name in (("route", b"tsd_drive_rollout"), ("fields", b"tsd_drive_fields_rollout")):
            rc, choice, sc, wh = GD._raw(grid, form, poses, *prm)
            assert rc == -1 and name in grid.lib.tsd_last_error(grid.h) and b"live" in grid.lib.tsd_last_error(grid.h)
            assert choice.tobytes() == bytes([0xA5]) * choice.nbytes and (sc == S64).all() and (wh == S16).all()
        rc, choice, sc, wh, tr = GF._raw(grid, poses, *prm, [0, 1], CELL)
        assert rc == -1 and b"tsd_drive_fleet_rollout" in grid.lib.tsd_last_error(grid.h)
        assert choice.tobytes() == bytes([0xA5]) * choice.nbytes and (sc == S64).all() and (wh == S16).all() and (tr == T64).all()
    assert np.array_equal(grid.route_fields_keys(), c["fields"])
    live = _live(grid, c, [(7, 5)], 1)                        # the right size: the calls pass again
    _check(grid, c, "fields", live, poses, *prm, "after the refusals")
    grid.drive_live_clear()
    GD._check(grid, c, "fields", poses, *prm, "and without a layer")


# ---- the fleet form
def _check_fleet(grid, c, live, poses, steps, step_q16, turn, order, sep, what="", **kw):
    want = LR.fleet_rollout(c["fields"], c["wi"], live, poses, steps, step_q16, turn, order, sep, **kw)
    rc, choice, sc, wh, tr = GF._raw(grid, poses, steps, step_q16, turn, order, sep, **kw)
    n, nt = want[1].size, want[3].size
    assert rc == 0, (what, grid.lib.tsd_last_error(grid.h))
    assert wh[:n].tobytes() == want[2].tobytes(), (what, "why", np.argwhere(wh[:n].reshape(want[2].shape) != want[2])[:4])
    assert sc[:n].tobytes() == want[1].tobytes(), (what, "scores", np.argwhere(sc[:n].reshape(want[1].shape) != want[1])[:4])
    assert choice.tobytes() == want[0].tobytes(), (what, choice, want[0])
    assert tr[:nt].tobytes() == want[3].tobytes(), (what, "tracks", np.argwhere(tr[:nt].reshape(want[3].shape) != want[3])[:4])
    assert (sc[n:] == S64).all() and (wh[n:] == S16).all() and (tr[nt:] == T64).all(), (what, "words beyond the outputs were written")
    return want


def test_7_against_6_across_the_round_edge(grid, cases):
    """a mover per row at x = 2, one cell per step, and a robot parked at x = 67 or 68 with the separation one cell: reason 6 at k = 64
    or 65.  The live cell of the row is entered at the same step, a step earlier or a step later."""
    c = cases["lanes_300x24"]
    GD._load(grid, c, route=False)
    rows = [(3, 67, 64), (5, 67, 63), (7, 67, 65), (9, 68, 65), (11, 68, 64), (13, 68, 66)]        # (row, the parked robot's x, k of the live cell)
    movers = [(2, y, 32768, 32768, 0, 0) for y, _, _ in rows]
    parked = [(x, y, 32768, 32768, 0, -1) for y, x, _ in rows]
    extra = [(100, 20, 0, 0, 0, -1), (2, 22, 32768, 32768, 0, 1)]          # a robot parked ON a live cell, and a mover nothing stops
    live = _live(grid, c, [(2 + k, y) for y, _, k in rows] + [(100, 20)], 0)
    poses = movers + parked + extra
    want = _check_fleet(grid, c, live, poses, 100, [65536], [0], list(range(14)), CELL + 1, "7 against 6")
    assert want[2][:6, 0, 0].tolist() == [(7 << 12) | 64, (7 << 12) | 63, (6 << 12) | 64, (7 << 12) | 65, (7 << 12) | 64, (6 << 12) | 65]
    assert want[0][12]["speed"] == -1 and (want[2][12] == 0).all() and want[2][13, 0, 0] == 0 and want[0][13]["speed"] == 0
    for T, why in ((63, [0, (7 << 12) | 63]), (64, [(7 << 12) | 64, (7 << 12) | 63]), (65, [(7 << 12) | 64, (7 << 12) | 63])):
        four = [poses[0], poses[1], poses[6], poses[7]]
        assert _check_fleet(grid, c, live, four, T, [65536], [0], [3, 2, 1, 0], CELL + 1, f"T {T}")[2][:2].ravel().tolist() == why
    grid.drive_live_clear()
    GF._check(grid, c, poses, 100, [65536], [0], list(range(14)), CELL + 1, "cleared: the rule without the layer")


def test_without_separation_the_fleet_is_the_fields_rollout_with_the_layer(grid, cases):
    c = cases["random_67x50"]
    GD._load(grid, c, route=False)
    L = c["fields"].shape[0]
    poses = GF._cluster(c, 8, L, parked=(3,))
    rng = np.random.default_rng(8)
    pts = np.stack([rng.integers(20, 50, 12), rng.integers(12, 40, 12)], axis=1)
    live = _live(grid, c, pts, 1, skip=[(p[0], p[1], 1) for p in poses])
    kw = dict(body=GD._body(7, 20000), weights=(1, 1, 1, 1), nose_q16=CELL, nose_miss=9)
    prm = (65, GD._speeds(5), GD._turns(9, 20))
    zero = _check_fleet(grid, c, live, poses, *prm, GF._order(8, "shuffle"), 0, "sep 0", **kw)
    moving = [r for r in range(8) if poses[r][5] >= 0]
    old = _check(grid, c, "fields", live, [poses[r] for r in moving], *prm, "the fields form", **kw)
    assert old[0].tobytes() == zero[0][moving].tobytes() and np.array_equal(old[1], zero[1][moving]) and np.array_equal(old[2], zero[2][moving])
    assert (zero[2] >> 12 == 7).any() and zero[4].sum() == 0
    apart = _check_fleet(grid, c, live, poses, *prm, GF._order(8, "shuffle"), 3 * CELL, "sep 3", **kw)
    assert {6, 7} <= set((apart[2] >> 12).ravel().tolist())
    grid.drive_live_clear()


# ---- the facade: explore_drive with live points on the two-node scene of test_gpu_route_fields.py
def _cells(points, m):
    """the facade's conversion, restated: the map cell of a point in metres"""
    import math
    return [(math.floor((x - m["origin_position"][0]) / m["resolution"]), math.floor((y - m["origin_position"][1]) / m["resolution"])) for x, y in points]


def _centre(cell, m):
    return ((cell[0] + 0.5) * m["resolution"] + m["origin_position"][0], (cell[1] + 0.5) * m["resolution"] + m["origin_position"][1])


def _across(pose, choice, lists, m):
    """three points [m] across the arc `choice` takes from `pose`, at the first step four cells from the start: the arc's cell and
    the cells beside it"""
    tr = DR.trajectory(pose, lists["step_q16"][int(choice["speed"])], lists["turn"][int(choice["turn"])], lists["steps"])
    k = next(k for k in range(1, len(tr)) if max(abs(tr[k][3] - pose[0]), abs(tr[k][4] - pose[1])) >= 4)
    (x, y), (px, py) = tr[k][3:5], tr[k - 1][3:5]
    side = (0, 1) if y == py else (1, 0)
    return [_centre((x + s * side[0], y + s * side[1]), m) for s in (-1, 0, 1)]


def _same(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        assert v.tobytes() == b[k].tobytes() if k == "choice" else np.array_equal(v, b[k]), k


def test_node_explore_drive_with_live_points():
    import math
    from ohm_tsd_slam_amd import facade
    gc, geo, scans, over = GD._scene(frontier_min_size=3)
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m = node.map_msg()
        data, W, res = m["data"], m["width"], m["resolution"]
        Hm = data.shape[0]
        plan = node.explore_plan()
        goal = int(np.nonzero(plan["goals"]["cell"] != RR.NONE)[0][0])
        g = plan["goals"][goal]
        xyt = GD._xyt(node)
        foot = [(res, 0.0), (-res, 0.0), (0.0, res), (0.0, -res)]
        w_max = 40 * 2 * np.pi / (H * res / GD.DRIVE["v_max"])
        dt, lists = GD._lists(res, w_max, foot)
        kw = dict(GD.DRIVE, w_max=w_max, footprint=foot)
        today = node.explore_drive(goal, xyt, **kw)
        keys, _ = RR.route(data, [(int(g["cell"]) % W, int(g["cell"]) // W)], limit=int(g["dist"]) + GD.DRIVE["margin"])
        wi = RR.weight_image(data)
        pose = GD._drive_pose(xyt, m)
        assert today["choice"].tobytes() == DR.rollout(keys, wi, pose, **lists)[0].tobytes()
        pts = _across(pose, today["choice"], lists, m)
        radius = 1.4 * res                                    # to the nearest cell: 1
        out = node.explore_drive(goal, xyt, live_points=pts, live_radius_m=radius, **kw)
        live, kept = LR.stamp(_cells(pts, m), 1, W, Hm, skip=[(pose[0], pose[1], 0)])
        want = LR.rollout(keys, wi, live, pose, **lists)
        assert out["choice"].tobytes() == want[0].tobytes() and out["live_kept"] == kept == 3
        assert out["blocked_live"] == LR.blocked_live(want[2]) > 0
        assert out["choice"].tobytes() != today["choice"].tobytes() and (out["v"], out["w"]) != (today["v"], today["w"]) and out["admissible"] > 0
        assert node.grid().drive_live() is None               # the layer went with the call
        assert np.array_equal(node.grid().route_keys(), keys)
        _same(node.explore_drive(goal, xyt, **kw), today)     # live_points=None: today's answer
        _same(node.explore_drive(goal, xyt, live_points=None, live_radius_m=radius, **kw), today)
        none = node.explore_drive(goal, xyt, live_points=[], live_radius_m=radius, **kw)
        assert none["choice"].tobytes() == today["choice"].tobytes() and none["live_kept"] == 0 and none["blocked_live"] == 0
        # the robot's own body in its scan: without the disc nothing is admissible, with it the points go
        own = [_centre((pose[0] + dx, pose[1]), m) for dx in (-1, 0, 1)]
        stuck = node.explore_drive(goal, xyt, live_points=own + pts, live_radius_m=radius, **kw)
        assert stuck["live_kept"] == 5 and stuck["admissible"] == 0 and stuck["v"] == stuck["w"] == 0.0
        assert stuck["blocked_live"] == (LR.rollout(keys, wi, LR.stamp(_cells(own + pts, m), 1, W, Hm, [(pose[0], pose[1], 0)])[0], pose, **lists)[2] >> 12 == 7).sum()
        freed = node.explore_drive(goal, xyt, live_points=own + pts, live_radius_m=radius, live_skip_m=0.5 * res, **kw)       # rounded up: one cell
        assert freed["live_kept"] == 3 and freed["choice"].tobytes() == out["choice"].tobytes() and freed["blocked_live"] == out["blocked_live"]
        for bad in (dict(live_radius_m=-res), dict(live_radius_m=65 * res), dict(live_radius_m=float("nan")), dict(live_skip_m=-1.0),
                    dict(live_skip_m=float("inf")), dict(live_points=[(float("nan"), 0.0)]), dict(live_points=[(1e12, 0.0)]),
                    dict(live_points=np.zeros((32769, 2)))):
            with pytest.raises(capi.TsdError):
                node.explore_drive(goal, xyt, **dict(dict(kw, live_points=pts, live_radius_m=radius), **bad))
        assert node.grid().drive_live() is None
        _same(node.explore_drive(goal, xyt, **kw), today)
        assert math.isfinite(out["dt"])
    finally:
        node.close()


def test_fleet_explore_drive_with_live_points():
    import math
    from ohm_tsd_slam_amd import facade
    gc, geo, scans, over = GD._scene(frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        data, W, res = m["data"], m["width"], m["resolution"]
        Hm = data.shape[0]
        poses = [GD._xyt(n) for n in nodes]
        w_max = 40 * 2 * np.pi / (H * res / GD.DRIVE["v_max"])
        d = fleet.explore_dispatch(view_radius_m=1.0, gain_weight=3, lookahead_m=1.5, unknown_depth=2, min_size=3, max_len=2048, max_way=64)
        assert (d["goal_of_robot"] >= 0).all()
        for r in range(2):                                    # every node facing along the first segment of its way
            way = d["waypoints"][r]
            poses[r] = poses[r][:2] + (float(np.arctan2(way[1][1] - way[0][1], way[1][0] - way[0][0])),)
        dt, lists = GD._lists(res, w_max, [])
        kw = dict(GD.DRIVE, w_max=w_max)
        today = fleet.explore_drive(poses, **kw)
        seeds = [(int(c) % W, int(c) // W) for c in d["goal"]["cell"]]
        keys, _ = RF.fields(data, seeds, limit=int(d["goal"]["dist"].max()) + GD.DRIVE["margin"])
        wi = RR.weight_image(data)
        dposes = [GD._drive_pose(poses[r], m, r) for r in range(2)]
        # node 0's best arc crossed, and node 1's body as node 0's scanner sees it
        pts = _across(dposes[0], today[0]["choice"], lists, m)
        body = [_centre((dposes[1][0] + dx, dposes[1][1] + dy), m) for dx, dy in ((0, 0), (1, 0), (0, 1))]
        radius, skip = 1.4 * res, 0.9 * res                  # one cell each
        discs = [(p[0], p[1], 1) for p in dposes]
        live, kept = LR.stamp(_cells(pts + body, m), 1, W, Hm, skip=discs)
        out = fleet.explore_drive(poses, live_points=pts + body, live_radius_m=radius, live_skip_m=skip, **kw)
        want = LR.rollout_all(keys, wi, live, dposes, **lists)
        for r in range(2):
            assert out[r]["choice"].tobytes() == want[0][r].tobytes() and out[r]["live_kept"] == kept == 3
            assert out[r]["blocked_live"] == LR.blocked_live(want[2])[r] and "tracks" not in out[r]
        assert out[0]["blocked_live"] > 0 and out[0]["choice"].tobytes() != today[0]["choice"].tobytes() and out[0]["admissible"] > 0
        assert out[1]["admissible"] > 0 and out[1]["choice"]["speed"] >= 0          # the member under another's points still gets a command
        stuck = fleet.explore_drive(poses, live_points=pts + body, live_radius_m=radius, **kw)      # no skip radius: only the point ON a pose's cell goes
        assert stuck[1]["admissible"] == 0 and stuck[0]["live_kept"] == 5
        assert nodes[0].grid().drive_live() is None and np.array_equal(nodes[0].grid().route_fields_keys(), keys)
        # with a separation as well: 7 in front of 6
        apart = math.hypot(poses[0][0] - poses[1][0], poses[0][1] - poses[1][1])
        sep_m = apart + 2 * res
        sep = math.floor(sep_m / res * 65536.0 + 0.5)
        fkw = {k: v for k, v in lists.items() if k not in ("steps", "step_q16", "turn")}
        for prio in ([0, 1], [1, 0]):
            got = fleet.explore_drive(poses, separation_m=sep_m, priority=prio, live_points=pts + body, live_radius_m=radius, live_skip_m=skip, **kw)
            ref = LR.fleet_rollout(keys, wi, live, dposes, lists["steps"], lists["step_q16"], lists["turn"], prio, sep, **fkw)
            for r in range(2):
                assert got[r]["choice"].tobytes() == ref[0][r].tobytes() and got[r]["blocked"] == ref[4][r] and got[r]["rank"] == prio.index(r)
                assert got[r]["blocked_live"] == LR.blocked_live(ref[2])[r] and got[r]["live_kept"] == 3 and got[r]["tracks"].shape == (lists["steps"] + 1, 2)
            assert got[0]["blocked_live"] > 0
        assert nodes[0].grid().drive_live() is None
        for r in range(2):                                    # live_points=None: today's answer, field for field
            _same(fleet.explore_drive(poses, **kw)[r], today[r])
        for bad in (dict(live_radius_m=-res), dict(live_radius_m=65 * res), dict(live_skip_m=-res), dict(live_points=[(float("inf"), 0.0)]),
                    dict(live_points=np.zeros((32769, 2))), dict(priority=[0, 1]), dict(separation_m=-1.0)):
            with pytest.raises(capi.TsdError):
                fleet.explore_drive(poses, **dict(dict(kw, live_points=pts, live_radius_m=radius), **bad))
        assert nodes[0].grid().drive_live() is None
    finally:
        fleet.close()
        for n in nodes:
            n.close()
