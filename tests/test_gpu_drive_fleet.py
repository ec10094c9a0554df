"""The fleet rollout on the device (csrc/drive.hip; tsd_drive_fleet_rollout) against the restatement of tests/drive_fleet_ref.py:
every comparison is byte for byte -- the choice records, the scores and `why` of every sample, the tracks, and the words of
sentinel-filled outputs the call must not write.  The goal fields are the device's own fields results of the maps of
drive_ref.cases() and of a free corridor map."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_fleet_ref as FR
from tests import drive_ref as DR
from tests import route_fields_ref as RF
from tests import route_ref as RR
from tests import test_gpu_drive as GD

pytestmark = pytest.mark.gpu

H = DR.H
CELL = 65536
S64, S16, TAIL = GD.S64, GD.S16, GD.TAIL
T64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cases():
    out = DR.cases()
    out["corridor_96x64"] = _corridor()
    return out


def _corridor():
    """96 x 64, free but for single cells on the rows the robots of the seam test drive along; two goals"""
    m = np.zeros((64, 96), dtype=np.int8)
    m[35, 66] = RR.O                                          # row 35: the centre enters it at k = 64
    m[45, 70] = RR.O                                          # row 45: at k = 68
    m[55, 68] = RR.O                                          # row 55: right in front of the robot that stands at x = 67
    goals = [(94, 1), (1, 62)]
    keys = RF.fields(m, goals)[0]
    keys.setflags(write=False)
    return dict(map=m, wi=RR.weight_image(m), keys=None, fields=keys, goals=goals, free_max=0, w=None, limit=0)


def _load(grid, c):
    GD._load(grid, c, route=False, fields=True)


def _raw(grid, poses, steps, step_q16, turn, order, sep, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0, scores=True, why=True,
         tracks=True, null=(), n=None):
    """one call into sentinel-filled outputs: (rc, choice, scores, why, tracks), the last three with TAIL words behind the call's own"""
    prm, keep = grid._drive_params(steps, step_q16, turn, body, weights, nose_q16, nose_miss)
    p = capi.drive_poses(poses)
    o = np.ascontiguousarray(order, dtype=np.int32)
    fleet = capi.DriveFleetParams(None if "order" in null else o.ctypes.data_as(C.POINTER(C.c_int32)), int(sep), 0)
    ns = p.size * prm.n_speeds * prm.n_turns
    choice = np.frombuffer(bytes([0xA5]) * (40 * p.size), dtype=capi.DRIVE_CHOICE_DTYPE).copy()
    sc, wh = np.full(ns + TAIL, S64, dtype=np.uint64), np.full(ns + TAIL, S16, dtype=np.uint16)
    tr = np.full(p.size * (int(steps) + 1) * 2 + TAIL, T64, dtype=np.int64)
    rc = grid.lib.tsd_drive_fleet_rollout(grid.h, None if "params" in null else C.byref(prm), None if "fleet" in null else C.byref(fleet),
                                          None if "poses" in null else p.ctypes.data, int(p.size) if n is None else n,
                                          None if "choice" in null else choice.ctypes.data, sc.ctypes.data if scores else None,
                                          wh.ctypes.data if why else None, tr.ctypes.data if tracks else None)
    return rc, choice, sc, wh, tr


def _check(grid, c, poses, steps, step_q16, turn, order, sep, what="", **kw):
    want = FR.rollout(c["fields"], c["wi"], poses, steps, step_q16, turn, order, sep, **kw)
    rc, choice, sc, wh, tr = _raw(grid, poses, steps, step_q16, turn, order, sep, **kw)
    n, nt = want[1].size, want[3].size
    assert rc == 0, (what, grid.lib.tsd_last_error(grid.h))
    assert wh[:n].tobytes() == want[2].tobytes(), (what, "why", np.argwhere(wh[:n].reshape(want[2].shape) != want[2])[:4])
    assert sc[:n].tobytes() == want[1].tobytes(), (what, "scores", np.argwhere(sc[:n].reshape(want[1].shape) != want[1])[:4])
    assert choice.tobytes() == want[0].tobytes(), (what, choice, want[0])
    assert tr[:nt].tobytes() == want[3].tobytes(), (what, "tracks", np.argwhere(tr[:nt].reshape(want[3].shape) != want[3])[:4])
    assert (sc[n:] == S64).all() and (wh[n:] == S16).all() and (tr[nt:] == T64).all(), (what, "words beyond the outputs were written")
    return want


def _order(R, kind):
    if kind == "identity":
        return list(range(R))
    if kind == "reversed":
        return list(range(R))[::-1]
    return [int(v) for v in np.random.default_rng(1000 + R).permutation(R)]


def _cluster(c, R, layers, parked=()):
    """R poses three cells apart round a free place of the map, headings all round, layer r mod layers; `parked`: with layer -1"""
    ys, xs = np.nonzero(c["wi"] > 0)
    Hh, W = c["wi"].shape
    x0, y0 = W // 2 - 6, Hh // 2 - 6
    out = []
    for r in range(R):
        x, y = x0 + 3 * (r % 4), y0 + 3 * (r // 4)
        if c["wi"][y, x] == 0:                                # (the next free cell in the row)
            x = int(xs[(ys == y) & (xs > x)][0])
        out.append((x, y, (977 * r) % 65536, (313 * r) % 65536, (257 * r + 300 * (r % 5)) % H, -1 if r in parked else r % layers))
    return out


# (T, B, V, Wn, the turns' unit, R, the order, sep): T at the wave's edges, B at its limits, sample counts round the four samples of
# a workgroup and the most there are, the robot counts with each kind of order, the separations at their limits
SHAPES = [(1, 0, 1, 1, 1, 1, "identity", CELL), (2, 1, 1, 3, 300, 2, "reversed", 3 * CELL), (63, 0, 2, 2, 8, 3, "shuffle", 4 * CELL),
          (64, 64, 1, 5, 6, 3, "reversed", 2 * CELL), (65, 1, 2, 3, 5, 16, "shuffle", 5 * CELL), (129, 0, 1, 4, 4, 2, "identity", FR.SEP_MAX),
          (256, 1, 3, 5, 2, 3, "identity", 6 * CELL), (8, 0, 64, 129, 8, 3, "reversed", 3 * CELL), (20, 4, 5, 13, 40, 16, "identity", 3 * CELL),
          (20, 4, 5, 13, 40, 16, "reversed", 1), (20, 4, 5, 13, 40, 16, "shuffle", 0),
          # the rest of the robot count x order grid, and the longest arcs with all 16 robots
          (12, 1, 2, 3, 60, 1, "reversed", 3 * CELL), (12, 1, 2, 3, 60, 1, "shuffle", 3 * CELL), (12, 1, 2, 3, 60, 2, "shuffle", 3 * CELL),
          (12, 1, 2, 3, 60, 2, "identity", 3 * CELL), (12, 1, 2, 3, 60, 3, "identity", 3 * CELL), (12, 1, 2, 3, 60, 16, "reversed", 3 * CELL),
          (129, 1, 2, 3, 5, 16, "reversed", 4 * CELL), (256, 0, 2, 3, 3, 16, "shuffle", 5 * CELL)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_B%d_V%d_W%d_u%d_R%d_%s_sep%d" % s)
@pytest.mark.parametrize("name", ["open_45x37", "random_67x50"])
def test_fleet_rollout_equals_the_restatement(grid, cases, name, shape):
    T, B, V, Wn, unit, R, kind, sep = shape
    c = cases[name]
    _load(grid, c)
    poses = _cluster(c, R, c["fields"].shape[0], parked=(R - 2,) if R >= 3 else ())
    kw = dict(body=GD._body(B, 20000 if name.startswith("random") else 98304) if B else None, weights=(3, 2, 1, 5), nose_q16=3 * CELL + 77, nose_miss=123)
    order = _order(R, kind)
    want = _check(grid, c, poses, T, GD._speeds(V), GD._turns(Wn, unit), order, sep, f"{name} {shape}", **kw)
    reasons = sorted(set((want[2] >> 12).ravel().tolist()))
    print(f"{name} {shape}: order {order}, reasons {reasons}, admissible {want[0]['admissible'].tolist()}, blocked {want[4].tolist()}")
    if sep == 0 or R == 1:                                    # byte for byte the fields rollout (a parked robot left out)
        live = [r for r in range(R) if poses[r][5] >= 0]
        old = GD._raw(grid, "fields", [poses[r] for r in live], T, GD._speeds(V), GD._turns(Wn, unit), **kw)
        ns = V * Wn
        assert old[0] == 0 and old[1].tobytes() == want[0][live].tobytes()
        assert old[2][:len(live) * ns].tobytes() == want[1][live].tobytes() and old[3][:len(live) * ns].tobytes() == want[2][live].tobytes()
        assert want[4].sum() == 0
    elif sep >= CELL and R > 1 and T > 1 and name == "open_45x37":
        assert 6 in reasons and want[4].sum() > 0             # the cluster is tight enough for the rule to bite
    if name == "open_45x37" and R >= 3:
        assert (want[0]["speed"][2::3] == -1).all()           # layer 2 holds no key: robots without an admissible sample stand


SEAM = dict(T=100, step_q16=[65536], turn=[0], sep=CELL + 1)
SEAM_ROWS = (5, 15, 25, 35, 45, 55)


def _seam_poses():
    """On each row a robot at x = 2 that drives along +x one cell per step, and one that stands in its way: parked at x = 4, 67 and
    68 (the first lane of the first round, the last one, and the first of the second round), at 67 behind a map refusal at k = 64 and
    before one at k = 68, and on row 55 a robot that is not parked but finds no admissible sample"""
    movers = [(2, y, 32768, 32768, 0, 0) for y in SEAM_ROWS]
    others = [(x, y, 32768, 32768, 0, -1) for x, y in zip((4, 67, 68, 67, 67), SEAM_ROWS)] + [(67, 55, 32768, 32768, 0, 1)]
    return movers + others


def test_conflicts_at_the_round_edges_and_beside_map_refusals(grid, cases):
    c = cases["corridor_96x64"]
    _load(grid, c)
    poses = _seam_poses()
    order = list(range(12))                                   # the movers first, the parked robots LAST: they count as decided all the same
    want = _check(grid, c, poses, SEAM["T"], SEAM["step_q16"], SEAM["turn"], order, SEAM["sep"], "seam")
    assert want[2][:6, 0, 0].tolist() == [(6 << 12) | 1, (6 << 12) | 64, (6 << 12) | 65, (2 << 12) | 64, (6 << 12) | 64, (2 << 12) | 66]
    assert want[2][11, 0, 0] == (2 << 12) | 1 and want[0][11]["speed"] == -1
    # the robot without an admissible sample decides first: it stands, and the mover on its row is refused at k = 64
    first = [11] + list(range(11))
    assert _check(grid, c, poses, SEAM["T"], SEAM["step_q16"], SEAM["turn"], first, SEAM["sep"], "seam, the standing robot first")[2][5, 0, 0] == (6 << 12) | 64
    for T, why in ((63, [0, 0]), (64, [(6 << 12) | 64, 0]), (65, [(6 << 12) | 64, (6 << 12) | 65])):
        rows = [poses[1], poses[2], poses[7], poses[8]]
        assert _check(grid, c, rows, T, SEAM["step_q16"], SEAM["turn"], [0, 1, 2, 3], SEAM["sep"], f"seam T {T}")[2][:2].ravel().tolist() == why


def test_the_way_out_across_the_round_edge(grid, cases):
    """a robot one cell from a parked one creeps away at 1/64 cell per step, the separation three cells: D_k < sep^2 at every step
    and D_k > D_{k-1} at every step, the first lane of the second round included (its D_{k-1} is the carry's); creeping closer is refused at k = 1"""
    c = cases["corridor_96x64"]
    _load(grid, c)
    poses = [(20, 20, 32768, 32768, H // 2, 0), (21, 20, 32768, 32768, 0, -1), (60, 50, 0, 0, 0, 1), (61, 50, 0, 0, 0, -1)]
    want = _check(grid, c, poses, 130, [1024, 0], [0, 3], [3, 2, 1, 0], 3 * CELL, "creeping")
    assert want[2][0, 0, 0] == 0 and want[2][0, 1, 0] == (6 << 12) | 1 and want[2][2, 0, 0] == (6 << 12) | 1
    assert FR.dist(want[3][0, 130], want[3][1, 130], 3 * CELL) < (3 * CELL) ** 2     # still inside the separation at the end


HEAD_ON = dict(T=80, step_q16=[32768], turn=[0], sep=30 * CELL)


def test_head_on_in_the_corridor(grid, cases):
    """Two pairs of robots drive at each other at half a cell per step, 93 and 94 cells apart, the separation 30 cells: rolled out
    each on its own (tsd_drive_fields_rollout) both robots of a pair take their arc and the arcs break the rule at k = 64 and k = 65;
    the fleet call lets the first of a pair drive and refuses the second -- whichever that is."""
    c = cases["corridor_96x64"]
    _load(grid, c)
    poses = [(2, 10, 0, 0, 0, 0), (95, 10, 0, 0, H // 2, 1), (1, 50, 0, 0, 0, 0), (95, 50, 0, 0, H // 2, 1)]
    lists = (HEAD_ON["T"], HEAD_ON["step_q16"], HEAD_ON["turn"])
    sep = HEAD_ON["sep"]
    rc, choice, _, _ = GD._raw(grid, "fields", poses, *lists)
    assert rc == 0 and (choice["speed"] == 0).all()
    old = np.stack([FR.track_of(poses[r], choice[r], *lists[1:], lists[0]) for r in range(4)])
    assert [v for v in FR.violations(old, sep) if v[2] in (64, 65)] == [(0, 1, 64), (0, 1, 65), (2, 3, 65)]
    ident = _check(grid, c, poses, *lists, [0, 1, 2, 3], sep, "head on")
    assert ident[2].ravel().tolist() == [0, (6 << 12) | 64, 0, (6 << 12) | 65] and not FR.violations(ident[3], sep)
    rev = _check(grid, c, poses, *lists, [3, 2, 1, 0], sep, "head on, reversed")
    assert rev[2].ravel().tolist() == [(6 << 12) | 64, 0, (6 << 12) | 65, 0] and not FR.violations(rev[3], sep)
    assert rev[0].tobytes() != ident[0].tobytes()
    assert np.array_equal(ident[3][0], old[0]) and np.array_equal(rev[3][1], old[1])          # rank 0 drives as if alone


def test_scratch_is_reused_and_null_outputs_change_nothing(grid, cases):
    c = cases["random_67x50"]
    _load(grid, c)
    L = c["fields"].shape[0]
    big = (_cluster(c, 8, L, parked=(3,)), 65, GD._speeds(9), GD._turns(21, 20), _order(8, "shuffle"), 3 * CELL)
    small = (_cluster(c, 2, L), 10, GD._speeds(2), [0, 7], [1, 0], 2 * CELL)
    kw = dict(body=GD._body(7, 20000), weights=(1, 1, 1, 1), nose_q16=CELL, nose_miss=9)
    first = _check(grid, c, *big, "first", **kw)
    block = grid.drive_dev_ptrs()
    _check(grid, c, *small, "a smaller call", **kw)
    assert grid.drive_dev_ptrs() == block
    again = _check(grid, c, *big, "the first shape again", **kw)
    assert grid.drive_dev_ptrs() == block and again[0].tobytes() == first[0].tobytes()
    GD._check(grid, c, "fields", big[0][:3], 65, GD._speeds(9), GD._turns(21, 20), "the fields form in between", **kw)
    assert grid.drive_dev_ptrs() == block                     # the fleet's block holds a fields call of the same shape
    _check(grid, c, *big, "and after it", **kw)
    for scores, why, tracks in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        rc, choice, sc, wh, tr = _raw(grid, *big, scores=scores, why=why, tracks=tracks, **kw)
        assert rc == 0 and choice.tobytes() == first[0].tobytes()
        assert (sc == S64).all() if not scores else sc[:first[1].size].tobytes() == first[1].tobytes()
        assert (wh == S16).all() if not why else wh[:first[2].size].tobytes() == first[2].tobytes()
        assert (tr == T64).all() if not tracks else tr[:first[3].size].tobytes() == first[3].tobytes()
    ch, sc, wh, tr = grid.drive_fleet_rollout(*big, want_scores=True, want_tracks=True, **kw)
    assert ch.tobytes() == first[0].tobytes() and np.array_equal(sc, first[1]) and np.array_equal(wh, first[2]) and np.array_equal(tr, first[3])
    assert grid.drive_fleet_rollout(*big, **kw).tobytes() == first[0].tobytes()
    ch, tr = grid.drive_fleet_rollout(*big, want_tracks=True, **kw)
    assert np.array_equal(tr, first[3])


def test_refusals_leave_everything_in_place(grid, cases):
    c = cases["open_45x37"]
    _load(grid, c)
    lib, h = grid.lib, grid.h
    good = dict(poses=[(5, 5, 0, 0, 0, 1), (44, 36, 65535, 65535, H - 1, -1), (7, 5, 0, 0, 0, 2)], steps=8, step_q16=[65536, 0], turn=[0, 512, -512],
                order=[2, 0, 1], sep=FR.SEP_MAX, body=[(64 * CELL, -64 * CELL)], weights=(255, 255, 255, 255), nose_q16=64 * CELL, nose_miss=RR.MAX_DIST)
    outs = []

    def call(**over):
        a = dict(good, **over)
        out = _raw(grid, a.pop("poses"), a.pop("steps"), a.pop("step_q16"), a.pop("turn"), a.pop("order"), a.pop("sep"), **a)
        outs.append(out)
        return out[0]

    p0 = good["poses"]
    bad = [dict(null=("params",)), dict(null=("fleet",)), dict(null=("order",)), dict(null=("poses",)), dict(null=("choice",)), dict(n=0), dict(n=17),
           dict(steps=0), dict(steps=257), dict(step_q16=[65537]), dict(turn=[0, 513]), dict(body=[(64 * CELL + 1, 0)]), dict(weights=(256, 0, 0, 0)),
           dict(nose_q16=-1), dict(nose_miss=RR.MAX_DIST + 1), dict(poses=[(45, 5, 0, 0, 0, 0), p0[1], p0[2]]), dict(poses=[p0[0], (5, 37, 0, 0, 0, -1), p0[2]]),
           dict(poses=[(5, 5, 65536, 0, 0, 0), p0[1], p0[2]]), dict(poses=[(5, 5, 0, 0, H, 0), p0[1], p0[2]]), dict(poses=[(5, 5, 0, 0, 0, 3), p0[1], p0[2]]),
           dict(poses=[(5, 5, 0, 0, 0, -2), p0[1], p0[2]]), dict(order=[0, 1, 1]), dict(order=[0, 1, 3]), dict(order=[-1, 0, 1]), dict(order=[0, 0, 0]),
           dict(sep=-1), dict(sep=FR.SEP_MAX + 1)]
    for kw in bad:
        assert call(**kw) == -1 and b"tsd_drive_fleet_rollout" in lib.tsd_last_error(h), (kw, lib.tsd_last_error(h))
    for rc, choice, sc, wh, tr in outs:
        assert choice.tobytes() == bytes([0xA5]) * choice.nbytes and (sc == S64).all() and (wh == S16).all() and (tr == T64).all()
    assert np.array_equal(grid.route_fields_keys(), c["fields"])
    assert call() == 0                                        # the values at their limits pass
    kw = {k: v for k, v in good.items() if k not in ("poses", "steps", "step_q16", "turn", "order", "sep")}
    _check(grid, c, good["poses"], good["steps"], good["step_q16"], good["turn"], good["order"], good["sep"], "after the refusals", **kw)
    with pytest.raises(capi.TsdError):
        grid.drive_fleet_rollout(good["poses"], 8, [65536], [0], [0, 1], CELL)                # two ranks for three robots
    fresh = capi.TsdGridDevice(8, 0.1, 0.3)
    try:
        rc, choice, sc, wh, tr = _raw(fresh, [(5, 5, 0, 0, 0, 0)], 8, [0], [0], [0], 0)
        assert rc == -1 and b"no fields result" in fresh.lib.tsd_last_error(fresh.h) and choice.tobytes() == bytes([0xA5]) * 40
        assert fresh.lib.tsd_drive_dev_ptrs(fresh.h, None, None) == -1
    finally:
        fresh.close()


def test_the_keys_under_the_poses(grid, cases):
    """tsd_drive_fields_togo: what the facade's default priority sorts by"""
    c = cases["open_45x37"]                                   # layer 2 holds no key
    _load(grid, c)
    poses = [(5, 5, 1, 2, 3, 0), (44, 36, 0, 0, 0, 1), (7, 5, 0, 0, 0, 2), (0, 0, 65535, 65535, H - 1, -1), (40, 30, 0, 0, 0, 0)] + _cluster(c, 11, 3)
    want = [int(c["fields"][p[5]][p[1], p[0]]) if p[5] >= 0 else RR.NONE for p in poses]
    assert grid.drive_fields_togo(poses).tolist() == want and want[2] == want[3] == RR.NONE and want[4] >> 4 == 0
    assert grid.drive_fields_togo(poses[:1]).tolist() == want[:1]
    out = np.full(4, 0xA5A5A5A5, dtype=np.uint32)
    p = capi.drive_poses(poses[:2])
    for bad, n, null in (([(45, 5, 0, 0, 0, 0)], 1, ()), ([(5, 37, 0, 0, 0, 0)], 1, ()), ([(5, 5, 0, 0, 0, 3)], 1, ()), ([(5, 5, 0, 0, 0, -2)], 1, ()),
                         (poses[:2], 0, ()), (poses[:2], 17, ()), (poses[:2], 2, ("poses",)), (poses[:2], 2, ("out",))):
        q = capi.drive_poses(bad)
        rc = grid.lib.tsd_drive_fields_togo(grid.h, None if "poses" in null else q.ctypes.data, n, None if "out" in null else out.ctypes.data)
        assert rc == -1 and b"tsd_drive_fields_togo" in grid.lib.tsd_last_error(grid.h), (bad, n, null)
    assert (out == 0xA5A5A5A5).all()
    assert grid.lib.tsd_drive_fields_togo(grid.h, p.ctypes.data, 2, out.ctypes.data) == 0 and out.tolist() == want[:2] + [0xA5A5A5A5] * 2
    _check(grid, c, poses[:4], 7, [65536, 0], [0, 1, -1], [1, 0, 3, 2], 3 * CELL, "a fleet call after it")      # the block still serves the rollout


def test_every_robot_parked(grid, cases):
    c = cases["open_45x37"]
    _load(grid, c)
    poses = [(5, 5, 1, 2, 3, -1), (6, 5, 0, 0, 0, -1)]
    want = _check(grid, c, poses, 7, [65536, 0], [0, 1, -1], [1, 0], 3 * CELL, "all parked")
    assert (want[0]["speed"] == -1).all() and (want[1] == DR.DRIVE_NONE).all() and (want[2] == 0).all()
    assert want[3][0].tolist() == [[(5 << 16) + 1, (5 << 16) + 2]] * 8


# ---- the facade: SlamFleet.explore_drive with a separation, on the two-node scene of test_gpu_drive.py
def test_fleet_explore_drive_keeps_the_nodes_apart():
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
        poses = [GD._xyt(n) for n in nodes]
        w_max = 40 * 2 * np.pi / (H * res / GD.DRIVE["v_max"])
        d = fleet.explore_dispatch(view_radius_m=1.0, gain_weight=3, lookahead_m=1.5, unknown_depth=2, min_size=3, max_len=2048, max_way=64)
        assert (d["goal_of_robot"] >= 0).all()
        for r in range(2):                                    # every node facing along the first segment of its way
            way = d["waypoints"][r]
            poses[r] = poses[r][:2] + (float(np.arctan2(way[1][1] - way[0][1], way[1][0] - way[0][0])),)
        dt, lists = GD._lists(res, w_max, [])
        # separation 0: today's answer, field for field
        today = fleet.explore_drive(poses, w_max=w_max, **GD.DRIVE)
        zero = fleet.explore_drive(poses, w_max=w_max, separation_m=0.0, **GD.DRIVE)
        seeds = [(int(c) % W, int(c) // W) for c in d["goal"]["cell"]]
        keys, _ = RF.fields(data, seeds, limit=int(d["goal"]["dist"].max()) + GD.DRIVE["margin"])
        wi = RR.weight_image(data)
        dposes = [GD._drive_pose(poses[r], m, r) for r in range(2)]
        for r in range(2):
            assert set(zero[r]) == set(today[r]) and "tracks" not in zero[r]
            for k, v in today[r].items():
                if k == "choice":
                    assert zero[r][k].tobytes() == v.tobytes()
                else:
                    assert np.array_equal(zero[r][k], v), k
            assert zero[r]["choice"].tobytes() == DR.rollout(keys[r], wi, dposes[r], **lists)[0].tobytes()
        # a separation two cells wider than the nodes stand apart: whoever decides second has to move away from the first
        apart = math.hypot(poses[0][0] - poses[1][0], poses[0][1] - poses[1][1])
        sep_m = apart + 2 * res
        sep = math.floor(sep_m / res * 65536.0 + 0.5)
        assert sep <= FR.SEP_MAX
        togo = [int(keys[r][dposes[r][1], dposes[r][0]]) for r in range(2)]
        default = sorted(range(2), key=lambda r: togo[r])     # (stable: ties by index)
        fkw = {k: v for k, v in lists.items() if k not in ("steps", "step_q16", "turn")}
        results = {}
        for prio in (None, [1, 0], [0, 1]):
            order = default if prio is None else prio
            out = fleet.explore_drive(poses, w_max=w_max, separation_m=sep_m, priority=prio, **GD.DRIVE)
            assert np.array_equal(nodes[0].grid().route_fields_keys(), keys)
            want = FR.rollout(keys, wi, dposes, lists["steps"], lists["step_q16"], lists["turn"], order, sep, **fkw)
            print(f"priority {prio}: order {order}, blocked {want[4].tolist()}, admissible {want[0]['admissible'].tolist()}")
            for r in range(2):
                assert out[r]["choice"].tobytes() == want[0][r].tobytes() and out[r]["blocked"] == want[4][r] and out[r]["rank"] == order.index(r)
                metres = want[3][r].astype(np.float64) / 65536.0 * res + np.asarray(m["origin_position"][:2], dtype=np.float64)
                assert out[r]["tracks"].shape == (lists["steps"] + 1, 2) and np.array_equal(out[r]["tracks"], metres)
                assert out[r]["steps"] == lists["steps"] and out[r]["dt"] == dt
            assert not FR.violations(want[3], sep)            # the tracks the device chose satisfy the rule
            assert want[4][order[0]] == 0 and want[4][order[1]] > 0
            first = order[0]                                  # rank 0 drives as if it were alone
            assert out[first]["choice"].tobytes() == today[first]["choice"].tobytes()
            results[tuple(order)] = out
        for kw in (dict(separation_m=-1.0), dict(separation_m=129 * res), dict(separation_m=sep_m, priority=[0, 0]), dict(separation_m=sep_m, priority=[0]),
                   dict(priority=[0, 1])):
            with pytest.raises(capi.TsdError):
                fleet.explore_drive(poses, w_max=w_max, **dict(GD.DRIVE, **kw))
    finally:
        fleet.close()
        for n in nodes:
            n.close()
