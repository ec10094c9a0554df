"""The live layer without a GPU: the ABI of tsd_drive_live_*, and the properties of the rule on the restatement of
tests/drive_live_ref.py, which is what tests/test_gpu_drive_live.py holds the kernels against."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_fleet_ref as FR
from tests import drive_live_ref as LR
from tests import drive_ref as DR

H = DR.H
CELL = 65536


@pytest.fixture(scope="module")
def cases():
    return DR.cases()


def _open(W=60, Hh=40, layers=1):
    """a free map: every cell has a key (the column distance to x = W - 1) and w = 1"""
    keys = np.tile(((W - 1 - np.arange(W, dtype=np.uint32)) * 5) << 4, (layers, Hh, 1))
    return keys, np.ones((Hh, W), dtype=np.uint8)


def _layer(shape, cells):
    live = np.zeros(shape, dtype=bool)
    for x, y in cells:
        live[y, x] = True
    return live


def test_the_abi_declares_the_live_calls(hip_lib):
    for name in ("tsd_drive_live_set", "tsd_drive_live_clear", "tsd_drive_live_fetch", "tsd_drive_live_dev_ptr"):
        assert name in capi.ABI and getattr(hip_lib, name) is not None
    assert C.sizeof(capi.DriveLiveParams) == 16 == hip_lib.tsd_abi_sizeof(b"tsd_drive_live_params")
    assert (capi.DRIVE_LIVE_MAX_POINTS, capi.DRIVE_LIVE_MAX_SKIP, capi.DRIVE_LIVE_MAX_RADIUS) == (32768, 16, 64) == (LR.MAX_POINTS, LR.MAX_SKIP, LR.MAX_RADIUS)
    for name in ("drive_live_set", "drive_live_clear", "drive_live"):
        assert hasattr(capi.TsdGridDevice, name)


@pytest.mark.parametrize("size", LR.STAMP_MAPS, ids=lambda s: "%dx%d" % s)
def test_the_two_stamps_agree(size):
    W, Hh = size
    for r in (0, 1, 2, 63, 64):
        pts = LR.stamp_points(W, Hh, r)
        if W > 1000:
            pts = [p for p in pts if p[0] < 0 or p[0] > W - 200 or abs(p[0]) > 1 << 20][:8]      # (the slow form walks every cell near a point)
        a, na = LR.stamp(pts, r, W, Hh)
        b, nb = LR.stamp_slow(pts, r, W, Hh)
        assert np.array_equal(a, b) and na == nb == len(pts), (size, r)
        words = LR.pack(a)
        assert words.shape == (Hh, LR.stride_words(W)) and np.array_equal(LR.unpack(words, W), a)
        if W % 32:
            assert (words[:, -1] >> (W % 32) == 0).all()                  # the tail bits stay 0
        # a point outside by r + 1 writes nothing, one outside by exactly r writes its one cell
        assert not LR.stamp([(-r - 1, 0), (W + r, 0), (0, -r - 1), (0, Hh + r)], r, W, Hh)[0].any()
        assert LR.stamp([(-r, 0)], r, W, Hh)[0].sum() == 1 and LR.stamp([(-r, 0)], r, W, Hh)[0][0, 0]


def test_the_skip_discs_drop_points_on_the_rim():
    W, Hh = 45, 37
    pts = [(10, 10), (13, 14), (13, 15), (20, 20), (20, 20), (40, 3)]
    skip = [(10, 10, 5), (20, 20, 0)]                                   # (13, 14) lies on the rim of the first: 9 + 16 == 25
    assert LR.kept(pts, skip).tolist() == [False, False, True, False, False, True]
    for r in (0, 2):
        a, na = LR.stamp(pts, r, W, Hh, skip)
        b, nb = LR.stamp_slow(pts, r, W, Hh, skip)
        assert np.array_equal(a, b) and na == nb == 2
        assert np.array_equal(a, LR.stamp([(13, 15), (40, 3)], r, W, Hh)[0])
    every = [(p[0], p[1], 0) for p in pts] + [(0, 0, 1 << 15)] * 10
    a, n = LR.stamp(pts, 3, W, Hh, every)
    assert len(every) == 16 and n == 0 and not a.any() and LR.stamp_slow(pts, 3, W, Hh, every)[1] == 0
    assert LR.stamp([], 5, W, Hh)[1] == 0 and not LR.stamp(None, 5, W, Hh)[0].any()


def test_no_layer_and_an_empty_layer_are_the_rules_without_it(cases):
    kw = dict(body=[(CELL, 30000), (-70000, 0)], weights=(3, 2, 1, 5), nose_q16=200000, nose_miss=77)
    speeds, turn = [65536, 40000, 0], [0, 5, -5, 100, -100]
    for name in ("door_96x64", "random_67x50"):
        c = cases[name]
        L = c["fields"].shape[0]
        poses = [(5, 5, 100, 65535, 17, 0), (6, 5, 65535, 65535, H - 1, 1 % L), (7, 6, 0, 0, H // 2, 0)]
        empty = np.zeros(c["wi"].shape, dtype=bool)
        for keys in (c["keys"], c["fields"]):
            want = DR.rollout_all(keys, c["wi"], poses, 20, speeds, turn, **kw)
            for live in (None, empty):
                got = LR.rollout_all(keys, c["wi"], live, poses, 20, speeds, turn, **kw)
                assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        want = FR.rollout(c["fields"], c["wi"], poses, 20, speeds, turn, [2, 0, 1], 3 * CELL, **kw)
        for live in (None, empty):
            got = LR.fleet_rollout(c["fields"], c["wi"], live, poses, 20, speeds, turn, [2, 0, 1], 3 * CELL, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and got[0].tobytes() == want[0].tobytes()


def test_the_two_forms_of_the_restatement_agree(cases):
    """``rollout`` and ``fleet_rollout`` (numpy over the samples) against ``sample`` and ``fleet_sample`` (the rule step by step)"""
    kw = dict(body=[(CELL, 0), (-CELL, 0), (0, 2 * CELL)], weights=(3, 2, 1, 5), nose_q16=200000, nose_miss=77)
    speeds, turn, T = [65536, 40000, 0], [0, 40, -40, 200, -200], 20
    c = cases["door_96x64"]
    live, _ = LR.stamp([(44, 30), (52, 36), (47, 25), (60, 33), (40, 33)], 1, 96, 64)
    poses = [(40, 31, 100, 65535, 0, 0), (56, 31, 65535, 65535, H // 2, 1), (44, 33, 0, 0, 100, 0), (47, 36, 9, 9, H // 4, -1), (52, 33, 0, 0, H // 2 + 50, 1)]
    reasons = set()
    for r, p in enumerate(poses[:3]):
        ch, sc, why = LR.rollout(c["keys"], c["wi"], live, p, T, speeds, turn, **kw)
        for i, s in enumerate(speeds):
            for j, t in enumerate(turn):
                w, score, rec = LR.sample(c["keys"], c["wi"], live, p, s, t, T, **kw)
                assert (w, score) == (int(why[i, j]), int(sc[i, j])), (r, i, j)
                reasons.add(w >> 12)
        assert ch["admissible"] == (why == 0).sum()
    assert reasons >= {0, 4, 7}
    reasons = set()
    for order, sep in (([0, 1, 2, 3, 4], 3 * CELL), ([4, 3, 2, 1, 0], 5 * CELL + 123)):
        ch, sc, why, tr, bl = LR.fleet_rollout(c["fields"], c["wi"], live, poses, T, speeds, turn, order, sep, **kw)
        decided = [3]
        for r in [q for q in order if q != 3]:
            others = [tr[q] for q in decided]
            for i, s in enumerate(speeds):
                for j, t in enumerate(turn):
                    w, score, rec = LR.fleet_sample(c["fields"][poses[r][5]], c["wi"], live, poses[r], s, t, T, others, sep, **kw)
                    assert (w, score) == (int(why[r, i, j]), int(sc[r, i, j])), (order, r, i, j)
                    reasons.add(w >> 12)
            assert bl[r] == (why[r] >> 12 == 6).sum() and ch[r]["admissible"] == (why[r] == 0).sum()
            assert np.array_equal(tr[r], FR.track_of(poses[r], ch[r], speeds, turn, T))
            decided.append(r)
    assert reasons >= {0, 6, 7}


def test_the_order_of_the_reasons():
    keys, wi = _open()
    me = (20, 20, 32768, 32768, 0, 0)                                   # one cell per step along +x: c_k = (20 + k, 20)
    arc = (12, [65536], [0])
    at = lambda live, **kw: int(LR.rollout(keys[0], wi, live, me, *arc, **kw)[2][0, 0])
    shape = wi.shape
    assert at(_layer(shape, [(26, 20)])) == (7 << 12) | 6
    # 4 beats 7 at one step: at k = 6 the body point beside the centre stands on a cell with w == 0, the centre on a live cell
    wall = wi.copy()
    wall[21, 26] = 0
    beside = [(0, CELL)]
    got = LR.rollout(keys[0], wall, _layer(shape, [(26, 20)]), me, *arc, body=beside)[2][0, 0]
    assert got == (4 << 12) | 6 and LR.sample(keys[0], wall, _layer(shape, [(26, 20)]), me, 65536, 0, 12, body=beside)[0] == got
    # ... and 7 one step earlier beats it, on the centre or on the body point
    assert LR.rollout(keys[0], wall, _layer(shape, [(25, 20)]), me, *arc, body=beside)[2][0, 0] == (7 << 12) | 5
    assert LR.rollout(keys[0], wall, _layer(shape, [(25, 21)]), me, *arc, body=beside)[2][0, 0] == (7 << 12) | 5
    # 2 at a later step loses to 7 at an earlier one; at the same step 2 wins
    wall = wi.copy()
    wall[20, 27] = 0
    assert LR.rollout(keys[0], wall, _layer(shape, [(24, 20)]), me, *arc)[2][0, 0] == (7 << 12) | 4
    assert LR.rollout(keys[0], wall, _layer(shape, [(27, 20)]), me, *arc)[2][0, 0] == (2 << 12) | 7
    # 5 loses: a live cell at c_T where c_T has no key
    nokey = keys.copy()
    nokey[0, 20, 32] = DR.NONE
    assert DR.rollout(nokey[0], wi, me, *arc)[2][0, 0] == (5 << 12) | 12
    assert LR.rollout(nokey[0], wi, _layer(shape, [(32, 20)]), me, *arc)[2][0, 0] == (7 << 12) | 12
    # the lowest body point is what the rule names; `why` holds the step: the later point's earlier step wins
    body = [(0, 3 * CELL), (2 * CELL, 0)]                               # point 0 beside the track, point 1 two cells ahead
    live = _layer(shape, [(23, 23), (30, 20)])
    assert at(live, body=body) == (7 << 12) | 3                       # point 0 at k = 3
    assert at(_layer(shape, [(30, 20)]), body=body) == (7 << 12) | 8  # point 1 at k = 8, the centre only at k = 10
    # 7 beats 6 at one step, and loses to it one step later
    parked = lambda x: (x, 20, 32768, 32768, 0, -1)
    for x, sep, live_at, want in ((29, 3 * CELL + 1, 26, (7 << 12) | 6), (28, 3 * CELL + 1, 26, (6 << 12) | 5), (29, 3 * CELL + 1, 27, (6 << 12) | 6)):
        live = _layer(shape, [(live_at, 20)])
        got = LR.fleet_rollout(keys, wi, live, [me, parked(x)], *arc, [1, 0], sep)
        assert got[2][0, 0, 0] == want, (x, live_at, hex(int(got[2][0, 0, 0])))
        assert LR.fleet_sample(keys[0], wi, live, me, 65536, 0, 12, [got[3][1]], sep)[0] == want


def test_a_robot_on_a_live_cell_is_freed_by_a_skip_disc():
    keys, wi = _open()
    me = (20, 20, 32768, 32768, 0, 0)
    pts = [(20, 20), (40, 5)]
    live, n = LR.stamp(pts, 1, 60, 40)
    ch, sc, why = LR.rollout(keys[0], wi, live, me, 6, [65536, 30000, 0], [0, 100])
    assert n == 2 and (why == (7 << 12) | 1).all() and ch["speed"] == -1 and ch["admissible"] == 0     # standing still (s = 0) is refused at k = 1 too
    live, n = LR.stamp(pts, 1, 60, 40, skip=[(20, 20, 2)])
    ch, sc, why = LR.rollout(keys[0], wi, live, me, 6, [65536, 30000, 0], [0, 100])
    assert n == 1 and (why == 0).all() and ch["speed"] == 0 and live[5, 40] and not live[20, 20]
    assert ch.tobytes() == DR.rollout(keys[0], wi, me, 6, [65536, 30000, 0], [0, 100])[0].tobytes()


# ---- the closed loop: something that is not on the map walks up and down in front of the doorway
WALK = dict(x=46, y0=14, span=36, speed=2, phase=38, radius=3)


def walker(n):
    """the cell of the walker at command n: up and down column WALK['x'], WALK['speed'] cells per command"""
    u = (WALK["phase"] + WALK["speed"] * n) % (2 * WALK["span"])
    return WALK["x"], WALK["y0"] + (u if u <= WALK["span"] else 2 * WALK["span"] - u)


def _walk(cases, with_layer, cap):
    """the loop of drive_ref.closed_loop with the walker: per command (the pose after the step, the layer the command was chosen on,
    whether the robot found an arc)"""
    c = cases["door_96x64"]
    keys, wi = c["fields"][0], c["wi"]                                 # (seeded at the goal behind the door alone)
    p = DR.loop_params()
    lists = (p["steps"], p["step_q16"], p["turn"])
    kw = dict(body=p["body"], weights=p["weights"], nose_q16=p["nose_q16"], nose_miss=p["nose_miss"])
    pose, log = tuple(DR.LOOP_START), []
    while True:
        k = int(keys[pose[1], pose[0]])
        if k != DR.NONE and (k >> 4) <= DR.LOOP_ARRIVED:
            return log
        assert len(log) < cap, ("the robot did not arrive", pose, len(log))
        live, _ = LR.stamp([walker(len(log))], WALK["radius"], 96, 64)
        ch, _, why = LR.rollout(keys, wi, live if with_layer else None, pose, *lists, **kw)
        if ch["speed"] >= 0:
            assert why[ch["speed"], ch["turn"]] == 0
            pose = DR.advance(pose, p["step_q16"][ch["speed"]], p["turn"][ch["turn"]], 1) + (0,)
        log.append((pose, live, bool(ch["speed"] >= 0)))


def _touches(pose, live):
    """the robot's centre cell or a body point's cell lies in the layer"""
    D = DR.table()
    x0, y0, fx, fy, h = (int(v) for v in pose[:5])
    cx, cy = int(D[h, 0]), int(D[h, 1])
    cells = [(x0, y0)] + [(x0 + ((fx + DR._q16(bx * cx - by * cy)) >> 16), y0 + ((fy + DR._q16(bx * cy + by * cx)) >> 16)) for bx, by in DR.LOOP["body"]]
    return any(LR._in(live, x, y) for x, y in cells)


def test_closed_loop_past_a_walker_in_front_of_the_door(cases):
    """Without the layer the robot drives as drive_ref's closed loop does and at some command stands with its centre or a body
    point inside the walker's disc.  With the layer it never does, at any command: not where a command leaves it, against the layer
    that command was chosen on, and not where the next command finds it, against the layer of that command -- the timetable (two
    cells per command, a disc of three) never walks the disc over the robot, so every command finds an arc -- and it arrives behind
    the door."""
    blind = _walk(cases, False, 120)
    hits = [n for n, (pose, live, moved) in enumerate(blind) if _touches(pose, live)]
    assert hits, "the timetable does not cross the robot's way"
    seeing = _walk(cases, True, 200)
    assert not [n for n, (pose, live, moved) in enumerate(seeing) if _touches(pose, live)]
    assert not [n for n in range(1, len(seeing)) if _touches(seeing[n - 1][0], seeing[n][1])]
    assert not _touches(DR.LOOP_START, seeing[0][1]) and all(moved for _, _, moved in seeing)
    assert seeing[-1][0][0] > 48 and any(not np.array_equal(a[0], b[0]) for a, b in zip(blind, seeing))
    c = cases["door_96x64"]
    assert all(c["wi"][pose[1], pose[0]] > 0 for pose, _, _ in seeing)
