"""The fleet rule without a GPU: the ABI of tsd_drive_fleet_rollout, and the properties of the rule on the restatement of
tests/drive_fleet_ref.py, which is what tests/test_gpu_drive_fleet.py holds the kernels against."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_fleet_ref as FR
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


def test_the_abi_declares_the_fleet_call(hip_lib):
    assert "tsd_drive_fleet_rollout" in capi.ABI and hip_lib.tsd_drive_fleet_rollout is not None
    assert "tsd_drive_fields_togo" in capi.ABI and hip_lib.tsd_drive_fields_togo is not None
    assert C.sizeof(capi.DriveFleetParams) == 16 == hip_lib.tsd_abi_sizeof(b"tsd_drive_fleet_params")
    assert capi.DRIVE_MAX_SEP == 128 * 65536 == FR.SEP_MAX
    assert hasattr(capi.TsdGridDevice, "drive_fleet_rollout")


def test_without_separation_and_alone_it_is_the_fields_rollout(cases):
    kw = dict(body=[(CELL, 30000), (-70000, 0)], weights=(3, 2, 1, 5), nose_q16=200000, nose_miss=77)
    speeds, turn = [65536, 40000, 0], [0, 5, -5, 100, -100]
    for name in ("door_96x64", "random_67x50"):
        c = cases[name]
        L = c["fields"].shape[0]
        poses = [(5, 5, 100, 65535, 17, 0), (6, 5, 65535, 65535, H - 1, 1 % L), (7, 6, 0, 0, H // 2, 0)]
        want = DR.rollout_all(c["fields"], c["wi"], poses, 20, speeds, turn, **kw)
        for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
            got = FR.rollout(c["fields"], c["wi"], poses, 20, speeds, turn, order, 0, **kw)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert (got[4] == 0).all()
        for r, p in enumerate(poses):                                      # one robot: whatever the separation
            got = FR.rollout(c["fields"], c["wi"], [p], 20, speeds, turn, [0], FR.SEP_MAX, **kw)
            assert got[0][0].tobytes() == want[0][r].tobytes() and np.array_equal(got[1][0], want[1][r]) and np.array_equal(got[2][0], want[2][r])
            tr = FR.track_of(p, got[0][0], speeds, turn, 20)
            assert np.array_equal(got[3][0], tr) and tuple(tr[0]) == ((p[0] << 16) + p[2], (p[1] << 16) + p[3])


def test_rank_zero_does_not_depend_on_the_others():
    keys, wi = _open(layers=2)
    prm = (10, [65536, 30000, 0], DR.turns(3))
    poses = [(20, 20, 32768, 32768, 0, 0), (24, 20, 32768, 32768, H // 2, 1), (22, 23, 0, 0, 3 * H // 4, 0)]
    alone = DR.rollout(keys[0], wi, poses[0], *prm)
    first = FR.rollout(keys, wi, poses, *prm, [0, 1, 2], 3 * CELL)
    assert first[0][0].tobytes() == alone[0].tobytes() and np.array_equal(first[1][0], alone[1]) and np.array_equal(first[2][0], alone[2])
    moved = [poses[0], (21, 20, 0, 0, H // 2, 1), (20, 21, 0, 0, 0, 0)]
    other = FR.rollout(keys, wi, moved, *prm, [0, 2, 1], 3 * CELL)
    assert other[0][0].tobytes() == alone[0].tobytes() and np.array_equal(other[2][0], alone[2])
    last = FR.rollout(keys, wi, poses, *prm, [2, 1, 0], 3 * CELL)           # as the last rank it does depend on them
    assert (last[2][0] >> 12 == 6).any() and last[4][0] > 0 and first[4][0] == 0
    # ... but for a parked robot, which counts as decided before rank 0 even where it is listed last
    parked = [poses[0], (24, 20, 32768, 32768, H // 2, -1)]
    got = FR.rollout(keys, wi, parked, *prm, [0, 1], 3 * CELL)
    assert (got[2][0] >> 12 == 6).any() and got[0][1]["speed"] == -1 and (got[1][1] == DR.DRIVE_NONE).all() and (got[2][1] == 0).all()
    assert np.array_equal(got[3][1], FR.standing(parked[1], 10))


def test_the_way_out_of_a_separation_already_broken():
    """Two robots one cell apart, the separation three cells.  An arc that closes in -- or keeps the distance: standing still -- is
    refused by reason 6 at k = 1; an arc on which every step takes the robot further away passes."""
    keys, wi = _open()
    parked = (21, 20, 32768, 32768, 0, -1)
    speeds, sep = [65536, 32768, 0], 3 * CELL
    for heading, want in ((0, [(6 << 12) | 1] * 3), (H // 2, [0, 0, (6 << 12) | 1])):
        ch, sc, why, tr, bl = FR.rollout(keys, wi, [(20, 20, 32768, 32768, heading, 0), parked], 8, speeds, [0], [0, 1], sep)
        assert why[0, :, 0].tolist() == want and bl[0] == sum(w != 0 for w in want)
        for i, s in enumerate(speeds):
            assert FR.sample(keys[0], wi, (20, 20, 32768, 32768, heading, 0), s, 0, 8, [tr[1]], sep)[0] == want[i]
    # sideways the distance grows too (1, sqrt 2, sqrt 5 ... cells): the arc passes; at a right angle round the other it does not
    ch, sc, why, tr, bl = FR.rollout(keys, wi, [(20, 20, 32768, 32768, H // 4, 0), parked], 8, speeds, [0, -512], [0, 1], sep)
    assert why[0, 0, 0] == 0 and why[0, 0, 1] >> 12 == 6
    # a moving other: the rear robot may follow more slowly, not at the same speed
    pair = [(22, 20, 32768, 32768, 0, 0), (21, 20, 32768, 32768, 0, 0)]
    ch, sc, why, tr, bl = FR.rollout(keys, wi, pair, 8, speeds, [0], [0, 1], sep)
    assert (ch[0]["speed"], ch[0]["turn"]) == (0, 0) and why[1, :, 0].tolist() == [(6 << 12) | 1, 0, 0] and ch[1]["speed"] == 1
    assert not FR.violations(tr, sep)
    # where the front robot stands (its only sample is refused by the map: it found none) the rear one may not come closer
    keys2, wi2 = _open()
    wi2[20, 23] = 0
    ch, sc, why, tr, bl = FR.rollout(keys2, wi2, [(22, 20, 32768, 32768, 0, 0), (19, 20, 32768, 32768, 0, 0)], 8, [65536], [0], [0, 1], sep)
    assert ch[0]["speed"] == -1 and why[0, 0, 0] == (2 << 12) | 1 and why[1, 0, 0] == (6 << 12) | 1 and np.array_equal(tr[0], FR.standing((22, 20, 32768, 32768), 8))


def test_the_maps_reason_wins_at_its_own_step_and_loses_behind_a_conflict():
    keys, wi = _open()
    wi = wi.copy()
    wi[20, 26] = 0                                                         # the centre enters (26, 20) at k = 6
    parked = lambda x: (x, 20, 32768, 32768, 0, -1)
    arc = (12, [65536], [0])
    me = (20, 20, 32768, 32768, 0, 0)
    assert DR.rollout(keys[0], wi, me, *arc)[2][0, 0] == (2 << 12) | 6
    # a robot parked three cells ahead of step 6's place: the distance falls below the separation AT k = 6 -- the map's reason stays
    for x, sep, want in ((29, 3 * CELL + 1, (2 << 12) | 6), (28, 3 * CELL + 1, (6 << 12) | 5), (24, CELL, (6 << 12) | 4), (40, 3 * CELL, (2 << 12) | 6)):
        got = FR.rollout(keys, wi, [me, parked(x)], *arc, [1, 0], sep)
        assert got[2][0, 0, 0] == want, (x, sep, hex(int(got[2][0, 0, 0])))
        assert FR.sample(keys[0], wi, me, 65536, 0, 12, [got[3][1]], sep)[0] == want
    # reason 5 stays behind step T: a conflict at k = T wins over it
    nokey = keys.copy()
    nokey[0, 20, 25] = DR.NONE
    assert DR.rollout(nokey[0], wi, me, 5, [65536], [0])[2][0, 0] == (5 << 12) | 5
    assert FR.rollout(nokey, wi, [me, parked(27)], 5, [65536], [0], [0, 1], 2 * CELL + 1)[2][0, 0, 0] == (6 << 12) | 5
    assert FR.rollout(nokey, wi, [me, parked(28)], 5, [65536], [0], [0, 1], 2 * CELL + 1)[2][0, 0, 0] == (5 << 12) | 5


def test_far_coordinates_do_not_overflow():
    """Poses 30 000 cells apart: dx = 30 000 * 65536 < 2^31, its square would need 62 bits and with dy^2 more than an int64 comparison
    against sep^2 tolerates in a careless form -- the rule calls the pair far before it multiplies."""
    keys, wi = _open(W=30010, Hh=4, layers=2)
    poses = [(3, 1, 0, 0, 0, 0), (30003, 1, 65535, 65535, H // 2, 1), (30004, 2, 0, 0, H // 2, 1)]
    prm = (6, [65536, 0], [0, 9])
    sep = FR.SEP_MAX
    assert FR.dist((3 << 16, 1 << 16), ((30003 << 16) + 65535, (1 << 16) + 65535), sep) == FR.FAR
    assert FR.dist((0, 0), (sep, 0), sep) == FR.FAR and FR.dist((0, 0), (sep - 1, -(sep - 1)), sep) == 2 * (sep - 1) ** 2 < 1 << 47
    got = FR.rollout(keys, wi, poses, *prm, [1, 0, 2], sep)
    want = DR.rollout_all(keys, wi, poses[:2], *prm)
    assert got[0][:2].tobytes() == want[0].tobytes() and np.array_equal(got[2][:2], want[2])             # robots 0 and 1 never meet
    # robot 2 stands all but on robot 1, which stays where it is (its field falls towards +x): driving off passes, staying does not
    assert got[0][1]["speed"] == 1 and (got[2][2, 0] == 0).all() and (got[2][2, 1] == (6 << 12) | 1).all() and got[4].tolist() == [0, 0, 2]
    assert int(got[3][1, 0, 0]) == (30003 << 16) + 65535 and got[3].dtype == np.int64


def test_the_two_forms_of_the_restatement_agree(cases):
    """``rollout`` (numpy over the samples and steps) against ``sample`` (the rule step by step), rank after rank"""
    kw = dict(body=[(CELL, 0), (-CELL, 0)], weights=(3, 2, 1, 5), nose_q16=200000, nose_miss=77)
    speeds, turn, T = [65536, 40000, 0], [0, 40, -40, 200, -200], 20
    c = cases["door_96x64"]
    poses = [(40, 32, 100, 65535, 0, 0), (56, 31, 65535, 65535, H // 2, 1), (44, 30, 0, 0, 100, 0), (47, 36, 9, 9, H // 4, -1), (52, 33, 0, 0, H // 2 + 50, 1)]
    reasons = set()
    for order, sep in (([0, 1, 2, 3, 4], 3 * CELL), ([4, 3, 2, 1, 0], 5 * CELL + 123), ([2, 0, 4, 1, 3], 2 * CELL)):
        ch, sc, why, tr, bl = FR.rollout(c["fields"], c["wi"], poses, T, speeds, turn, order, sep, **kw)
        decided = [3]
        for r in [q for q in order if q != 3]:
            others = [tr[q] for q in decided]
            for i, s in enumerate(speeds):
                for j, t in enumerate(turn):
                    w, score, rec = FR.sample(c["fields"][poses[r][5]], c["wi"], poses[r], s, t, T, others, sep, **kw)
                    assert (w, score) == (int(why[r, i, j]), int(sc[r, i, j])), (order, r, i, j)
                    reasons.add(w >> 12)
            assert bl[r] == (why[r] >> 12 == 6).sum() and ch[r]["admissible"] == (why[r] == 0).sum()
            assert np.array_equal(tr[r], FR.track_of(poses[r], ch[r], speeds, turn, T))
            decided.append(r)
        assert not FR.violations(tr, sep, pairs=None if all(c["speed"] >= 0 for c in ch[[0, 1, 2, 4]]) else set())
    assert reasons >= {0, 4, 6} and reasons & {2, 3}


# ---- the closed loop: two robots through one doorway in opposite directions
LOOP_STARTS = [(36, 32, 32768, 32768, 0), (60, 31, 32768, 32768, H // 2)]         # left of the door looking at it, and right of it
LOOP_SEP = 3 * CELL


def _loop(cases, fleet, cap):
    """Both robots take the first step of their choice and roll out again, robot r on layer r (the goals right and left of the wall);
    a robot that has arrived is parked.  Per command: (poses, choices, the chosen tracks)."""
    c = cases["door_96x64"]
    keys, wi = c["fields"], c["wi"]
    p = DR.loop_params()
    lists = (p["steps"], p["step_q16"], p["turn"])
    kw = dict(body=p["body"], weights=p["weights"], nose_q16=p["nose_q16"], nose_miss=p["nose_miss"])
    poses, log = [tuple(s) for s in LOOP_STARTS], []
    while True:
        here = [int(keys[r][q[1], q[0]]) for r, q in enumerate(poses)]
        arrived = [k != DR.NONE and (k >> 4) <= DR.LOOP_ARRIVED for k in here]
        if all(arrived):
            return log
        assert len(log) < cap, ("the robots did not arrive", poses, len(log))
        ps = [q[:5] + ((-1 if arrived[r] else r),) for r, q in enumerate(poses)]
        if fleet:
            ch, _, why, tr, _ = FR.rollout(keys, wi, ps, *lists, [0, 1], LOOP_SEP, **kw)
        else:                                                              # each robot alone on the map
            ch = np.array([DR.rollout(keys[r], wi, ps[r], *lists, **kw)[0] for r in range(2)], dtype=DR.CHOICE_DTYPE)
            tr = np.stack([FR.track_of(ps[r], ch[r], *lists[1:], lists[0]) if not arrived[r] else FR.standing(ps[r], lists[0]) for r in range(2)])
        log.append((list(poses), ch, tr))
        for r in range(2):
            if not arrived[r]:
                assert ch[r]["speed"] >= 0 and wi[poses[r][1], poses[r][0]] > 0, (r, poses, len(log))
                poses[r] = DR.advance(poses[r], p["step_q16"][ch[r]["speed"]], p["turn"][ch[r]["turn"]], 1)


def test_closed_loop_two_robots_through_one_door(cases):
    """Rolled out each on its own the two robots arrive after 66 commands, and from the first command on their chosen arcs cross in
    the doorway at the same step: that is what the fleet rule removes.  With it robot 1 gives way to robot 0 (rank 0), no pair of
    chosen arcs ever breaks the rule, the robots themselves never come closer than the separation, and both arrive after 77 commands
    (integer arithmetic: the same everywhere); the cap is 90."""
    old = _loop(cases, False, 90)
    assert len(old) == 66
    broken = [n for n, (_, _, tr) in enumerate(old) if FR.violations(tr, LOOP_SEP)]
    assert broken and broken[0] == 0
    near = min((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for (a, b), _, _ in old)
    assert near < 9                                                        # ... and the robots do meet: closer than three cells
    new = _loop(cases, True, 90)
    assert len(new) == 77
    for n, (poses, ch, tr) in enumerate(new):
        assert not FR.violations(tr, LOOP_SEP), n
    at = lambda q: ((q[0] << 16) + q[2], (q[1] << 16) + q[3])
    assert min(FR.dist(at(a), at(b), 1 << 40) for (a, b), _, _ in new) >= LOOP_SEP ** 2
    last = new[-1][0]
    assert last[0][0] > 70 and last[1][0] < 20                             # each one on its own side of the wall, at its goal
