"""The drive rule without a GPU: the direction table and tsd_drive_advance of the library (host code) against their statement in
include/tsd_hip.h, and the properties of the rule itself on the restatement of tests/drive_ref.py, which reads the table through
tsd_drive_table and is what tests/test_gpu_drive.py holds the kernel against."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_ref as DR
from tests import route_ref as RR

H = DR.H


@pytest.fixture(scope="module")
def cases():
    return DR.cases()


def test_the_abi_declares_the_drive_calls(hip_lib):
    for name in ("tsd_drive_table", "tsd_drive_advance", "tsd_drive_rollout", "tsd_drive_fields_rollout"):
        assert name in capi.ABI and getattr(hip_lib, name) is not None
    assert (capi.DRIVE_HEADINGS, capi.DRIVE_MAX_STEPS, capi.DRIVE_MAX_SPEEDS, capi.DRIVE_MAX_TURNS, capi.DRIVE_MAX_BODY,
            capi.DRIVE_MAX_ROBOTS) == (4096, 256, 64, 129, 64, 16)
    assert C.sizeof(capi.DriveParams) == 64 and C.sizeof(capi.DrivePose) == 24 and C.sizeof(capi.DriveChoice) == 40
    assert capi.DRIVE_CHOICE_DTYPE.itemsize == 40 and capi.DRIVE_POSE_DTYPE.itemsize == 24 and capi.DRIVE_CHOICE_DTYPE == DR.CHOICE_DTYPE


# ---- the table
def test_table_axes_and_symmetries():
    D = DR.table()
    assert D.shape == (H, 2) and capi.drive_table().dtype == np.int32
    assert tuple(D[0]) == (65536, 0) and tuple(D[H // 4]) == (0, 65536) and tuple(D[H // 2]) == (-65536, 0) and tuple(D[3 * H // 4]) == (0, -65536)
    h = np.arange(H)
    assert np.array_equal(D[(h + H // 2) % H], -D)                                        # the half turn
    assert np.array_equal(D[(h + H // 4) % H], np.stack([-D[:, 1], D[:, 0]], axis=1))     # the quarter turn
    assert np.array_equal(D[(-h) % H], np.stack([D[:, 0], -D[:, 1]], axis=1))             # the mirror at the x axis
    assert np.array_equal(D[(H // 4 - h) % H], D[:, ::-1])                                # the mirror at the diagonal: the octants
    assert (np.diff(D[:H // 4 + 1, 0]) <= 0).all() and (np.diff(D[:H // 4 + 1, 1]) >= 0).all()


def test_table_entries_lie_on_the_circle():
    """cx = 65536 cos + e1, cy = 65536 sin + e2 with |e1|, |e2| <= 1/2 (lrint), so
    cx^2 + cy^2 - 2^32 = 2 * 65536 (e1 cos + e2 sin) + e1^2 + e2^2, at most 65536 (|cos| + |sin|) + 1/2 in magnitude.  With
    65536 |cos| <= |cx| + 1/2 that is at most |cx| + |cy| + 3/2, and the left side is an integer: |cx^2 + cy^2 - 2^32| <= |cx| + |cy| + 1."""
    D = DR.table()
    err = np.abs(D[:, 0] ** 2 + D[:, 1] ** 2 - (1 << 32))
    assert (err <= np.abs(D[:, 0]) + np.abs(D[:, 1]) + 1).all(), int(err.max())
    assert err.max() > 0                                                                   # (the bound is not idle: some entry is rounded)


def test_table_refuses_a_null_pointer(hip_lib):
    assert hip_lib.tsd_drive_table(None) == -1


# ---- tsd_drive_advance
ADVANCES = [((5, 7, 0, 0, 0, 3), 65536, 0, 10), ((5, 7, 65535, 65535, H // 8, 0), 65536, 1, 1),          # an offset that carries into the cell
            ((5, 7, 100, 200, 3, 0), 40000, -1, 9),                                                          # the heading wraps below 0
            ((5, 7, 100, 200, H - 2, 1), 40000, 1, 9),                                                       # ... and above H - 1
            ((-1000, 1 << 30, 1, 65535, H - 1, 15), 65536, 512, 256), ((0, 0, 0, 0, 0, 0), 65536, -512, 256),
            ((9, 9, 32768, 32768, 1234, 0), 0, 77, 200), ((9, 9, 32768, 32768, 1234, 0), 1, -77, 200), ((9, 9, 32768, 32768, 1234, 0), 12345, 5, 0)]


@pytest.mark.parametrize("pose,s,t,n", ADVANCES)
def test_advance_equals_the_restatement(pose, s, t, n):
    got = capi.drive_advance(pose, s, t, n)
    want = DR.advance(pose, s, t, n)
    assert tuple(int(got[f]) for f in ("x", "y", "fx", "fy", "heading")) == want and int(got["layer"]) == pose[5]
    assert 0 <= want[2] <= 65535 and 0 <= want[3] <= 65535 and 0 <= want[4] < H
    # n steps at once are n single steps of the trajectory only for t = 0 (the heading of step k is h0 + k t): the rule's own identity
    tr = DR.trajectory(pose, s, t, n)
    assert (want[0], want[1]) == (tr[n][3], tr[n][4]) and want[4] == (tr[n][2] if n else pose[4])


def test_advance_in_place_and_its_refusals(hip_lib):
    p = capi.drive_poses([(5, 7, 100, 200, 3, 2)])
    want = DR.advance((5, 7, 100, 200, 3, 2), 65536, 2, 5)
    assert hip_lib.tsd_drive_advance(p.ctypes.data, 65536, 2, 5, p.ctypes.data) == 0          # out may be p
    assert tuple(int(p[0][f]) for f in ("x", "y", "fx", "fy", "heading", "layer")) == want + (2,)
    good = (5, 7, 100, 200, 3, 0)
    out = np.full(6, 0x5A5A5A5A, dtype=np.int32)

    def call(pose=good, s=65536, t=0, n=1, p_null=False, out_null=False):
        q = capi.drive_poses([pose])
        return hip_lib.tsd_drive_advance(None if p_null else q.ctypes.data, s, t, n, None if out_null else out.ctypes.data)

    assert call() == 0
    out[:] = 0x5A5A5A5A
    bad = [dict(p_null=True), dict(out_null=True), dict(pose=(5, 7, -1, 0, 0, 0)), dict(pose=(5, 7, 65536, 0, 0, 0)), dict(pose=(5, 7, 0, -1, 0, 0)),
           dict(pose=(5, 7, 0, 65536, 0, 0)), dict(pose=(5, 7, 0, 0, -1, 0)), dict(pose=(5, 7, 0, 0, H, 0)), dict(pose=((1 << 30) + 1, 7, 0, 0, 0, 0)),
           dict(pose=(5, -(1 << 30) - 1, 0, 0, 0, 0)), dict(s=-1), dict(s=65537), dict(t=H // 8 + 1), dict(t=-H // 8 - 1), dict(n=-1), dict(n=257)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert (out == 0x5A5A5A5A).all()
    for kw in (dict(s=0), dict(s=65536), dict(t=H // 8), dict(t=-H // 8), dict(n=0), dict(n=256), dict(pose=(1 << 30, -(1 << 30), 65535, 65535, H - 1, 0))):
        assert call(**kw) == 0, kw


# ---- the rule, on the restatement
def _open(W=40, Hh=30):
    m = np.zeros((Hh, W), dtype=np.int8)
    return RR.route(m, [(W - 2, Hh - 2)])[0], RR.weight_image(m)


def test_heading_zero_at_full_speed_visits_one_cell_per_step():
    keys, wi = _open()
    for fx, fy in ((0, 0), (32768, 65535), (65535, 1)):
        tr = DR.trajectory((3, 4, fx, fy, 0, 0), 65536, 0, 30)
        assert [(c[3], c[4]) for c in tr] == [(3 + k, 4) for k in range(31)]
        tr = DR.trajectory((3, 4, fx, fy, H // 4, 0), 65536, 0, 20)
        assert [(c[3], c[4]) for c in tr] == [(3, 4 + k) for k in range(21)]
    choice, scores, why = DR.rollout(keys, wi, (3, 4, 100, 100, 0, 0), 30, [65536], [0])
    assert why[0, 0] == 0 and choice["end_cell"] == 4 * 40 + 33 and choice["cost"] == 30
    choice, scores, why = DR.rollout(keys, wi, (3, 4, 100, 100, 0, 0), 37, [65536], [0])
    assert why[0, 0] == (1 << 12) | 37 and choice["speed"] == -1 and choice["score"] == DR.DRIVE_NONE      # x = 40 is outside


def test_speed_zero_stays_on_its_cell(cases):
    """s = 0 never leaves the start's cell, whatever the offset, the heading and the turn.  The start pose is not tested, but c_1 is,
    and with s = 0 it is the start's cell: the sample is admissible on every cell that is traversable and has a key -- beside a wall,
    on the border, in a corner -- and is refused by reason 2 (or 5) at the first step on any other."""
    c = cases["random_67x50"]
    keys, wi = c["keys"], c["wi"]
    turn = [0, 1, -1, 512, -512]
    seen = set()
    for y in range(0, 50, 7):
        for x in range(0, 67, 3):
            choice, scores, why = DR.rollout(keys, wi, (x, y, 65535, 0, (37 * x + y) % H, 0), 256, [0], turn, weights=(1, 0, 1, 0))
            if wi[y, x] == 0:
                assert (why == (2 << 12) | 1).all()
            elif keys[y, x] == RR.NONE:
                assert (why == (5 << 12) | 256).all()
            else:
                assert (why == 0).all() and choice["end_cell"] == y * 67 + x and choice["cost"] == 256 * wi[y, x] and choice["admissible"] == 5
                assert (scores == (int(keys[y, x]) >> 4) + 256 * int(wi[y, x])).all() and (choice["speed"], choice["turn"]) == (0, 0)
            seen.add(int(why[0, 0]) >> 12)
    assert seen >= {0, 2}


def test_one_blocked_corner_refuses_a_diagonal_step():
    m = np.zeros((20, 20), dtype=np.int8)
    for x in range(12):
        m[11 - x, x] = RR.O                                      # a wall down the anti-diagonal x + y = 11 ...
    m[6, 5] = 0                                                  # ... with the cell (5, 6) taken out
    keys, wi = RR.route(m, [(15, 15)])[0], RR.weight_image(m)
    arc = dict(steps=3, step_q16=[65536], turn=[0])
    # (5, 5) -> (6, 6) cuts (5, 6), free, and (6, 5), wall: ONE blocked corner refuses
    _, _, why = DR.rollout(keys, wi, (5, 5, 32768, 32768, H // 8, 0), **arc)
    assert why[0, 0] == (3 << 12) | 1
    assert DR.sample(keys, wi, (5, 5, 32768, 32768, H // 8, 0), 65536, 0, 3)[0] == (3 << 12) | 1
    # the same arc one cell aside: (4, 5) -> (5, 6) -> (6, 7) goes through the gap and cuts free cells only
    choice, _, why = DR.rollout(keys, wi, (4, 5, 32768, 32768, H // 8, 0), **arc)
    assert why[0, 0] == 0 and choice["end_cell"] == 7 * 20 + 6
    # with the second corner taken out as well the first arc passes
    m[5, 6] = 0
    keys, wi = RR.route(m, [(15, 15)])[0], RR.weight_image(m)
    assert DR.rollout(keys, wi, (5, 5, 32768, 32768, H // 8, 0), **arc)[2][0, 0] == 0


def test_a_body_point_refuses_where_the_centre_passes():
    m = np.zeros((20, 20), dtype=np.int8)
    m[6, 10] = RR.O
    keys, wi = RR.route(m, [(18, 5)])[0], RR.weight_image(m)
    pose = (5, 5, 32768, 32768, 0, 0)
    assert DR.rollout(keys, wi, pose, 10, [65536], [0])[2][0, 0] == 0
    assert DR.rollout(keys, wi, pose, 10, [65536], [0], body=[(0, -65536)])[2][0, 0] == 0              # the right-hand point passes too
    for body in ([(0, 65536)], [(0, -65536), (0, 65536)], [(0, 65536), (3 * 65536, 0)]):                  # the left-hand point meets (10, 6)
        assert DR.rollout(keys, wi, pose, 10, [65536], [0], body=body)[2][0, 0] == (4 << 12) | 5
    assert DR.rollout(keys, wi, pose, 10, [65536], [0], body=[(65536, 65536)])[2][0, 0] == (4 << 12) | 4   # a point ahead on the left: a step sooner
    assert DR.rollout(keys, wi, pose, 10, [65536], [0], body=[(-(1 << 22), 0)])[2][0, 0] == (4 << 12) | 1   # 64 cells behind: outside the map
    # turned by a quarter the same point lies behind the robot's left: heading H/4 looks along +y, its left is -x
    pose = (11, 1, 32768, 32768, H // 4, 0)
    assert DR.rollout(keys, wi, pose, 10, [65536], [0], body=[(0, 65536)])[2][0, 0] == (4 << 12) | 5


def test_ties_go_to_the_lowest_index():
    keys, wi = _open()
    pose = (3, 4, 0, 0, 0, 0)
    choice, scores, why = DR.rollout(keys, wi, pose, 5, [65536, 65536, 100], [0, 0, 7], weights=(0, 0, 0, 0))
    assert (scores == 0).all() and (choice["speed"], choice["turn"], choice["admissible"]) == (0, 0, 9)
    choice, scores, why = DR.rollout(keys, wi, pose, 5, [30000, 65536, 65536], [3, 0, 0], weights=(1, 0, 0, 0))
    assert scores[1, 1] == scores[1, 2] == scores[2, 1] == scores[2, 2] == scores.min() and (choice["speed"], choice["turn"]) == (1, 1)
    # where the preferred sample is refused the next index takes the tie
    pose = (37, 4, 0, 0, 0, 0)
    choice, scores, why = DR.rollout(keys, wi, pose, 5, [65536, 0, 0], [0, 0], weights=(0, 0, 0, 0))
    assert (why[0] == (1 << 12) | 3).all() and (choice["speed"], choice["turn"], choice["admissible"]) == (1, 0, 4)


def test_the_two_forms_of_the_restatement_agree(cases):
    """``rollout`` (numpy over the samples) against ``sample`` (the rule step by step)"""
    kw = dict(body=[(65536, 30000), (-70000, 0)], weights=(3, 2, 1, 5), nose_q16=200000, nose_miss=77)
    speeds, turn = [65536, 40000, 0], [0, 5, -5, 100, -100]
    reasons = set()
    for name, c in cases.items():
        Hh, W = c["keys"].shape
        for pose in ((5, 5, 100, 65535, 17, 0), (30, 20, 65535, 65535, H - 1, 0), (0, 0, 0, 0, H // 2, 0), (W - 1, Hh - 2, 9, 9, 3 * H // 4 + 100, 0)):
            choice, scores, why = DR.rollout(c["keys"], c["wi"], pose, 20, speeds, turn, **kw)
            best = None
            for i, s in enumerate(speeds):
                for j, t in enumerate(turn):
                    w, score, rec = DR.sample(c["keys"], c["wi"], pose, s, t, 20, **kw)
                    assert (w, score) == (int(why[i, j]), int(scores[i, j])), (name, pose, i, j)
                    reasons.add(w >> 12)
                    if w == 0 and (best is None or (score, i * len(turn) + j) < best[0]):
                        best = ((score, i * len(turn) + j), (i, j) + rec)
            if best is None:
                assert choice["speed"] == -1 and choice["score"] == DR.DRIVE_NONE
            else:
                assert tuple(choice)[:2] + tuple(choice)[3:7] == best[1] and choice["score"] == best[0][0]
    assert reasons == {0, 1, 2, 3, 4, 5}


def test_closed_loop_through_the_door(cases):
    """The robot starts left of the wall looking away from the doorway, takes the first step of every choice (tsd_drive_advance of the
    library) and rolls out again.  Integer arithmetic throughout, so the run is the same everywhere: it takes 101 commands here --
    the first one on the spot (no forward arc is better than standing: the nose term picks the rotation), then a tight arc round
    towards the doorway, through it and on to the goal -- and the cap is 120."""
    c = cases["door_96x64"]
    keys, wi = c["fields"][0], c["wi"]
    p = DR.loop_params()
    log = DR.closed_loop(lambda pose: DR.rollout(keys, wi, pose, **p),
                         lambda pose, s, t: tuple(int(v) for v in capi.drive_advance(pose, s, t, 1)), 120, keys, wi)
    assert len(log) == 101
    poses = [l[0] for l in log]
    assert p["step_q16"][log[0][1]] == 0 and p["turn"][log[0][2]] != 0                   # it turns where it stands, first of all
    assert poses[1][:2] == DR.LOOP_START[:2] and poses[1][4] != DR.LOOP_START[4]
    assert any(p["turn"][l[2]] != 0 and p["step_q16"][l[1]] > 0 for l in log[1:12])      # ... and on while it drives
    assert any(q[0] == 48 and 30 <= q[1] <= 33 for q in poses)                           # through the doorway
    assert poses[-1][0] > 70 and all(wi[q[1], q[0]] > 0 for q in poses)
    # the field falls along the way once the robot drives (the nose term turned it first)
    d = [int(keys[q[1], q[0]]) >> 4 for q in poses]
    assert d[-1] < d[0] and d[1] == d[0]
