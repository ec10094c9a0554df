"""The fields rule's restatement (tests/route_fields_ref.py) against the routes' and the views' restatements it is built on, and the
assignment across robots on maps drawn for it.  No GPU: the device is compared with the same restatement in test_gpu_route_fields.py."""
import numpy as np
import pytest

from tests import route_fields_ref as RF
from tests import route_ref as RR
from tests import view_ref as VR

CASES = RR.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def convoy():
    out = RF.convoy()
    for a in (out[0], out[2], out[3]):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_minimum_over_the_layers_is_the_joint_field(case):
    name, src, _, p = case
    keys, used = RF.fields(src, p["seeds"], p["free_max"], p["w"], p["limit"])
    joint, n_used = RR.route(src, p["seeds"], p["free_max"], p["w"], p["limit"])
    assert keys.shape == (len(p["seeds"]),) + src.shape and sum(used) == n_used
    assert np.array_equal(keys.min(axis=0), joint), name
    for r, seed in enumerate(p["seeds"]):
        alone, n = RR.route(src, [seed], p["free_max"], p["w"], p["limit"])
        has = alone != RR.NONE
        assert n == used[r] and np.array_equal(keys[r] != RR.NONE, has), (name, r)
        assert np.array_equal(keys[r][has] >> 4, alone[has] >> 4) and ((keys[r][has] & 15) == r).all(), (name, r)
        if not used[r]:
            assert not has.any()


def test_convoy_the_rear_robot_gets_a_goal_only_on_its_own_field(convoy):
    m, seeds, joint, matrix = convoy
    assert [tuple(g)[:3] for g in joint] == [(2318, 34, 0), (2328, 84, 0), (2360, 244, 0)]
    assert matrix.shape == (2, 3) and matrix["cell"].tolist() == [[2318, 2328, 2360]] * 2
    assert matrix["dist"].tolist() == [[34, 84, 244], [74, 124, 284]] and matrix["seed"].tolist() == [[0] * 3, [1] * 3]
    assert matrix[0].tobytes() == joint.tobytes()
    goal_of, _, rounds, _ = VR.assign(m, joint, 2, 10, 1)
    assert goal_of.tolist() == [0, -1] and rounds == 1
    goal_of, picked, rounds, claims = RF.assign_fields(m, matrix, 10, 1)
    assert goal_of.tolist() == [0, 1] and rounds == 2
    assert picked["cell"].tolist() == [2318, 2328] and (picked["gain"] > 0).all()
    want = VR.claim(m, np.zeros(m.shape, dtype=np.uint8), [2318, 2328], 10)
    assert np.array_equal(claims, want) and claims.any()
    # the second round saw the first one's claim
    assert picked[1]["gain"] == VR.gains(m, [2328], 10, claims=VR.claim(m, np.zeros(m.shape, dtype=np.uint8), [2318], 10))[0]["gain"]


def _matrix(rows):
    """a goal matrix from rows of (cell, dist) or None"""
    out = np.zeros((len(rows), len(rows[0])), dtype=RR.GOAL_DTYPE)
    for r, row in enumerate(rows):
        for f, g in enumerate(row):
            out[r, f] = (RR.NONE, RR.NONE, -1, 0) if g is None else (g[0], g[1], r, 0)
    return out


def _table(gain_of):
    """a stand-in for view_ref.gains: the gain of a cell from a table, claims ignored"""
    def gains(m, cells, R, free_max=0, unknown_depth=0, claims=None):
        out = np.zeros(len(cells), dtype=VR.GAIN_DTYPE)
        for n, c in enumerate(cells):
            out[n] = (c, gain_of[int(c)], gain_of[int(c)], gain_of[int(c)])
        return out
    return gains


M = np.zeros((8, 8), dtype=np.int8)            # (no unknown cell: the claims of the stand-in's picks are empty)


def test_a_pair_with_gain_0_never_wins():
    # frontier 0 scores best by far but uncovers nothing: it does not compete, and frontier 1 still goes to a robot
    goals = _matrix([[(10, 0), (11, 500)], [(10, 1), (11, 600)]])
    goal_of, picked, rounds, _ = RF.assign_fields(M, goals, 3, 1, gains=_table({10: 0, 11: 7}))
    assert goal_of.tolist() == [1, -1] and picked["gain"].tolist() == [7, 0] and rounds == 2
    # every gain 0: nobody competes, one round
    goal_of, picked, rounds, claims = RF.assign_fields(M, goals, 3, 1, gains=_table({10: 0, 11: 0}))
    assert goal_of.tolist() == [-1, -1] and picked["cell"].tolist() == [RR.NONE] * 2 and rounds == 1 and not claims.any()
    # on a real map: all known, so every view's gain is 0
    goal_of, _, rounds, claims = RF.assign_fields(M, goals, 3, 1)
    assert goal_of.tolist() == [-1, -1] and rounds == 1 and not claims.any()


def test_more_robots_than_frontiers():
    goals = _matrix([[(10, 30)], [(10, 10)], [(10, 20)]])
    goal_of, picked, rounds, _ = RF.assign_fields(M, goals, 3, 1, gains=_table({10: 5}))
    assert goal_of.tolist() == [-1, 0, -1] and picked["cell"].tolist() == [RR.NONE, 10, RR.NONE] and rounds == 1
    goal_of, _, rounds, _ = RF.assign_fields(M, np.zeros((3, 0), dtype=RR.GOAL_DTYPE), 3, 1)
    assert goal_of.tolist() == [-1, -1, -1] and rounds == 0


def test_a_robot_whose_seed_is_unused_gets_nothing(convoy):
    m, _, _, _ = convoy
    from tests import frontier_ref as FR
    seeds = [(12, 42), (0, 0), (4, 42)]                      # (0, 0) is unknown space: not used
    rec, lab, _ = FR.frontiers(m, 0, 1, seeds)
    keys, used = RF.fields(m, seeds)
    assert used == [1, 0, 1] and (keys[1] == RR.NONE).all()
    matrix = RF.goal_matrix(keys, lab, rec)
    assert (matrix[1]["cell"] == RR.NONE).all() and (matrix[1]["seed"] == -1).all()
    goal_of, _, rounds, _ = RF.assign_fields(m, matrix, 10, 1)
    assert goal_of.tolist() == [0, -1, 1] and rounds == 2


def test_the_tie_order_is_f_then_r():
    gains = _table({10: 5, 11: 5, 12: 5})
    # all four pairs score 5 - 3: frontier 0 first, and of its two robots robot 0; then frontier 1 to robot 1
    goals = _matrix([[(10, 3), (11, 3)], [(10, 3), (11, 3)]])
    goal_of, _, rounds, _ = RF.assign_fields(M, goals, 3, 1, gains=gains)
    assert goal_of.tolist() == [0, 1] and rounds == 2
    # the lower f beats the lower r: robot 1's pair on frontier 0 ties with robot 0's pair on frontier 1
    goals = _matrix([[None, (11, 3)], [(10, 3), (12, 3)]])
    goal_of, _, rounds, _ = RF.assign_fields(M, goals, 3, 1, gains=gains)
    assert goal_of.tolist() == [1, 0] and rounds == 2
    # a higher score beats both
    goals = _matrix([[(10, 3), (11, 3)], [(10, 3), (12, 2)]])
    goal_of, _, _, _ = RF.assign_fields(M, goals, 3, 1, gains=gains)
    assert goal_of.tolist() == [0, 1]


def test_the_library_exports_the_fields_entries(hip_lib):
    from ohm_tsd_slam_amd import capi
    for name in ("tsd_route_fields_dev", "tsd_route_fields_frame", "tsd_route_fields_goals", "tsd_route_fields_goals_fetch",
                 "tsd_route_fields_trace", "tsd_route_fields_waypoints", "tsd_route_fields_dev_ptrs", "tsd_route_fields_counts",
                 "tsd_view_assign_fields"):
        assert name in capi.ABI and getattr(hip_lib, name) is not None
    assert hip_lib.tsd_abi_sizeof(b"tsd_route_fields_info") == 96
