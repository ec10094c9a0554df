"""The view rule without a GPU: the numpy restatement of tests/view_ref.py (what the device is compared with, byte for byte, in
tests/test_gpu_view.py) against a scalar statement of the rule that walks one ray at a time, the closed form on open maps, the named
numbers of the room, its door and the diagonal wall, the claims' algebra and the assignment; the ABI's struct sizes and symbols."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import view_ref as V

CASES = V.cases()
IDS = [c[0] for c in CASES]


def sgn(a):
    return (a > 0) - (a < 0)


def scalar_view(m, cell, R, free_max=0, unknown_depth=0, cut_test=True):
    """V(cell) as a set of (x, y), ray by ray and step by step, every test written as the rule states it"""
    H, W = m.shape
    if cell >= W * H:
        return set()
    cx, cy = cell % W, cell // W

    def inside(x, y):
        return 0 <= x < W and 0 <= y < H

    def blocking(x, y):
        return int(m[y, x]) > free_max

    if blocking(cx, cy):
        return set()
    seen = {(cx, cy)}
    for tx, ty in V.targets(R).tolist():
        px, py, unknowns = cx, cy, 0
        for j in range(1, R + 1):
            ox, oy = sgn(tx) * ((2 * j * abs(tx) + R) // (2 * R)), sgn(ty) * ((2 * j * abs(ty) + R) // (2 * R))
            x, y = cx + ox, cy + oy
            if ox * ox + oy * oy > R * R:
                break
            if not inside(x, y):
                break
            if cut_test and x != px and y != py and all(not inside(a, b) or blocking(a, b) for a, b in ((x, py), (px, y))):
                break
            if blocking(x, y):
                break
            seen.add((x, y))
            if m[y, x] < 0 and unknown_depth > 0:
                unknowns += 1
                if unknowns == unknown_depth:
                    break
            px, py = x, y
    return seen


def as_set(mask):
    ys, xs = np.nonzero(mask)
    return set(zip(xs.tolist(), ys.tolist()))


def test_targets_are_the_ring_in_order():
    for R in (1, 2, 3, 16, 511):
        t = V.targets(R)
        assert t.shape == (8 * R, 2) and (np.abs(t).max(axis=1) == R).all() and len(set(map(tuple, t.tolist()))) == 8 * R
        assert t[0].tolist() == [-R, -R] and t[2 * R].tolist() == [R, -R] and t[2 * R + 1].tolist() == [R, -R + 1]
        assert t[4 * R].tolist() == [R, R] and t[6 * R].tolist() == [-R, R] and t[-1].tolist() == [-R, -R + 1]
    assert V.targets(1).tolist() == [[-1, -1], [0, -1], [1, -1], [1, 0], [1, 1], [0, 1], [-1, 1], [-1, 0]]


def test_steps_move_by_at_most_one_cell_and_never_back():
    for R in (1, 2, 7, 32, 33, 511):
        t = np.abs(V.targets(R))
        j = np.arange(0, R + 1)[:, None, None]
        o = (2 * j * t[None] + R) // (2 * R)
        d = np.diff(o, axis=0)
        assert (o[0] == 0).all() and (o[R] == t).all() and (d >= 0).all() and (d <= 1).all() and (d.max(axis=2) == 1).all()


def test_the_reciprocal_divides_exactly():
    """view.hip divides by 2R with a multiplication: floor(n * (floor(2^32 / 2R) + 1) / 2^32) == n / 2R for every n of the rule"""
    for R in range(1, V.MAX_RADIUS + 1):
        n = np.arange(0, 2 * R * R + R + 1, dtype=np.uint64)
        recip = np.uint64((1 << 32) // (2 * R) + 1)
        assert np.array_equal((n * recip) >> np.uint64(32), n // np.uint64(2 * R)), R


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_scalar_statement(case):
    name, m, _, p = case
    for c in sorted(set(p["cells"])):
        got = as_set(V.view(m, c, p["R"], p["free_max"], p["unknown_depth"]))
        assert got == scalar_view(m, c, p["R"], p["free_max"], p["unknown_depth"]), (name, c)


OPEN = [(200, 200, 100, 100), (40, 30, 0, 0), (40, 30, 39, 29), (1, 50, 0, 25), (50, 1, 25, 0), (70, 70, 3, 66)]


@pytest.mark.parametrize("R", [1, 2, 3, 7, 31, 32, 33, 64])
def test_open_map_closed_form(R):
    for W, H, cx, cy in OPEN:
        rec = V.gains(V.open_map(W, H, cx, cy), [cy * W + cx], R)[0]
        n = V.disc_cells(W, H, cx, cy, R)
        assert tuple(rec) == (cy * W + cx, n - 1, n - 1, n), (R, W, H)


def test_open_map_closed_form_at_the_largest_radius():
    rec = V.gains(V.open_map(97, 130, 48, 65), [65 * 97 + 48], 511)[0]
    assert tuple(rec) == (65 * 97 + 48, 97 * 130 - 1, 97 * 130 - 1, 97 * 130)


def test_the_room_and_its_door():
    c = 10 * 21 + 10
    assert tuple(V.gains(V.room(False), [c], 20)[0]) == (c, 0, 0, 81)
    assert tuple(V.gains(V.room(True), [c], 20)[0]) == (c, 7, 7, 89)
    assert tuple(V.gains(V.room(True), [c], 20, 0, 2)[0]) == (c, 2, 2, 84)
    # on the wall, outside the map: nothing, not even the cell itself
    for cell in (5 * 21 + 5, 21 * 21, 0xFFFFFFFE):
        assert tuple(V.gains(V.room(True), [cell], 20)[0]) == (cell, 0, 0, 0)
    # from an unknown cell outside the room the walls are not passed
    v = V.view(V.room(False), 0, 20)
    assert v[0, 0] and not v[5:16, 5:16].any()


def test_a_diagonal_wall_is_a_wall():
    """41 x 41 with an anti-diagonal wall: nothing behind it is seen -- from (5, 5) at R = 31, 110 cells would be without the test
    of the cut cells"""
    m = V.diagonal_wall(41, True)
    c = 5 * 41 + 5
    xs, ys = zip(*as_set(V.view(m, c, 31)))
    assert max(x + y for x, y in zip(xs, ys)) < 40
    leaky = scalar_view(m, c, 31, cut_test=False)
    assert sum(1 for x, y in leaky if x + y > 40) == 110
    m = V.diagonal_wall(41, False)
    assert all(x > y for x, y in as_set(V.view(m, 5 * 41 + 35, 31)))


def test_unknown_depth():
    """a corridor of unknown cells: depth d sees d of them; a clear cell in between does not count"""
    m = np.full((1, 40), V.U, dtype=np.int8)
    m[0, 0] = 0
    for d in (1, 2, 5):
        assert tuple(V.gains(m, [0], 30, 0, d)[0]) == (0, d, d, d + 1)
    assert tuple(V.gains(m, [0], 30, 0, 0)[0]) == (0, 30, 30, 31)
    m[0, 2] = 0
    assert tuple(V.gains(m, [0], 30, 0, 2)[0]) == (0, 2, 2, 4)
    m[0, 0] = V.U                                     # the candidate's own unknown cell is seen, but is no step of a ray
    assert tuple(V.gains(m, [0], 30, 0, 2)[0]) == (0, 3, 3, 4)


def test_claims_are_idempotent_and_independent_of_order():
    name, m, _, p = CASES[IDS.index("fog_97x130_R64_depth3")]
    cells = [65 * 97 + 50, 60 * 97 + 40, 66 * 97 + 58, 0]
    a = V.claim(m, np.zeros(m.shape, dtype=np.uint8), cells, 33, 0, 3)
    b = V.claim(m, np.zeros(m.shape, dtype=np.uint8), cells[::-1], 33, 0, 3)
    assert a.any() and np.array_equal(a, b) and set(np.unique(a)) == {0, 1}
    assert np.array_equal(V.claim(m, a.copy(), cells[:2], 33, 0, 3), a)
    assert not a[m >= 0].any()                        # only unknown cells are claimed
    for c in cells:
        rec = V.gains(m, [c], 33, 0, 3, a)[0]
        assert rec["gain"] == 0 and rec["unknown"] > 0
    near = V.gains(m, [64 * 97 + 62], 33, 0, 3, a)[0]
    assert 0 < near["gain"] < near["unknown"]


def test_assign_sends_the_second_robot_to_the_other_room():
    m, seeds, goals = V.two_rooms()
    W = m.shape[1]
    assert [(int(g["cell"]) % W, int(g["cell"]) // W, int(g["seed"])) for g in goals] == [(15, 36, 0), (25, 36, 1), (56, 36, 1)]
    # the nearest-only choice: every robot takes the nearest of the goals it is nearest to -- both look into the first room
    nearest = [min((int(g["dist"]), k) for k, g in enumerate(goals) if g["seed"] == r)[1] for r in (0, 1)]
    assert nearest == [0, 1]
    plain = V.gains(m, goals["cell"], 12)
    of, picked, rounds, claims = V.assign(m, goals, 2, 12, 10)
    assert of.tolist() == [0, 2] and rounds == 2
    assert picked[0] == plain[0] and picked[1] == plain[2]              # the other room is all new
    assert np.array_equal(claims, V.claim(m, np.zeros(m.shape, dtype=np.uint8), goals["cell"][[0, 2]], 12))
    # what the first robot is about to see is worth less to the second: that is why
    shared = V.gains(m, goals["cell"], 12, claims=V.claim(m, np.zeros(m.shape, dtype=np.uint8), goals["cell"][:1], 12))
    assert shared[1]["gain"] < shared[2]["gain"] == plain[2]["gain"] < plain[1]["gain"]
    # gain_weight 0: by distance alone
    of, picked, rounds, _ = V.assign(m, goals, 2, 12, 0)
    assert of.tolist() == [0, 1] and rounds == 2 and picked[1]["gain"] == shared[1]["gain"]
    # a goal whose gain is 0 ends the rounds; goals without a cell or of a seed that is no robot are not remaining
    done = goals.copy()
    done["cell"][1:] = V.NONE
    of, _, rounds, _ = V.assign(m, done, 2, 12, 10)
    assert of.tolist() == [0, -1] and rounds == 1
    of, _, rounds, _ = V.assign(m, goals, 1, 12, 10)
    assert of.tolist() == [0] and rounds == 1
    walled = m.copy()
    walled[m < 0] = 0
    of, picked, rounds, claims = V.assign(walled, goals, 2, 12, 10)
    assert of.tolist() == [-1, -1] and rounds == 1 and (picked["cell"] == V.NONE).all() and not claims.any()


def test_struct_sizes(hip_lib):
    assert hip_lib.tsd_abi_sizeof(b"tsd_view_params") == C.sizeof(capi.ViewParams) == 16
    assert hip_lib.tsd_abi_sizeof(b"tsd_view_gain") == C.sizeof(capi.ViewGain) == capi.VIEW_GAIN_DTYPE.itemsize == 16
    assert capi.VIEW_GAIN_DTYPE == V.GAIN_DTYPE and capi.VIEW_MAX_RADIUS == V.MAX_RADIUS and capi.VIEW_MAX_CELLS == V.MAX_CELLS


def test_the_library_has_the_view_entries(hip_lib):
    for name in ("tsd_view_gains", "tsd_view_claim", "tsd_view_claims_reset", "tsd_view_claims_dev_ptr", "tsd_view_assign"):
        assert name in capi.ABI and getattr(hip_lib, name) is not None, name
