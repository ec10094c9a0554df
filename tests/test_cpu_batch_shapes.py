"""The scenarios of tests/batch_shapes_ref.py reach the branches they are meant for -- shown with the ORACLE alone (no device): every
scenario is run round by round with Robot.localise / apply_push of tests/test_gpu_batch.py, og.dump() is taken around every robot's
push and the dumps are diffed (batch_shapes_ref.push_effect) to see which tiles that robot updated or emptied.  These are conditions
on the scenarios: tests/test_gpu_batch_shapes.py runs the same scenarios on the device and is only worth its time if they hold.  A
scenario edited so that its branch is no longer reached fails here (e.g. mixed_five with the robot that stands on the pool tile moved
to the end of the batch order: "neither first nor last" below)."""
import functools

import pytest

from tests import batch_shapes_ref as B

MIXED = ["mixed_two_360_first", "mixed_two_1081_first", "mixed_three_fov", "mixed_five", "robot0_gated_mixed", "mixed_mode3"]


@functools.lru_cache(maxsize=None)
def _run_cached(name):
    from oracle import pyoracle
    pyoracle.build()
    scn = B.SCENARIOS[name]
    if scn.armed:
        # (the pre-registration changes where a registration starts, not who sees which tile: the plain registration is what the
        # coverage conditions are about, and mode 3's own draws are the GPU test's business)
        scn = B.Scenario(scn.name, scn.geos, scn.offsets, scn.moves, armed=False)
    return scn, B.drive(pyoracle, scn, device=False, effects=True)


def _pushed(run):
    return [[ro["pushed"] for ro in ros] for ros in run["ros"]]


@pytest.mark.parametrize("name", sorted(B.SCENARIOS))
def test_every_robot_registers_and_pushes(oracle, name):
    """no registration error, no round without a model, every robot pushes at least once -- in every scenario"""
    scn, run = _run_cached(name)
    assert len(run["ros"]) == scn.rounds and 3 <= scn.rounds <= 5
    for k, ros in enumerate(run["ros"], 1):
        for i, ro in enumerate(ros):
            assert not ro["reg_error"] and not ro["no_model"], f"round {k} robot {i}: {ro}"
            assert ro["pairs"] > 0 and ro["iterations"] > 0
    pushed = _pushed(run)
    for i in range(scn.n):
        assert any(p[i] for p in pushed), f"robot {i} never pushes"


@pytest.mark.parametrize("name", MIXED)
def test_mixed_scenarios_have_a_tile_updated_by_two_resolutions(oracle, name):
    """k_mp_update's own_rot: in some round one tile is UPDATED by a robot with robot 0's resolution and by one with another --
    robot 0 itself among the updating robots, so both the staged table and a table read from memory serve the same tile"""
    scn, run = _run_cached(name)
    res0 = scn.geos[0].angle_increment
    assert any(g.angle_increment != res0 for g in scn.geos)
    hit = False
    for eff in run["effects"]:
        tiles = set.union(*[e["updated"] for e in eff])
        for p in tiles:
            who = [i for i, e in enumerate(eff) if p in e["updated"]]
            if any(scn.geos[i].angle_increment == res0 for i in who) and any(scn.geos[i].angle_increment != res0 for i in who):
                hit = True
    assert hit


def test_mixed_three_fov_shares_robot_0s_table_with_another_window(oracle):
    """the 270-beam scanner has robot 0's resolution (it takes robot 0's table out of LDS) but another phi_min and beam count, and
    updates a tile that robot 0 and the 1081-beam robot update in the same round"""
    scn, run = _run_cached("mixed_three_fov")
    assert scn.geos[1].angle_increment == scn.geos[0].angle_increment and scn.geos[1].beams != scn.geos[0].beams
    assert scn.geos[1].angle_min != scn.geos[0].angle_min and scn.geos[2].angle_increment != scn.geos[0].angle_increment
    assert any(e[0]["updated"] & e[1]["updated"] & e[2]["updated"] for e in run["effects"])


def test_mixed_five_reaches_the_pool_spill(oracle):
    """The scan-window pool of k_mp_update (push_multi.hip) holds Bp = 1084 beams in mixed_five (the widest scanner's 1081, rounded up
    to 4).  In some round the tile POOL_TILE is updated by at least three robots, and POOL_ROBOT -- neither first nor last in batch
    order -- stands on it when it pushes.

    Why its window is its whole scan: tile_in_range (push_device.hpp) presets `win` to 0 | (beams - 1) << 16 and narrows it to the
    corners' beams only where the sensor is farther than three tile radii from the tile's centroid; a sensor INSIDE the tile is at most
    one radius away.  k_mp_update widens by one beam and clamps to [0, beams - 1]: len = beams = 1081 for POOL_ROBOT.  The pool is
    filled in batch order while `off + len <= Bp`; an earlier robot that updates the tile has pooled a window of at least 4 beams
    (asserted below from the tile's corners), so 1081 more do not fit: s_off = -1, the window is staged on the robot's turn at the
    pool's START (`pool < 0`).  A LATER robot's short window still fitted behind the earlier ones (asserted below with the upper
    bounds of every earlier window) and lies at an offset below 1081 -- under the staged scan -- so the invalidation of later robots'
    pooled windows (`s_off[q] = -1` for q > r) is what keeps that robot from reading POOL_ROBOT's ranges."""
    scn, run = _run_cached("mixed_five")
    gc = run["gc"]
    PX = gc.cells // B.TILE_DIM
    p = B.POOL_TILE[1] * PX + B.POOL_TILE[0]
    m = B.POOL_ROBOT
    assert 0 < m < scn.n - 1, "the robot on the pool tile is neither first nor last in batch order"
    Bp = (max(g.beams for g in scn.geos) + 3) & ~3
    reached = False
    for eff, poses in zip(run["effects"], run["push_poses"]):
        who = [i for i, e in enumerate(eff) if p in e["updated"]]
        if len(who) < 3 or m not in who:
            continue
        x, y = poses[m][0, 2], poses[m][1, 2]
        on_tile = int(x / gc.cell_size) // B.TILE_DIM == B.POOL_TILE[0] and int(y / gc.cell_size) // B.TILE_DIM == B.POOL_TILE[1]
        cx, cy, rad, _ = B.tile_geometry(gc, p)
        if not on_tile:
            continue
        assert (x - cx) ** 2 + (y - cy) ** 2 <= rad * rad
        assert B.window_bounds(gc, scn.geos[m], poses[m], p) == (scn.geos[m].beams,) * 2
        earlier = [B.window_bounds(gc, scn.geos[i], poses[i], p) for i in who if i < m]
        later = [(i, B.window_bounds(gc, scn.geos[i], poses[i], p)) for i in who if i > m]
        if not earlier or any(w is None for w in earlier):
            continue
        spill = max(w[0] for w in earlier) >= 4 and scn.geos[m].beams + 4 > Bp
        most, pooled_later = sum(w[1] for w in earlier), []
        for i, w in later:          # (batch order; a window that may or may not have fitted is counted as if it took its room)
            hi = scn.geos[i].beams if w is None else w[1]
            if w is not None and most + hi <= Bp:
                pooled_later.append(i)
            most += hi
        if spill and pooled_later:
            reached = True
    assert reached, "no round in which the robot on the pool tile spills while a later robot's window is pooled"


@pytest.mark.parametrize("name", ["robot0_gated_one_scanner", "robot0_gated_mixed"])
def test_gating_pattern_holds_exactly(oracle, name):
    """rounds 2-3: robot 0 gated out while both others push; round 4: nobody pushes; rounds 1 and 5: everybody"""
    scn, run = _run_cached(name)
    assert _pushed(run) == [[1, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 0], [1, 1, 1]]
    if name == "robot0_gated_mixed":
        assert scn.geos[0].angle_increment != scn.geos[1].angle_increment == scn.geos[2].angle_increment, "robot 0 is the odd scanner"
    for k in (1, 2):        # (rounds 2-3) the others' updates happen on tiles, with robot 0's push disabled
        assert not run["effects"][k][0]["changed"] and run["effects"][k][1]["updated"] and run["effects"][k][2]["updated"]
    assert not any(e["changed"] for e in run["effects"][3])


@pytest.mark.parametrize("name", ["n16", "n17"])
def test_robot_15_updates_and_empties(oracle, name):
    """robot 15 owns the highest bits of the per-tile mask (15: updates, 31: empties, right under MP_DIRTY = 1 << 32): it updates at
    least one tile, and in some round a tile that was materialised before its push goes through increaseEmptiness by it -- every cell
    of the tile one unit of weight up, no measurement averaged in (TsdGridPartition.cpp:136-164)"""
    scn, run = _run_cached(name)
    assert scn.n == int(name[1:]) and all(g.beams == 360 for g in scn.geos)
    assert len(set((o[0], o[1]) for o in scn.offsets)) == scn.n, "distinct starts"
    assert any(e[15]["updated"] for e in run["effects"])
    assert any(e[15]["emptied"] for e in run["effects"])
    for i in range(scn.n):
        assert all(p[i] for p in _pushed(run)), f"robot {i} pushes every round"
