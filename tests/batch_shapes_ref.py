"""Scenarios for the batched multi-robot path (tsd_batch_*) at its shape edges -- scanners of different beam counts and resolutions in
one batch, 5 / 16 / 17 robots, rounds in which robot 0 or everybody is gated out of the push -- and the one driver that runs a
scenario on the oracle's primitives (tests/test_gpu_batch.py's Robot: every localisation of a round against the grid as it is before
the round's pushes, the pushes in batch order) and, beside it, on the device.  tests/test_cpu_batch_shapes.py asserts with the oracle
alone that every scenario reaches the branch it is meant for; tests/test_gpu_batch_shapes.py compares the device with the oracle.

What a batch decides from its widest scanner and its size (csrc/capi_scan.hip tsd_batch_begin / tsd_batch_push, icp_shape.hpp,
push_multi.hip): the registrations' workgroup shape and the helper grid, the ray cast's and the tables' launch width, the push's scan
pool, by-value or copied ray-cast entries (16 / 17), the one-pass or the serial pushes (16 / 17), helpers on or off (4 / 5)."""
import math
from dataclasses import dataclass

import numpy as np

from ohm_tsd_slam_amd import synth
from tests import helpers as H

GEO360 = synth.ScanGeometry.full_circle_360()
GEO1081 = synth.ScanGeometry.utm30lx()
GEO270 = synth.ScanGeometry(270, math.radians(-135.0), 2.0 * math.pi / 360.0)      # the 360's resolution, another field of view

CFG = "cfg1"                      # 2^9 cells of 0.05 m, scene "room" (16 m x 12 m around the grid's centre)
# one move.  Twice the push gate (0.05 m): the registration of a 360-beam scan in the room follows a step along the long walls only in
# part (30 iterations, MAXITERATIONS: the reference's behaviour, oracle and device alike), and the planned push patterns need every
# moving robot over the gate in every round (0.06 m as in synth.trajectory is not enough: test_cpu_batch_shapes.py would say so)
STEP_X, STEP_YAW = 0.1, 0.01
TILE_DIM, TILE_CELLS, MAX_WEIGHT = 32, 33 * 33, 32.0


@dataclass
class Scenario:
    name: str
    geos: list                    # one ScanGeometry per robot, in batch order
    offsets: list                 # (x, y, yaw) of every robot's start relative to the grid's centre
    moves: list                   # [round][robot]: 1 = the robot moves one step before this round's scan, 0 = it stands still
    armed: bool = False           # registration_mode 3: every robot's pre-registration armed every round

    @property
    def n(self):
        return len(self.geos)

    @property
    def rounds(self):
        return len(self.moves)

    def poses(self, gc):
        """per robot the ground-truth poses of its scans: [rounds + 1][x, y, yaw], scan 0 at the start"""
        out = []
        for i, off in enumerate(self.offsets):
            cum = np.concatenate([[0], np.cumsum([m[i] for m in self.moves])])
            out.append(np.stack([0.5 * gc.width + off[0] + STEP_X * cum, 0.5 * gc.width + off[1] + 0.0 * cum, off[2] + STEP_YAW * cum], axis=1))
        return out


def _all_move(n, rounds):
    return [[1] * n for _ in range(rounds)]


OFFSETS = [(0.37, -0.21, 0.1), (-0.7, 0.4, 0.0), (0.9, 0.8, -0.2), (-0.3, -0.9, 0.3)]
# rounds 2-3: robot 0 stands still while the others move; round 4: everybody stands still; round 5: everybody moves
GATED_MOVES = [[1, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 0], [1, 1, 1]]
# mixed_five: the tile with the wall y = 6.8 m in it, T = (8, 4) (x 12.8-14.4 m, y 6.4-8.0 m), is updated by everybody; robot 3 (1081
# beams) stands on it, robots 1 and 2 (360) stand next to it, robots 0 (1081) and 4 (270) look at it from 5 m
FIVE_OFFSETS = [(0.5, -0.5, -1.5), (-1.2, -3.8, 0.2), (2.7, -3.8, -0.3), (0.6, -5.1, 1.4), (-2.6, -1.6, -0.9)]
POOL_TILE = (8, 4)
POOL_ROBOT = 3


def _lattice(n):
    """n distinct starts on a 5-wide lattice of 1.2 m around the centre (17: four rows), each row and column a little off the last"""
    return [(-2.4 + 1.2 * (i % 5) + 0.07 * (i // 5), -1.8 + 1.2 * (i // 5) + 0.05 * (i % 5), 0.1 * ((i % 7) - 3)) for i in range(n)]


SCENARIOS = {s.name: s for s in [
    Scenario("mixed_two_360_first", [GEO360, GEO1081], OFFSETS[:2], _all_move(2, 4)),
    Scenario("mixed_two_1081_first", [GEO1081, GEO360], OFFSETS[:2], _all_move(2, 4)),
    Scenario("mixed_three_fov", [GEO360, GEO270, GEO1081], OFFSETS[:3], _all_move(3, 4)),
    Scenario("mixed_five", [GEO1081, GEO360, GEO360, GEO1081, GEO270], FIVE_OFFSETS, _all_move(5, 3)),
    Scenario("robot0_gated_one_scanner", [GEO360] * 3, OFFSETS[:3], GATED_MOVES),
    Scenario("robot0_gated_mixed", [GEO1081, GEO360, GEO360], OFFSETS[:3], GATED_MOVES),
    Scenario("n16", [GEO360] * 16, _lattice(16), _all_move(16, 3)),
    Scenario("n17", [GEO360] * 17, _lattice(17), _all_move(17, 3)),
    Scenario("mixed_mode3", [GEO360, GEO1081], OFFSETS[:2], _all_move(2, 3), armed=True),
]}


# ---- what one robot's push did to the grid, from the oracle's dumps around it ---------------------------------------------------------
def push_effect(before, after):
    """Tiles that one push changed, by kind.  `updated`: the tile holds data afterwards and cells of it (or its state) changed by an
    update of its cells (TsdGrid.cpp:237-274); `emptied`: a tile that was materialised BEFORE the push and went through
    TsdGridPartition::increaseEmptiness (TsdGridPartition.cpp:136-164) -- every one of its cells, halo included, got exactly one more
    unit of weight (capped), which no update does (an update adds 0.01 * the partition's weight to the cells it touches);
    `changed`: any difference, the _initWeight of a tile without data included."""
    bi, biw, bt, bw = before
    ai, aiw, at, aw = after
    same_t = (bt == at) | (np.isnan(bt) & np.isnan(at))
    cells = ((bw != aw) | ~same_t).any(axis=1)
    changed = cells | (bi != ai) | (biw != aiw)
    plus_one = np.where(np.isnan(bt), bw + 1.0, np.minimum(bw + 1.0, MAX_WEIGHT))
    emptied = (bi == 1) & cells & (aw == plus_one).all(axis=1)
    updated = (ai == 1) & (cells | (bi == 0)) & ~emptied
    f = lambda m: set(int(p) for p in np.nonzero(m)[0])
    return dict(updated=f(updated), emptied=f(emptied), changed=f(changed))


def tile_geometry(gc, p):
    """centroid and radius of tile p as the push sees it (csrc/push_device.hpp tile_geometry), and its four corner points"""
    PX = gc.cells // TILE_DIM
    x, y = (p % PX) * TILE_DIM, (p // PX) * TILE_DIM
    e = [((x + dx + 0.5) * gc.cell_size, (y + dy + 0.5) * gc.cell_size) for dy in (0, TILE_DIM) for dx in (0, TILE_DIM)]
    return (x + 16.5) * gc.cell_size, (y + 16.5) * gc.cell_size, math.hypot(TILE_DIM, TILE_DIM) * gc.cell_size * 0.5, e


def window_bounds(gc, geo, pose, p):
    """(least, most) beams of the scan window that robot `pose` stages for its update of tile p (tile_in_range's `win`, widened by one
    beam at either end and clamped by k_mp_update).  A sensor within three tile radii of the centroid: the whole scan, exactly.  A far
    one: the corners' beam indices; None where a corner lies outside the field of view or the tile straddles the scan's cut (the
    argument of the pool case does not use such a robot)."""
    cx, cy, rad, e = tile_geometry(gc, p)
    px, py, yaw = pose[0, 2], pose[1, 2], math.atan2(pose[1, 0], pose[0, 0])
    if math.hypot(px - cx, py - cy) <= 3.0 * rad:
        return geo.beams, geo.beams
    b = [(math.atan2(y - py, x - px) - yaw + math.pi) % (2.0 * math.pi) - math.pi for x, y in e]
    res = geo.angle_increment
    if max(b) - min(b) > math.pi or min(b) < geo.angle_min + 3 * res or max(b) > geo.angle_min + (geo.beams - 4) * res:
        return None
    span = (max(b) - min(b)) / res
    return int(math.floor(span)), int(math.ceil(span)) + 4


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def drive(oracle, scn, device=True, multi=True, effects=False, compare=None):
    """Run scenario `scn` round by round on the oracle's primitives and, with device=True, through ONE TsdBatch of scn.n scans on a
    device grid (multi=False: tsd_debug_set_push_multi(0), one push per robot).  compare(k, i, ro, sr) is called per round and robot
    (tests/test_gpu_batch.py's _compare) and returns the pose difference.  effects=True: og.dump() around every robot's push.
    Everything that owns device memory is closed here."""
    from ohm_tsd_slam_amd import capi
    import tests.test_gpu_batch as T

    gc = synth.CONFIGS[CFG][0]
    n, rounds = scn.n, scn.rounds
    gc, _geo, _kw, og, dg, robots, scans, sensors, params, gates = T._setup(oracle, CFG, n, rounds + 1, geos=scn.geos, offsets=scn.offsets,
                                                                             poses=scn.poses(gc), device=device)
    out = dict(gc=gc, ros=[], effects=[], push_poses=[], device=[], pre=[], worst=0.0, worst_rad=0.0)
    batch = None
    try:
        if scn.armed:
            for rb in robots:
                rb.kw.update(trials=40, size_control_set=120)
        if device:
            dg.set_push_multi(multi)
            dg.push_stats_total(reset=True)
            batch = capi.TsdBatch(dg, n)
            bounds = (dg.min_x, dg.max_x, dg.min_y, dg.max_y)
        else:
            bounds = (0.0, og.max_x, 0.0, og.max_x)         # TsdGrid's _minX/_maxX/_minY/_maxY (the device grid reports the same)
        rng = np.random.default_rng(4242)
        for k in range(1, rounds + 1):
            ing = [rb.ingest(sc[k]) for rb, sc in zip(robots, scans)]
            draws = [tuple(rng.integers(0, 2 ** 31 - 1, m) for m in (g.beams, rb.kw["size_control_set"], rb.kw["trials"])) if scn.armed else None
                     for rb, g in zip(robots, scn.geos)]
            ros = [rb.localise(og, d_, m_, bounds, dr) for rb, (d_, m_, _), dr in zip(robots, ing, draws)]
            eff, pp = [], []
            for rb in robots:
                before = og.dump() if effects else None
                pp.append(None if rb._push is None else rb._push[0].copy())
                rb.apply_push(og)
                eff.append(push_effect(before, og.dump()) if effects else None)
            out["ros"].append(ros); out["effects"].append(eff); out["push_poses"].append(pp)
            if not device:
                continue
            if scn.armed:
                for rb, s, (d_, m_, _), dr in zip(robots, sensors, ing, draws):
                    sc_, ms_, _n = oracle.scene_from_scan(rb.rays_local, d_, m_)
                    s.preregister(sc_, ms_, rb.kw["trials"], rb.kw["size_control_set"], rb.kw["zrand"], np.radians(rb.kw["ransac_phi_max"]),
                                  rb.kw["angle_increment"], *dr)
            batch.begin(sensors, [x[0] for x in ing], [x[1] for x in ing], [x[2] for x in ing], params, gates)
            res = batch.results()
            for i, (ro, sr) in enumerate(zip(ros, res)):
                if compare is not None:
                    compare(k, i, ro, sr)
                d, a = H.pose_delta(ro["pose"], np.array(sr.pose[:]).reshape(3, 3))
                out["worst"], out["worst_rad"] = max(out["worst"], d), max(out["worst_rad"], a)
                if scn.armed and not ro["no_model"]:
                    pr = sensors[i].preregistration_result()
                    assert (pr["candidates"], pr["idx"], pr["i"]) == ro["pre"], f"round {k} robot {i}: pre-registration {pr} vs {ro['pre']}"
            out["device"].append([(np.array(sr.pose[:]).tobytes(), int(sr.pushed), int(sr.reg_error), int(sr.no_model), int(sr.icp.n_model),
                                   int(sr.icp.pairs), int(sr.icp.iterations), int(sr.icp.state)) for sr in res])
        out["oracle_grid"] = og.dump()
        if device:
            out["tiles"] = dg.download_tiles()
            out["stats"] = dg.push_stats_total()
            out["digest"] = dg.digest()
    finally:
        if batch is not None:
            batch.close()
        for s in sensors:
            s.close()
        if dg is not None:
            dg.close()
    return out
