"""The node parameters the suite sweeps beside the defaults: truncation radius, max_range, min_range and low_reflectivity_range
(the yaml's `truncation_radius`, `max_range`, `min_range`, `low_reflectivity_range`).  One table of named points, two small shapes and
one way to make the scans, shared by tests/test_cpu_params.py (the oracle against the numpy restatements) and tests/test_gpu_params.py
(the kernels against the oracle).  A plain module: nothing here is a fixture.

The counts next to the table are what the ORACLE ALONE produces on the CPU for each point and shape (`oracle_counts`): every point must
meet the minimum counts there before the GPU half uses it (tests/test_cpu_params.py: test_points_are_not_vacuous), and the GPU half
asserts the same minimums on what it computed.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from ohm_tsd_slam_amd import synth
from tests import helpers as H

Point = namedtuple("Point", "trunc max_range min_range low_refl")

# name -> (truncation REQUEST in cells, max_range, min_range, low_refl)
POINTS = {
    "default":        Point(3,    30.0, 0.001, 2.0),    # today's point, the control
    "trunc_min":      Point(2,    30.0, 0.001, 2.0),    # the band is narrower than a negmask group of 4 cells
    "trunc_clamped":  Point(1,    30.0, 0.001, 2.0),    # below the minimum: the grid reports 2 cells and equals trunc_min's bit for bit
    "trunc_odd":      Point(4.37, 30.0, 0.001, 2.0),    # max_trunc is not a multiple of the cell size
    "trunc_wide":     Point(12,   30.0, 0.001, 2.0),    # over a third of a tile: more candidates per tile
    "trunc_tile":     Point(40,   30.0, 0.001, 2.0),    # wider than a 32-cell tile: `closest` is negative for every near tile
    "short_sensor":   Point(3,    7.0,  2.5,   2.0),    # both range culls act, steep partition weight, the ray cast clamps at both ends
    "lowrefl_zero":   Point(3,    30.0, 0.001, 0.0),    # low2 = 0: no infinite reading updates anything
    "lowrefl_beyond": Point(5,    7.0,  0.3,   9.0),    # low_refl > max_range with a non-default band
}

# shape -> (map_size_log2, cell_size, scene, scanner): near and far tiles, several tiles per workgroup, the +-pi cut in the scanner's view
SHAPES = {
    "room8":    (8, 0.1,  "room",    synth.ScanGeometry.full_circle_360),
    "pillars9": (9, 0.05, "pillars", synth.ScanGeometry.utm30lx),
}

N_PUSHES = 5                        # H.sensor_pose(world, 0..4); a freeFootprint follows the third
FOOTPRINT = (0.28, 1.0, 1.0)        # x offset from the sensor, width, height (the node's footprint)
RAYCAST_K = 5                       # the ray cast's pose: H.sensor_pose(world, 5)

# Where the sensor starts: the scene's own start (grid centre + (0.37, -0.21)) unless the point cannot meet its counts there.
#   room, 7 m sensor: the walls are 5.8 .. 8.4 m from the centre -- two of them out of range, most beams without a hit, and no tile of
#     3.2 m that every reading clears.  The sensor starts near the centre of tile (2, 3), 3.1 m from the left wall and 3.6 m from the
#     lower one: beyond min_range = 2.5 m, inside max_range for 57 % of the circle, and its own tile is emptied by the clean scans.
#   pillars, the three points that must show an emptied tile: from the scene's own start the oracle empties none (a pillar stands in
#     every tile's sector) and a 7 m sensor hits on 42 % of its beams; from (13.17, 7.59) it empties 2 to 3 and hits on 57 % and more.
#     (World places its pillars away from the start it is given, so this is another pillar field as well.)
STARTS = {
    ("room8", "short_sensor"): (7.9, 10.4), ("room8", "lowrefl_beyond"): (7.9, 10.4),
    ("pillars9", "short_sensor"): (13.17, 7.59), ("pillars9", "lowrefl_beyond"): (13.17, 7.59), ("pillars9", "lowrefl_zero"): (13.17, 7.59),
}


def start_of(shape, point):
    st = STARTS.get((shape, point))
    return None if st is None else list(st)


# Minimum counts every (point, shape) must reach on the oracle.  "Well over a thousand cells": 2 000 in the best push.  "A clear
# majority of beams": 55 %.  Emptied / culled tiles over the five pushes, where the point is about them.
MIN_CELLS_BEST_PUSH = 2000
MIN_HIT_SHARE = 0.55
NEEDS_EMPTIED_AND_CULLED = ("short_sensor", "lowrefl_zero", "lowrefl_beyond")
# "culled": by RANGE (tiles_total - tiles_range_pass) at the points whose max_range a 25.6 m grid exceeds (short_sensor,
# lowrefl_beyond).  At lowrefl_zero max_range is 30 m and no tile of these grids is further away than 19 m: there the cull that can act is
# the classifier's own (range passed, then neither updated nor emptied: not visible, or behind every reading).
CULLED_BY_RANGE = ("short_sensor", "lowrefl_beyond")

# What the oracle produced, per point and shape: (cells updated by the best of the five pushes, tiles emptied over the five pushes,
# tiles culled over the five pushes, beams hit by the ray cast from pose 5).  tests/test_cpu_params.py holds the oracle to these
# figures and to the minimums above; the GPU half's statistics must equal the oracle's, so it reaches them too.
#                    room8: 64 tiles, 360 beams  pillars9: 256 tiles, 1081 beams
ORACLE_COUNTS = {
    "default":        ((19448, 14,  93, 360), (33017,  0, 581, 865)),
    "trunc_min":      ((18970, 14,  99, 345), (32545,  0, 583, 647)),
    "trunc_clamped":  ((18970, 14,  99, 345), (32545,  0, 583, 647)),
    "trunc_odd":      ((20017, 14,  87, 360), (33707,  0, 581, 906)),
    "trunc_wide":     ((23914,  6,  73, 360), (37470,  0, 569, 938)),
    "trunc_tile":     ((43576,  0,   0, 360), (52324,  0, 529, 981)),
    "short_sensor":   (( 3951,  2, 189, 206), (15879,  2, 871, 614)),
    "lowrefl_zero":   ((19426, 14,  93, 360), (32201,  2, 600, 878)),
    "lowrefl_beyond": ((11299, 20, 177, 209), (32273,  3, 858, 745)),
}


def grid_config(shape, point):
    log2, cs, _, _ = SHAPES[shape]
    return synth.GridConfig(log2, cs, POINTS[point].trunc)


def geometry(shape):
    return SHAPES[shape][3]()


def world_of(shape, point):
    log2, cs, scene, _ = SHAPES[shape]
    return synth.World(scene, synth.GridConfig(log2, cs), start_xy=start_of(shape, point))


def spoil(rng, r32):
    """tools/fuzz_parity.py's spoil -- zero / NaN / over-range / tiny readings at random beams, sometimes a dropped sector -- plus
    readings that arrive infinite; at least one of each kind (Sensor.cpp:246-272 treats each differently)"""
    r = r32.copy()
    n = len(r)
    for val in (0.0, np.nan, 45.0, 0.0005, np.inf):
        k = rng.integers(1, max(2, n // 40))
        r[rng.integers(0, n, k)] = val
    if n > 40 and rng.random() < 0.3:
        a = rng.integers(0, n - 20); r[a:a + rng.integers(3, 20)] = 0.0
    return r.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scans(shape, point, n=N_PUSHES + 1):
    """[(pose 3x3, (x, y, yaw), spoiled float32 ranges)] along H.sensor_pose(world, 0 .. n-1); the same readings at every point that
    shares the start (the ingest, which knows max_range, is the caller's)"""
    world, geo = world_of(shape, point), geometry(shape)
    rng = np.random.default_rng(977 + sorted(SHAPES).index(shape))
    out = []
    for k in range(n):
        pose, (x, y, yaw) = H.sensor_pose(world, k)
        r32 = world.scan(x, y, yaw, geo)
        out.append((pose, (x, y, yaw), spoil(rng, r32) if k % 2 == 0 else r32))
    return out


def outside_pose(shape):
    """a sensor outside the grid that looks into it"""
    log2, cs, _, _ = SHAPES[shape]
    W = (1 << log2) * cs
    return synth.pose_matrix(-0.7, 0.45 * W, 0.12)


def behind_wall_pose(shape, point):
    """a sensor BEHIND a surface the pushes saw, looking out of the scene: the model point the oracle's ray cast from pose 5 finds on
    its middle beam (the nearest beam that hits), moved on along that beam by 0.4 of the band (3 cells at the most) into the negative
    band, heading further out.  Its beams start at negative values: those that turn back into the scene meet the miss event
    (prev < 0 < cur) at the surface, the others run into unseen space."""
    g, _, (co, _, mo, _), _ = oracle_case(shape, point)
    gc, geo = grid_config(shape, point), geometry(shape)
    pose = scans(shape, point)[RAYCAST_K][0]
    b = min(np.nonzero(mo)[0], key=lambda i: abs(int(i) - geo.beams // 2))
    hit = pose @ np.array([co[2 * b], co[2 * b + 1], 1.0])
    dx, dy = hit[0] - pose[0, 2], hit[1] - pose[1, 2]
    n = math.hypot(dx, dy)
    depth = min(0.4 * max(gc.max_trunc, 2 * gc.cell_size), 3 * gc.cell_size)
    return synth.pose_matrix(hit[0] + depth * dx / n, hit[1] + depth * dy / n, math.atan2(dy, dx) + 0.07)


def push_all(oracle, grid, shape, point, n=N_PUSHES, footprint_after=2, on_push=None):
    """the pushes of a case on one backend's grid (oracle.Grid or capi.TsdGridDevice): -> [stats]"""
    P, geo = POINTS[point], geometry(shape)
    stats = []
    for k, (pose, (x, y, yaw), r32) in enumerate(scans(shape, point)[:n]):
        data, mask = oracle.ingest_f32(r32, P.max_range, geo.angle_increment)
        stats.append(grid.push(pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl))
        if on_push is not None:
            on_push(k, stats[-1])
        if k == footprint_after:
            assert grid.free_footprint([x + FOOTPRINT[0], y], FOOTPRINT[1], FOOTPRINT[2])
    return stats


def raycast_rays(oracle, shape, point, pose):
    gc, geo = grid_config(shape, point), geometry(shape)
    return H.world_rays(oracle, geo, pose, gc.cell_size)[1]


def counts_of(point, stats, hits, beams):
    """the non-vacuity figures of a case from its push statistics and its ray cast's hit count"""
    emptied = sum(s["tiles_emptied_init"] + s["tiles_emptied_uninit"] for s in stats)
    if point in CULLED_BY_RANGE:
        culled = sum(s["tiles_total"] - s["tiles_range_pass"] for s in stats)
    else:
        culled = sum(s["tiles_range_pass"] - s["tiles_update"] - s["tiles_emptied_init"] - s["tiles_emptied_uninit"] for s in stats)
    return dict(cells=max(s["cells_updated"] for s in stats), emptied=emptied, culled=culled, hits=int(hits), beams=int(beams))


def assert_not_vacuous(point, c):
    assert c["cells"] >= MIN_CELLS_BEST_PUSH, f"{point}: the best push updates {c['cells']} cells"
    assert c["hits"] >= MIN_HIT_SHARE * c["beams"], f"{point}: {c['hits']} of {c['beams']} beams hit"
    if point in NEEDS_EMPTIED_AND_CULLED:
        assert c["emptied"] >= 1 and c["culled"] >= 1, f"{point}: {c['emptied']} tiles emptied, {c['culled']} culled"


@functools.lru_cache(maxsize=None)
def oracle_case(shape, point):
    """the oracle's run of a case, once per process: (grid after the pushes, [stats], ray cast from pose 5, counts)"""
    from oracle import pyoracle as O
    gc, geo, P = grid_config(shape, point), geometry(shape), POINTS[point]
    g = O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    stats = push_all(O, g, shape, point)
    pose = scans(shape, point)[RAYCAST_K][0]
    rc = g.raycast(pose, raycast_rays(O, shape, point, pose), P.min_range, P.max_range)
    return g, stats, rc, counts_of(point, stats, rc[3], geo.beams)
