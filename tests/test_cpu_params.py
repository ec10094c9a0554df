"""The oracle away from the default node parameters (tests/param_points.py): at every point of the table the oracle's push, tile
classification and ray cast against numpy / pure-Python restatements written from the reference's text.  The oracle's push and ray
cast cannot be pinned to the compiled reference (those units need GSL and FLANN); these restatements are what pins them, and until
now they ran at the default truncation radius, max_range, min_range and low_reflectivity_range only.

  cells  numpy_push_from_empty (test_cpu_oracle_properties.py): every cell of one push into an empty grid, 1e-12 / 1e-15
  tiles  np_tile_decisions (below): TsdGridComponent::isInRange per tile -- range cull, four-corner visibility, update / empty /
         skip -- against the tiles the oracle initialised, the _initWeight it left and its push statistics
  rays   _np_raycast_beam with the normal look-ups: hit or miss per beam exact, coordinates and normals 1e-12
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from ohm_tsd_slam_amd import synth
from oracle import pyoracle as O
from tests import helpers as H
from tests import param_points as PP
from tests.test_cpu_oracle_properties import _np_bilinear, _np_raycast_beam, numpy_push_from_empty

CASES = [(s, p) for s in PP.SHAPES for p in PP.POINTS]
SKIP_RANGE, SKIP_UNSEEN, EMPTIED, UPDATE = 0, 1, 2, 3
EDGE = 1e-9            # a decision this close (metres) to one of its thresholds may be left out ...
EDGE_SHARE = 0.01      # ... for at most this share of the tiles in range


def np_tile_decisions(gc, geo, pose, data, mask, max_range, min_range, low_refl):
    """TsdGridComponent::isInRange (TsdGridComponent.cpp:43-124) for every 32 x 32 partition of the grid, with the partition's
    geometry of TsdGridPartition.cpp:48-70 and the corner look-up of SensorPolar2D::backProject (:117-135): -> (decision[tiles],
    on_edge[tiles]); on_edge: a comparison of the decision against a range lies within EDGE of equality."""
    cs, PX = gc.cell_size, gc.cells // 32
    maxT = max(gc.max_trunc, 2 * cs)                       # TsdGrid::setMaxTruncation (TsdGrid.cpp:206-215)
    Pi = np.linalg.inv(pose)
    lower = -0.5 * geo.angle_increment + geo.angle_min     # SensorPolar2D.cpp:26-30
    upper = geo.angle_min + (geo.beams - 0.5) * geo.angle_increment
    finite = ~np.isinf(data)
    decision = np.zeros(PX * PX, dtype=np.int64)
    on_edge = np.zeros(PX * PX, dtype=bool)
    for p in range(PX * PX):
        x, y = (p % PX) * 32, (p // PX) * 32
        ex = np.array([x + 0.5, x + 32 + 0.5, x + 0.5, x + 32 + 0.5]) * cs
        ey = np.array([y + 0.5, y + 0.5, y + 32 + 0.5, y + 32 + 0.5]) * cs
        cen = (ex.sum() / 4.0, ey.sum() / 4.0)
        rad = math.sqrt((ex[3] - ex[0]) ** 2 + (ey[3] - ey[0]) ** 2) * 0.5
        distance = math.sqrt((pose[0, 2] - cen[0]) ** 2 + (pose[1, 2] - cen[1]) ** 2)
        closest = distance - rad - maxT
        farthest = distance + rad + maxT
        on_edge[p] = abs(closest - max_range) < EDGE or abs(farthest - min_range) < EDGE
        if closest > max_range or farthest < min_range:
            decision[p] = SKIP_RANGE
            continue
        phi = np.arctan2(Pi[1, 0] * ex + Pi[1, 1] * ey + Pi[1, 2], Pi[0, 0] * ex + Pi[0, 1] * ey + Pi[0, 2])
        below, above = phi <= lower, phi >= upper
        v = (phi - geo.angle_min) * (1.0 / geo.angle_increment)
        idx = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(int)                  # C's round(): halves away from zero
        idx = np.where(below, 0, np.where(above, geo.beams - 1, idx))
        if (below | above).all():
            decision[p] = SKIP_UNSEEN
            continue
        lo, hi = idx.min(), idx.max()
        d, m, f = data[lo:hi + 1], mask[lo:hi + 1].astype(bool), finite[lo:hi + 1]
        on_edge[p] |= bool((np.abs(d[f] - closest) < EDGE).any())
        if not ((d > closest) & m).any():
            decision[p] = SKIP_UNSEEN
            continue
        decision[p] = UPDATE
        if not (below | above).any():
            on_edge[p] |= bool((np.abs(d[f] - farthest) < EDGE).any()) or ((~f).any() and abs(distance - low_refl) < EDGE)
            ok_inf = distance < low_refl
            if np.where(f, (d > farthest) & m, ok_inf).all():
                decision[p] = EMPTIED
    return decision, on_edge


def _ingest(shape, point, k):
    P, geo = PP.POINTS[point], PP.geometry(shape)
    pose, _, r32 = PP.scans(shape, point)[k]
    data, mask = O.ingest_f32(r32, P.max_range, geo.angle_increment)
    return pose, data, mask


def test_table_holds_the_points_of_the_sweep():
    want = {"default": (3, 30, 0.001, 2.0), "trunc_min": (2, 30, 0.001, 2.0), "trunc_clamped": (1, 30, 0.001, 2.0),
            "trunc_odd": (4.37, 30, 0.001, 2.0), "trunc_wide": (12, 30, 0.001, 2.0), "trunc_tile": (40, 30, 0.001, 2.0),
            "short_sensor": (3, 7, 2.5, 2.0), "lowrefl_zero": (3, 30, 0.001, 0.0), "lowrefl_beyond": (5, 7, 0.3, 9.0)}
    for name, v in want.items():
        assert tuple(PP.POINTS[name]) == v
    assert tuple(PP.POINTS["default"]) == (synth.GridConfig(8, 0.1).truncation_radius, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
    assert [PP.SHAPES[s][:3] for s in ("room8", "pillars9")] == [(8, 0.1, "room"), (9, 0.05, "pillars")]
    # the spoiled scans carry every kind of reading the ingest treats differently
    for shape in PP.SHAPES:
        r = PP.scans(shape, "default")[0][2]
        assert np.isinf(r).any() and np.isnan(r).any() and (r == 0.0).any() and (r > 30.0).any() and (r == np.float32(0.0005)).any()


@pytest.mark.parametrize("shape,point", CASES)
def test_points_are_not_vacuous(shape, point):
    """the minimum counts of param_points on what the oracle alone produces, and the figures written next to the table"""
    g, stats, rc, c = PP.oracle_case(shape, point)
    print(f"{shape:9s} {point:15s} cells {c['cells']:6d}  emptied {c['emptied']:3d}  culled {c['culled']:4d}  hits {c['hits']:4d} / {c['beams']}")
    PP.assert_not_vacuous(point, c)
    assert (c["cells"], c["emptied"], c["culled"], c["hits"]) == PP.ORACLE_COUNTS[point][list(PP.SHAPES).index(shape)]
    cs = PP.SHAPES[shape][1]
    assert g.max_trunc == max(PP.POINTS[point].trunc, 2) * cs                 # the clamp of setMaxTruncation
    if point == "short_sensor":
        assert any(s["tiles_range_pass"] < s["tiles_total"] for s in stats)
    if point in ("trunc_min", "trunc_tile"):
        pose = PP.behind_wall_pose(shape, point)              # the extra ray cast of these points starts inside the negative band
        st, v = g.bilinear(pose[0, 2], pose[1, 2])
        assert st == 0 and v < 0


@pytest.mark.parametrize("shape", list(PP.SHAPES))
def test_clamped_request_gives_the_minimum_grid(shape):
    """a truncation request below 2 cells: the grid reports 2 cells and equals trunc_min's bit for bit"""
    a, b = PP.oracle_case(shape, "trunc_clamped"), PP.oracle_case(shape, "trunc_min")
    assert a[0].max_trunc == b[0].max_trunc == 2 * PP.SHAPES[shape][1] and a[1] == b[1]
    for x, y in zip(a[0].dump(), b[0].dump()):
        assert np.array_equal(x, y, equal_nan=True)
    g = O.Grid(PP.SHAPES[shape][0], PP.SHAPES[shape][1], 3 * PP.SHAPES[shape][1])
    assert g.set_max_truncation(0.5 * PP.SHAPES[shape][1]) == 2 * PP.SHAPES[shape][1] == g.max_trunc
    assert g.set_max_truncation(6 * PP.SHAPES[shape][1]) == 6 * PP.SHAPES[shape][1]


@pytest.mark.parametrize("shape,point", CASES)
def test_push_cells_against_numpy_rederivation(shape, point):
    """one push into an empty grid, every cell of every initialised tile: the spoiled scan 0 and the clean scan 1"""
    gc, geo, P = PP.grid_config(shape, point), PP.geometry(shape), PP.POINTS[point]
    PX = gc.cells // 32
    for k in (0, 1):
        pose, data, mask = _ingest(shape, point, k)
        g = O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
        st = g.push(pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
        init, iw, tsd, w = g.dump()
        e_tsd, e_w, e_upd = numpy_push_from_empty(gc, geo, pose, data, mask, P.max_range, P.low_refl)
        n_upd = 0
        for p in np.nonzero(init)[0]:
            py, px = divmod(p, PX)
            t = tsd[p].reshape(33, 33)[:32, :32]
            ww = w[p].reshape(33, 33)[:32, :32]
            et = e_tsd[py * 32:(py + 1) * 32, px * 32:(px + 1) * 32]
            ew = e_w[py * 32:(py + 1) * 32, px * 32:(px + 1) * 32]
            assert np.array_equal(np.isnan(t), np.isnan(et)), f"scan {k} tile {p}"
            m = ~np.isnan(t)
            assert np.allclose(t[m], et[m], rtol=0, atol=1e-12)
            assert np.allclose(ww, ew, rtol=0, atol=1e-15)
            n_upd += int(m.sum())
        assert n_upd == st["cells_updated"] > 1000
        if P.low_refl == 0.0:
            # no infinite reading updates anything: every updated cell lies on a finite beam
            assert not np.isinf(_beam_reading(gc, geo, pose, data)[e_upd]).any()
        # the band's cells of every finite reading lie in initialised tiles: the classifier cut off no surface
        near = e_upd & (np.abs(e_tsd) < 1.0)
        tiles_of_near = np.unique((np.nonzero(near)[0] // 32) * PX + np.nonzero(near)[1] // 32)
        assert init[tiles_of_near].all()


def _beam_reading(gc, geo, pose, data):
    """the reading of the beam every cell centre projects onto (as numpy_push_from_empty names it)"""
    N, cs = gc.cells, gc.cell_size
    Pi = np.linalg.inv(pose)
    c = (np.arange(N) + 0.5) * cs
    cx, cy = np.meshgrid(c, c)
    phi = np.arctan2(Pi[1, 0] * cx + Pi[1, 1] * cy + Pi[1, 2], Pi[0, 0] * cx + Pi[0, 1] * cy + Pi[0, 2])
    return data[np.clip(np.round((phi - geo.angle_min) / geo.angle_increment).astype(int), 0, geo.beams - 1)]


@pytest.mark.parametrize("shape,point", CASES)
def test_tile_decisions_against_numpy_restatement(shape, point):
    """which tiles the oracle initialised, which carry _initWeight and its push statistics after ONE push into an empty grid,
    against np_tile_decisions; scan 0 (spoiled) and scan 1 (clean: the one that empties tiles)"""
    gc, geo, P = PP.grid_config(shape, point), PP.geometry(shape), PP.POINTS[point]
    seen = set()
    for k in (0, 1):
        pose, data, mask = _ingest(shape, point, k)
        g = O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
        st = g.push(pose, data, mask, geo.angle_increment, geo.angle_min, P.max_range, P.min_range, P.low_refl)
        init, iw = g.tile_state()
        dec, edge = np_tile_decisions(gc, geo, pose, data, mask, P.max_range, P.min_range, P.low_refl)
        in_range = int((dec != SKIP_RANGE).sum())
        assert edge.sum() <= EDGE_SHARE * in_range, f"{int(edge.sum())} of {in_range} tiles sit on a threshold"
        keep = ~edge
        assert np.array_equal(init[keep].astype(bool), dec[keep] == UPDATE), f"scan {k}: initialised tiles differ at {np.nonzero(keep & (init.astype(bool) != (dec == UPDATE)))[0][:8]}"
        assert np.array_equal(iw[keep], np.where(dec[keep] == EMPTIED, 1.0, 0.0)), f"scan {k}: _initWeight differs"
        if not edge.any():
            n_upd, n_emp = int((dec == UPDATE).sum()), int((dec == EMPTIED).sum())
            assert st == dict(st, tiles_total=len(dec), tiles_range_pass=in_range, tiles_update=n_upd, tiles_new=n_upd,
                              tiles_new_from_empty=0, tiles_emptied_init=0, tiles_emptied_uninit=n_emp, cells_visited=1024 * n_upd)
        seen |= set(dec.tolist())
    assert UPDATE in seen
    if (shape, point) != ("room8", "trunc_tile"):       # (a 4 m band on 3.2 m tiles: every tile of the room's grid is updated)
        assert SKIP_UNSEEN in seen
    if point in PP.NEEDS_EMPTIED_AND_CULLED:
        assert EMPTIED in seen
    if point in PP.CULLED_BY_RANGE:
        assert SKIP_RANGE in seen


@pytest.mark.parametrize("shape,point", CASES)
def test_raycast_against_python_rederivation(shape, point):
    """the ray march with its normal look-ups after three pushes, from pose 5 and from outside the grid with the point's min_range and
    max_range, every beam; at trunc_min and trunc_tile also from behind a wall, inside the negative band"""
    gc, geo, P = PP.grid_config(shape, point), PP.geometry(shape), PP.POINTS[point]
    g = O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    PP.push_all(O, g, shape, point, n=3, footprint_after=-1)
    dump = g.dump()
    gcc = synth.GridConfig(gc.map_size_log2, gc.cell_size)
    cs = gc.cell_size
    poses = [PP.scans(shape, point)[PP.RAYCAST_K][0], PP.outside_pose(shape)]
    if point in ("trunc_min", "trunc_tile"):
        poses.append(PP.behind_wall_pose(shape, point))
    for n_pose, pose in enumerate(poses):
        rw = PP.raycast_rays(O, shape, point, pose)
        co, no, mo, cnt = g.raycast(pose, rw, P.min_range, P.max_range)
        Pi = np.linalg.inv(pose)
        hits = 0
        beams = range(geo.beams)
        for b in beams:
            hit, cx, cy = _np_raycast_beam(gcc, dump, (pose[0, 2], pose[1, 2]), (rw[b], rw[geo.beams + b]), P.min_range, P.max_range)
            if hit:
                vals = [_np_bilinear(gcc, dump, cx + dx, cy + dy) for dx, dy in ((cs, 0), (-cs, 0), (0, cs), (0, -cs))]
                if any(s_ != 0 for s_, _ in vals):
                    hit = False
                else:
                    n = np.array([vals[0][1] - vals[1][1], vals[2][1] - vals[3][1]])
                    ln = math.sqrt(n[0] * n[0] + n[1] * n[1])
                    if abs(ln) > 10e-6:
                        n = n / ln
            assert bool(mo[b]) == hit, f"pose {n_pose} beam {b}"
            if hit:
                hits += 1
                m = Pi @ np.array([cx, cy, 1.0])
                nn = Pi[:2, :2] @ n
                assert abs(m[0] - co[2 * b]) <= 1e-12 and abs(m[1] - co[2 * b + 1]) <= 1e-12, f"pose {n_pose} beam {b}"
                assert abs(nn[0] - no[2 * b]) <= 1e-12 and abs(nn[1] - no[2 * b + 1]) <= 1e-12, f"pose {n_pose} beam {b}"
        assert hits == int(mo[list(beams)].sum())
        if n_pose == 0:
            assert cnt >= PP.MIN_HIT_SHARE * geo.beams, f"{cnt} of {geo.beams} beams hit"
            if P.min_range > 1.0 or P.max_range < 10.0:
                # the clamps of the march act: no model point nearer than min_range or further than max_range (+ one step)
                rng_model = np.hypot(co[0::2], co[1::2])[mo.astype(bool)]
                assert rng_model.min() >= P.min_range - cs and rng_model.max() <= P.max_range + cs


def test_oracle_against_rederivations_on_random_parameters():
    """tools/fuzz_oracle.py params: the re-derivations against the oracle on random grids, scanners, poses AND random truncation
    (1-40 cells, non-integers included), max_range (3-30), min_range (0.001-3) and low_refl (0-12); a short run"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_oracle.py"), "40", "9100", "params"], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "all 40 cases ok" in p.stdout
