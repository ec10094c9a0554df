"""Plain numpy restatement of the map-alignment rules of include/tsd_hip.h (tsd_align_points / tsd_map_align): the coarse score of a
pose candidate, one accumulation of the refinement, the Gauss-Newton step with its gain rule, the winner rule and the whole-cell shift
-- written from the header's text on a canonical tile dump, not from the kernels.  The look-ups are ``reloc_ref.GridView.bilinear``, the
peaks ``reloc_ref.peaks``.  Also the scenes the alignment tests share (``scene``), built once per process with the oracle.

Sums are numpy's (pairwise) sums: the device sums in another order, so a test compares them within the summation bound, never bit
for bit; ``accumulate`` returns the sum of the terms' magnitudes for that bound.
"""
import functools
import math

import numpy as np

from tests import reloc_ref as R
from tests import surface_ref as S

MAXITER, CONVERGED, DEGENERATE = 0, 1, 2
MAX_POINTS_COARSE = 2048             # TSD_MAX_ICP_POINTS
V_CUT, EPS = 0.75, 1e-6


def coarse_points(points_xy, pivot):
    """every stride-th point minus the pivot, stride = ceil(n / 2048) -> (points [P, 2], stride)"""
    pts = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2)
    stride = (len(pts) + MAX_POINTS_COARSE - 1) // MAX_POINTS_COARSE
    return pts[::stride] - np.asarray(pivot, dtype=np.float64)[None, :], stride


def scores(view, points_xy, pivot, x0, y0, step, nx, ny, cos_sin):
    """volume uint32 [ntheta, ny, nx]: tsd_relocalize's sum over the coarse points carried to every candidate, without the gate"""
    rel, _ = coarse_points(points_xy, pivot)
    px, py = rel[:, 0][None, :], rel[:, 1][None, :]
    tab = np.asarray(cos_sin, dtype=np.float64).reshape(-1, 2)
    tx = np.tile(x0 + np.arange(nx).astype(np.float64) * step, ny)[:, None]
    ty = np.repeat(y0 + np.arange(ny).astype(np.float64) * step, nx)[:, None]
    vol = np.zeros((tab.shape[0], ny * nx), dtype=np.uint32)
    for k in range(tab.shape[0]):
        c, s = tab[k, 0], tab[k, 1]
        wx = (c * px - s * py) + tx
        wy = (s * px + c * py) + ty
        st, v = view.bilinear(wx, wy)
        ok = st == R.SUCCESS
        term = np.zeros(v.shape, dtype=np.uint32)
        term[ok] = (np.uint32(R.ONE) - np.rint(np.abs(v[ok]) * 1048576.0).astype(np.uint32)).astype(np.uint32)
        vol[k] = term.sum(axis=1, dtype=np.uint32)
    return vol.reshape(tab.shape[0], ny, nx)


def normal(view, x, y):
    """TsdGrid::interpolateNormal on arrays -> (all four look-ups succeed, nx, ny, length before normalising)"""
    cs = view.cs
    look = [view.bilinear(x + cs, y), view.bilinear(x - cs, y), view.bilinear(x, y + cs), view.bilinear(x, y - cs)]
    ok = np.ones(np.shape(x), dtype=bool)
    for st, _ in look:
        ok &= st == R.SUCCESS
    with np.errstate(invalid="ignore", divide="ignore"):
        nx = look[0][1] - look[1][1]
        ny = look[2][1] - look[3][1]
        ln = np.sqrt(nx * nx + ny * ny)
        norm = ~(np.abs(ln) <= 10e-6)
        nx = np.where(norm, nx / ln, nx)
        ny = np.where(norm, ny / ln, ny)
    return ok, nx, ny, ln


def terms(view, rel, m, c, s, v_cut, max_trunc):
    """the 11 terms of every point (rel = points - pivot) at the state (m, c, s): (T [11, n], counted [n] bool)"""
    px, py = rel[:, 0], rel[:, 1]
    qx = (c * px - s * py) + m[0]
    qy = (s * px + c * py) + m[1]
    st, v = view.bilinear(qx, qy)
    okn, nx, ny, ln = normal(view, qx, qy)
    with np.errstate(invalid="ignore"):
        counted = (st == R.SUCCESS) & okn & (ln > 10e-6)
        u = v / v_cut
        live = counted & (np.abs(u) < 1.0)
        h = 1.0 - u * u
        w = h * h
        r = v * max_trunc
        jt = nx * (-(qy - m[1])) + ny * (qx - m[0])
        wjx, wjy, wjt = w * nx, w * ny, w * jt
        T = np.stack([wjx * nx, wjx * ny, wjx * jt, wjy * ny, wjy * jt, wjt * jt, -(wjx * r), -(wjy * r), -(wjt * r), w, (w * r) * r])
    T[:, ~live] = 0.0
    return T, counted


def accumulate(view, rel, m, c, s, v_cut, max_trunc):
    """-> (sums [11], n_ok, sum of |term| [11])"""
    T, counted = terms(view, rel, m, c, s, v_cut, max_trunc)
    return T.sum(axis=1), int(counted.sum()), np.abs(T).sum(axis=1)


def solve(S):
    """A d = b by LDL^T without pivoting, in the header's order -> (dx, dy, dth) or None when a pivot is not positive"""
    S = [float(v) for v in S]
    d0 = S[0]
    if not d0 > 0.0:
        return None
    l10, l20 = S[1] / d0, S[2] / d0
    d1 = S[3] - l10 * S[1]
    if not d1 > 0.0:
        return None
    t21 = S[4] - l20 * S[1]
    l21 = t21 / d1
    d2 = (S[5] - l20 * S[2]) - l21 * t21
    if not d2 > 0.0:
        return None
    y0 = S[6]
    y1 = S[7] - l10 * y0
    y2 = (S[8] - l20 * y0) - l21 * y1
    dt = y2 / d2
    dy = y1 / d1 - l21 * dt
    dx = (y0 / d0 - l10 * dy) - l20 * dt
    return dx, dy, dt


def refine(view, points_xy, pivot, m, c, s, iterations, max_trunc, lever, v_cut=V_CUT, eps=EPS, gain_rule=True):
    """the refinement of one peak from the state (m, c, s) -> dict(status, iterations, m, c, s, gain, sums, n_ok, steps); steps[i] =
    (hypot(dx, dy), lever * |dth|) of step i"""
    rel = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2) - np.asarray(pivot, dtype=np.float64)[None, :]
    m = [float(m[0]), float(m[1])]
    c, s = float(c), float(s)
    gain, prev, converged, it, steps = 1.0, (0.0, 0.0, 0.0), False, 0, []
    while True:
        sums, n_ok, _ = accumulate(view, rel, m, c, s, v_cut, max_trunc)
        if n_ok < 3:
            status = DEGENERATE
            break
        if converged:
            status = CONVERGED
            break
        if it >= iterations:
            status = MAXITER
            break
        d = solve(sums)
        if d is None:
            status = DEGENERATE
            break
        dot = (d[0] * prev[0] + d[1] * prev[1]) + (lever * lever) * (d[2] * prev[2])
        if gain_rule and dot < 0.0:
            gain = max(gain * 0.5, 0.0625)
        d = (d[0] * gain, d[1] * gain, d[2] * gain)
        prev = d
        h = math.hypot(1.0, d[2])
        rc, rs = 1.0 / h, d[2] / h
        c2, s2 = c * rc - s * rs, s * rc + c * rs
        hh = math.hypot(c2, s2)
        c, s = c2 / hh, s2 / hh
        m = [m[0] + d[0], m[1] + d[1]]
        steps.append((math.hypot(d[0], d[1]), lever * abs(d[2])))
        converged = steps[-1][0] < eps and steps[-1][1] < eps
        it += 1
    return dict(status=status, iterations=it, m=(m[0], m[1]), c=c, s=s, gain=gain, sums=sums, n_ok=n_ok, steps=steps)


def winner(records):
    """index of the record with the largest sum w whose status is not degenerate, the earlier one keeps a tie (-1: none)"""
    best = -1
    for j, r in enumerate(records):
        if r["status"] == DEGENERATE:
            continue
        if best < 0 or r["sums"][9] > records[best]["sums"][9]:
            best = j
    return best


def transform(rec, pivot):
    """T (3 x 3, points -> grid) of a refined state: rotation (c, s), translation m - R * pivot"""
    c, s, m = rec["c"], rec["s"], rec["m"]
    return np.array([[c, -s, m[0] - (c * pivot[0] - s * pivot[1])], [s, c, m[1] - (s * pivot[0] + c * pivot[1])], [0.0, 0.0, 1.0]])


def cell_shift(T, cs, src_cells):
    """(cell_off, cell_error): the whole-cell shift nearest to T -- src's cell (x, y) is dst's cell (x + ox, y + oy), tsd_fuse's
    convention -- and the largest distance in cells between T p and p + off * cs over the corners p of src's grid"""
    ox, oy = np.rint(T[0, 2] / cs), np.rint(T[1, 2] / cs)
    side = float(src_cells) * cs
    worst = 0.0
    for px, py in ((0.0, 0.0), (side, 0.0), (0.0, side), (side, side)):
        q = T @ np.array([px, py, 1.0])
        worst = max(worst, math.hypot(q[0] - (px + ox * cs), q[1] - (py + oy * cs)) / cs)
    return (int(ox), int(oy)), worst


def map_error(T, D, side):
    """(metres, radians) between two transforms: the largest |T p - D p| over the centre and the four corners of a grid of width
    `side` (what any point of the map is displaced by at most), and the angle between the rotations"""
    worst = 0.0
    for px, py in ((0.5 * side, 0.5 * side), (0.0, 0.0), (side, 0.0), (0.0, side), (side, side)):
        p = np.array([px, py, 1.0])
        worst = max(worst, float(np.linalg.norm((T @ p - D @ p)[:2])))
    a = math.atan2(T[1, 0], T[0, 0]) - math.atan2(D[1, 0], D[0, 0])
    return worst, abs(math.atan2(math.sin(a), math.cos(a)))


# ---- the scenes the tests share ---------------------------------------------------------------------------------------------------
STEP, NXY, NTHETA, DTHETA = R.STEP, R.NXY, R.NTHETA, R.DTHETA     # 24 x 24 x 36 at 0.1 m and 10 degrees
POSES = 18
K, ITERATIONS = 16, 64
D_ANGLE, D_SHIFT = math.radians(7.3), (0.43, -0.27)
CELLS_SHIFT = (16, -7)


class Scene:
    pass


def rigid_about(angle, centre, shift):
    """rotation by `angle` about `centre`, then the translation `shift`, 3 x 3"""
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, centre[0] - (c * centre[0] - s * centre[1]) + shift[0]],
                     [s, c, centre[1] - (s * centre[0] + c * centre[1]) + shift[1]], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def _world():
    from ohm_tsd_slam_amd import synth
    from oracle import pyoracle as O
    O.build()
    gc = synth.GridConfig(9, 0.05)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("pillars", gc)
    poses = synth.trajectory(world, POSES, step_x=0.25, step_yaw=0.01)
    scans = [O.ingest_f32(world.scan(p[0], p[1], p[2], geo), R.MAX_RANGE, geo.angle_increment) for p in poses]
    return gc, geo, world, poses, scans


@functools.lru_cache(maxsize=None)
def pushed_map(first, last, d_key):
    """the oracle grid of the scans first .. last - 1 pushed at D * pose (d_key: D's nine entries) -> (dump, view, surface xy)"""
    from ohm_tsd_slam_amd import synth
    from oracle import pyoracle as O
    gc, geo, world, poses, scans = _world()
    D = np.array(d_key).reshape(3, 3)
    grid = O.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for p, (data, mask) in list(zip(poses, scans))[first:last]:
        grid.push(D @ synth.pose_matrix(*p), data, mask, geo.angle_increment, geo.angle_min, R.MAX_RANGE, R.MIN_RANGE, R.LOW_REFL)
    dump = grid.dump()
    view = R.GridView(dump, grid.cells, gc.cell_size)
    xy, _ = S.points(gc.map_size_log2, gc.cell_size, np.asarray(dump[0]), np.asarray(dump[2]).reshape(len(dump[0]), -1))
    return dump, view, xy


@functools.lru_cache(maxsize=None)
def scene(name):
    """Map A = src: poses 0-11 at their true poses.  Map B = dst: the scans pushed at D * pose -- self: B = A, D = I; same: poses 0-11,
    D = 7.3 degrees about world.start plus (0.43, -0.27) m; diff: poses 6-17, same D; cells: poses 6-17, D = a translation by
    (16, -7) cells.  T = D carries A's coordinates into B's.  The lattice is 24 x 24 x 36 at 0.1 m / 10 degrees, the truth (where D
    carries the pivot, D's angle) 11.4 / 11.7 / 12.3 steps from its corner; the pivot is the centre of A's grid."""
    gc, geo, world, poses, scans = _world()
    cs = gc.cell_size
    sc = Scene()
    sc.name, sc.gc, sc.cs, sc.max_trunc, sc.cells = name, gc, cs, gc.max_trunc, gc.cells
    sc.geo, sc.world, sc.poses = geo, world, poses
    sc.side = gc.cells * cs
    ident = np.eye(3)
    if name == "self":
        sc.D, b_range = ident, (0, 12)
    elif name == "same":
        sc.D, b_range = rigid_about(D_ANGLE, world.start, D_SHIFT), (0, 12)
    elif name == "diff":
        sc.D, b_range = rigid_about(D_ANGLE, world.start, D_SHIFT), (6, 18)
    elif name == "cells":
        sc.D, b_range = rigid_about(0.0, world.start, (CELLS_SHIFT[0] * cs, CELLS_SHIFT[1] * cs)), (6, 18)
    else:
        raise KeyError(name)
    sc.dump_a, sc.view_a, sc.surface_a = pushed_map(0, 12, tuple(ident.reshape(-1)))
    sc.dump_b, sc.view_b, _ = pushed_map(b_range[0], b_range[1], tuple(sc.D.reshape(-1)))
    sc.points_raw = sc.surface_a                                   # the list as tsd_surface_* gives it
    sc.points = sc.surface_a + 0.5 * cs                            # ... and as tsd_map_align stages it
    sc.pivot = (0.5 * sc.side, 0.5 * sc.side)
    sc.lever = 0.5 * sc.side
    land = sc.D @ np.array([sc.pivot[0], sc.pivot[1], 1.0])
    sc.truth = (float(land[0]), float(land[1]), math.atan2(sc.D[1, 0], sc.D[0, 0]))
    sc.x0, sc.y0 = sc.truth[0] - 11.4 * STEP, sc.truth[1] - 11.7 * STEP
    sc.theta0 = sc.truth[2] - 12.3 * DTHETA
    sc.table = R.rotation_table(NTHETA, sc.theta0, DTHETA)
    sc.lattice = dict(x0=sc.x0, y0=sc.y0, step_xy=STEP, nx=NXY, ny=NXY, ntheta=NTHETA, cos_sin=sc.table, theta_wraps=True)
    return sc


@functools.lru_cache(maxsize=None)
def scene_scores(name):
    sc = scene(name)
    return scores(sc.view_b, sc.points, sc.pivot, sc.x0, sc.y0, STEP, NXY, NXY, sc.table)


def start_of(sc, idx):
    """(m, c, s) of lattice candidate idx"""
    k, rem = divmod(int(idx), NXY * NXY)
    iy, ix = divmod(rem, NXY)
    return (sc.x0 + float(ix) * STEP, sc.y0 + float(iy) * STEP), float(sc.table[k, 0]), float(sc.table[k, 1])


@functools.lru_cache(maxsize=None)
def scene_records(name, points="staged"):
    """the restatement's whole alignment of a scene: (peak idx, peak scores, refined records)"""
    sc = scene(name)
    pts = sc.points if points == "staged" else sc.points_raw
    vol = scene_scores(name) if points == "staged" else scores(sc.view_b, pts, sc.pivot, sc.x0, sc.y0, STEP, NXY, NXY, sc.table)
    idx, sco = R.peaks(vol, (NTHETA, NXY, NXY), True, K)
    recs = []
    for i in idx:
        m, c, s = start_of(sc, i)
        recs.append(refine(sc.view_b, pts, sc.pivot, m, c, s, ITERATIONS, sc.max_trunc, sc.lever))
    return idx, sco, recs
