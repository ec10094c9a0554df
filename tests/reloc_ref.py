"""Plain numpy restatement of the relocalisation rules of include/tsd_hip.h (tsd_relocalize): the score of a pose candidate, the
peak rule and the winner rule -- written from the header's text on a canonical tile dump (``download_tiles`` / the oracle's
``dump``), not from the kernels.  ``GridView.bilinear`` mirrors oracle/tsd_oracle.c: ora_interpolate_bilinear statement for
statement.  Also the one scene the relocalisation tests share (``scene``), built once per process with the oracle.
"""
import functools
import itertools
import math

import numpy as np

SUCCESS, INVALIDINDEX, EMPTYPARTITION, ISNAN = 0, 1, 2, 3
ONE = 1048576          # 2^20: the weight of a scan point that lies exactly on a surface


class GridView:
    """a tile dump (initialized[tiles], init_weight[tiles], tsd[tiles][1089], weight[tiles][1089]) with the grid's geometry"""

    def __init__(self, dump, cells, cell_size):
        self.init = np.asarray(dump[0]).astype(bool)
        self.tsd = np.asarray(dump[2], dtype=np.float64).reshape(-1, 33 * 33)
        self.N, self.PX = int(cells), int(cells) // 32
        self.cs, self.inv_cs = float(cell_size), 1.0 / float(cell_size)

    def bilinear(self, x, y):
        """TsdGrid::interpolateBilinear on arrays: (status, value); the value is meaningful where status == SUCCESS"""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        cs, inv = self.cs, self.inv_cs
        # coord2Cell
        xi = np.floor(x * inv).astype(np.int64)
        yi = np.floor(y * inv).astype(np.int64)
        dx = (xi.astype(np.float64) + 0.5) * cs
        dy = (yi.astype(np.float64) + 0.5) * cs
        lo = x < dx
        xi = np.where(lo, xi - 1, xi); dx = np.where(lo, dx - cs, dx)
        lo = y < dy
        yi = np.where(lo, yi - 1, yi); dy = np.where(lo, dy - cs, dy)
        status = np.full(x.shape, SUCCESS, dtype=np.int32)
        outside = (xi >= self.N) | (xi < 0) | (yi >= self.N) | (yi < 0)
        xc, yc = np.where(outside, 0, xi), np.where(outside, 0, yi)
        p = (yc >> 5) * self.PX + (xc >> 5)
        lx, ly = xc & 31, yc & 31
        empty = ~self.init[p]
        wx = np.abs((x - dx) * inv)
        wy = np.abs((y - dy) * inv)
        t = self.tsd
        with np.errstate(invalid="ignore"):
            v = (t[p, ly * 33 + lx] * (1. - wy) * (1. - wx)
                 + t[p, (ly + 1) * 33 + lx] * wy * (1. - wx)
                 + t[p, ly * 33 + lx + 1] * (1. - wy) * wx
                 + t[p, (ly + 1) * 33 + lx + 1] * wy * wx)
        status[np.isnan(v)] = ISNAN
        status[empty] = EMPTYPARTITION
        status[outside] = INVALIDINDEX
        return status, v


def rotation_table(ntheta, theta0, dtheta):
    """cos / sin of theta0 + k * dtheta with libm, (ntheta, 2): what the host fills in for a NULL table"""
    return np.array([[math.cos(theta0 + float(k) * dtheta), math.sin(theta0 + float(k) * dtheta)] for k in range(ntheta)])


def scores(view, points_xy, x0, y0, step, nx, ny, cos_sin):
    """(volume uint32 [ntheta, ny, nx], gate bool [ny, nx]): the score of every candidate and which positions pass the gate"""
    pts = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2)
    px, py = pts[:, 0][None, :], pts[:, 1][None, :]
    tab = np.asarray(cos_sin, dtype=np.float64).reshape(-1, 2)
    tx = np.tile(x0 + np.arange(nx).astype(np.float64) * step, ny)
    ty = np.repeat(y0 + np.arange(ny).astype(np.float64) * step, nx)
    st, v = view.bilinear(tx, ty)
    with np.errstate(invalid="ignore"):
        gate = (st == SUCCESS) & (v > 0)
    vol = np.zeros((tab.shape[0], ny * nx), dtype=np.uint32)
    sel = np.flatnonzero(gate)
    gx, gy = tx[sel][:, None], ty[sel][:, None]
    for k in range(tab.shape[0]):
        c, s = tab[k, 0], tab[k, 1]
        wx = (c * px - s * py) + gx
        wy = (s * px + c * py) + gy
        st, v = view.bilinear(wx, wy)
        ok = st == SUCCESS
        term = np.zeros(v.shape, dtype=np.uint32)
        term[ok] = (np.uint32(ONE) - np.rint(np.abs(v[ok]) * 1048576.0).astype(np.uint32)).astype(np.uint32)
        vol[k, sel] = term.sum(axis=1, dtype=np.uint32)
    return vol.reshape(tab.shape[0], ny, nx), gate.reshape(ny, nx)


def peaks(volume, shape, wraps, K):
    """(idx, score) of the K best peaks of a volume of shape (ntheta, ny, nx): score > 0 and, against every lattice neighbour n
    (up to 26; k wraps when `wraps`), score > score_n or (score == score_n and idx < idx_n).  Score descending, idx ascending."""
    nt, ny, nx = (int(v) for v in shape)
    S = np.asarray(volume).reshape(nt, ny, nx).astype(np.int64)
    flat = S.reshape(-1)
    idx = np.arange(flat.size, dtype=np.int64).reshape(nt, ny, nx)
    kk0, yy0, xx0 = np.meshgrid(np.arange(nt), np.arange(ny), np.arange(nx), indexing="ij")
    ok = S > 0
    for dk, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        if dk == dy == dx == 0:
            continue
        kk, yy, xx = kk0 + dk, yy0 + dy, xx0 + dx
        valid = (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
        if wraps:
            kk = kk % nt
        else:
            valid &= (kk >= 0) & (kk < nt)
        nidx = (np.clip(kk, 0, nt - 1) * ny + np.clip(yy, 0, ny - 1)) * nx + np.clip(xx, 0, nx - 1)
        valid &= nidx != idx                       # a candidate is not its own neighbour (one rotation that wraps onto itself)
        sn = flat[nidx]
        ok &= ~valid | (S > sn) | ((S == sn) & (idx < nidx))
    cand = np.flatnonzero(ok.reshape(-1))
    order = np.lexsort((cand, -flat[cand]))
    top = cand[order][:K]
    return top.astype(np.int32), flat[top].astype(np.uint32)


def winner(pairs):
    """IcpMultiInitIterator's assignBetterSolution over the refined peaks in order: strictly more pairs win (-1: nothing refined)"""
    best = -1
    for j, p in enumerate(pairs):
        if best < 0 or p > pairs[best]:
            best = j
    return best


def candidate_pose(idx, x0, y0, step, nx, ny, cos_sin):
    """3 x 3 pose of candidate idx = (k * ny + iy) * nx + ix"""
    k, rem = divmod(int(idx), nx * ny)
    iy, ix = divmod(rem, nx)
    c, s = np.asarray(cos_sin, dtype=np.float64).reshape(-1, 2)[k]
    return np.array([[c, -s, x0 + float(ix) * step], [s, c, y0 + float(iy) * step], [0.0, 0.0, 1.0]])


def rays_world(pose, rays_local, cell_size):
    """Sensor::transform then getNormalizedRayMap(cellSize) from _rayNorm = 1, in the operation order of tsd_relocalize"""
    rl = np.asarray(rays_local, dtype=np.float64)
    b = rl.size // 2
    x, y = rl[:b], rl[b:]
    wx = (0.0 + pose[0, 0] * x) + pose[0, 1] * y
    wy = (0.0 + pose[1, 0] * x) + pose[1, 1] * y
    if cell_size != 1.0:
        wx, wy = wx * (cell_size / 1.0), wy * (cell_size / 1.0)
    return np.concatenate([wx, wy])


def pose_error(pose, truth):
    """(metres, radians) between a 3 x 3 pose and (x, y, yaw)"""
    d = math.hypot(pose[0, 2] - truth[0], pose[1, 2] - truth[1])
    a = math.atan2(pose[1, 0], pose[0, 0]) - truth[2]
    return d, abs(math.atan2(math.sin(a), math.cos(a)))


# ---- the scene the tests share ---------------------------------------------------------------------------------------------------
MAX_RANGE, MIN_RANGE, LOW_REFL = 30.0, 0.001, 2.0
ICP = dict(iterations=30, dist_max=0.4, dist_min=0.02)
STEP, NXY, NTHETA, DTHETA = 0.1, 24, 36, math.radians(10.0)
PUSHED = 12                      # trajectory poses whose scans make the map
# the pose to find: never pushed, between the lattice's nodes in x, y and theta, turned by 123 degrees against the trajectory (yaw 0.1 ..)
TRUTH_OFFSET = (0.93, 0.38, 0.1 + math.radians(123.0))


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def scene(beams):
    """The oracle-built map and the query scan for `beams` = 360 (full circle) or 1081 (270 degrees): pillars world, 512^2 cells of
    0.05 m, PUSHED scans pushed at their true poses, and the lattice of 24 x 24 x 36 around the query pose."""
    from ohm_tsd_slam_amd import synth
    from oracle import pyoracle as O
    O.build()
    sc = Scene()
    sc.gc = synth.GridConfig(9, 0.05)
    sc.geo = synth.ScanGeometry.full_circle_360() if beams == 360 else synth.ScanGeometry.utm30lx()
    geo = sc.geo
    world = synth.World("pillars", sc.gc)
    poses = synth.trajectory(world, PUSHED, step_x=0.25, step_yaw=0.01)
    grid = O.Grid(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
    for p in poses:
        data, mask = O.ingest_f32(world.scan(p[0], p[1], p[2], geo), MAX_RANGE, geo.angle_increment)
        grid.push(synth.pose_matrix(*p), data, mask, geo.angle_increment, geo.angle_min, MAX_RANGE, MIN_RANGE, LOW_REFL)
    sc.world, sc.grid, sc.poses = world, grid, poses
    sc.dump = grid.dump()
    sc.view = GridView(sc.dump, grid.cells, sc.gc.cell_size)
    sc.truth = (world.start[0] + TRUTH_OFFSET[0], world.start[1] + TRUTH_OFFSET[1], TRUTH_OFFSET[2])
    # lattice: the truth lies 11.4 / 11.7 steps from the corner and 0.3 of a rotation step from a node
    sc.x0, sc.y0 = sc.truth[0] - 11.4 * STEP, sc.truth[1] - 11.7 * STEP
    sc.theta0 = sc.truth[2] - 12.3 * DTHETA
    sc.table = rotation_table(NTHETA, sc.theta0, DTHETA)
    sc.rays_local = O.rays_local(geo.beams, geo.angle_min, geo.angle_increment)
    sc.data, sc.mask = O.ingest_f32(world.scan(*sc.truth, geo), MAX_RANGE, geo.angle_increment)
    scene_xy, ms, _ = O.scene_from_scan(sc.rays_local, sc.data, sc.mask)
    sc.points = scene_xy.reshape(-1, 2)[ms.astype(bool)].copy()
    sc.bounds = (0.0, grid.max_x, 0.0, grid.max_x)
    return sc


@functools.lru_cache(maxsize=None)
def scene_scores(beams):
    """the restatement's volume and gate for scene(beams), computed once"""
    sc = scene(beams)
    return scores(sc.view, sc.points, sc.x0, sc.y0, STEP, NXY, NXY, sc.table)


def oracle_refine(sc, pose):
    """the oracle's ray cast + ICP from `pose`: dict(T, pairs, ..) or None without a model"""
    from oracle import pyoracle as O
    rw = rays_world(pose, sc.rays_local, sc.gc.cell_size)
    co, _, mo, cnt = sc.grid.raycast(pose, rw, MIN_RANGE, MAX_RANGE)
    if cnt == 0:
        return None
    M = co.reshape(-1, 2)[mo.astype(bool)]
    return O.icp(M, sc.points, pose, ICP["iterations"], ICP["dist_max"], ICP["dist_min"], sc.bounds)


# ---- hand-made volumes for the peak rule: name -> (volume [ntheta, ny, nx], wraps, expected peak indices in output order or None) ----
def handmade_volumes():
    out = {}
    out["all_zero"] = (np.zeros((3, 4, 5), dtype=np.uint32), False, [])
    v = np.zeros((3, 4, 5), dtype=np.uint32); v[1, 2, 3] = 9; v[1, 2, 2] = 4
    out["one_interior"] = (v, False, [(1 * 4 + 2) * 5 + 3])
    v = np.ones((3, 5, 7), dtype=np.uint32); v[0, 0, 0] = 8; v[2, 4, 6] = 8; v[1, 2, 3] = 6
    out["two_equal_maxima"] = (v, False, [0, (2 * 5 + 4) * 7 + 6, (1 * 5 + 2) * 7 + 3])
    v = np.zeros((3, 5, 7), dtype=np.uint32); v[1, 1:3, 2:5] = 5
    out["plateau"] = (v, False, [(1 * 5 + 1) * 7 + 2])                      # the plateau's lowest index alone
    v = np.full((1, 4, 4), 3, dtype=np.uint32)
    out["flat_everywhere"] = (v, True, [0])
    v = np.zeros((3, 3, 3), dtype=np.uint32)
    for k, y, x in itertools.product((0, 2), repeat=3):
        v[k, y, x] = 5
    corners = [(k * 3 + y) * 3 + x for k, y, x in itertools.product((0, 2), repeat=3)]
    out["corners_nowrap"] = (v, False, sorted(corners))
    out["corners_wrap"] = (v, True, sorted(c for c in corners if c < 9))     # k = 0 and k = 2 are neighbours: the lower index keeps the tie
    v = np.zeros((4, 5, 6), dtype=np.uint32); v[0, 2, 3] = 7; v[3, 2, 3] = 9; v[2, 0, 5] = 3
    out["faces_nowrap"] = (v, False, [(3 * 5 + 2) * 6 + 3, (0 * 5 + 2) * 6 + 3, (2 * 5 + 0) * 6 + 5])
    out["faces_wrap"] = (v, True, [(3 * 5 + 2) * 6 + 3, (2 * 5 + 0) * 6 + 5])
    v = np.zeros((2, 3, 3), dtype=np.uint32); v[0, 1, 1] = 4; v[1, 1, 1] = 4
    out["two_rotations_wrap"] = (v, True, [4])                               # k - 1 and k + 1 are the same neighbour
    # more peaks than K, many equal scores: every other node of a (4, 20, 20) lattice
    v = np.zeros((4, 20, 20), dtype=np.uint32)
    for k, y, x in itertools.product(range(0, 4, 2), range(0, 20, 2), range(0, 20, 2)):
        v[k, y, x] = 1 + (((k * 20 + y) * 20 + x) * 7919) % 37
    out["many_peaks"] = (v, True, None)
    # one line of a million nodes, every other one a peak: more peaks per workgroup than its buffer holds
    n = 1000000
    v = np.zeros((1, n, 1), dtype=np.uint32)
    v[0, ::2, 0] = 1 + (np.arange(0, n, 2, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(100003)).astype(np.uint32)
    out["long_line"] = (v, False, None)
    return out
