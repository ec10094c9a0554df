"""The route rule of include/tsd_hip.h restated in numpy and plain Python, written from the rule and not from the kernels: the keys
by vectorised gather sweeps to the fixed point, the goals by a plain minimum over each frontier's cells, the paths by the stated
neighbour order.  ``route`` returns what tsd_route_dev leaves in its key image.  The maps the CPU and the GPU tests share are
drawn here as well (``cases``)."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_DIST = 0x0FFFF000
OFFS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))       # neighbour k, (dx, dy)
COST = (5, 5, 5, 5, 7, 7, 7, 7)
GOAL_DTYPE = np.dtype([("cell", "<u4"), ("dist", "<u4"), ("seed", "<i4"), ("reserved", "<u4")])
U, O = -1, 100
_INF = 1 << 40


def weights(free_max, max_weight):
    """tsd_route_weights: W[v] = 1 + v * (max_weight - 1) / 98 by integer division, at most 255 (v = 99 alone can pass it)"""
    return np.array([min(255, 1 + v * (max_weight - 1) // 98) for v in range(free_max + 1)], dtype=np.uint8)


def weight_image(m, free_max=0, w=None):
    """int64 (H, W): W[v] on the traversable cells, 0 elsewhere"""
    m = np.asarray(m, dtype=np.int8)
    t = (m >= 0) & (m <= free_max)
    table = np.ones(free_max + 1, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    assert table.size == free_max + 1 and (table >= 1).all() and (table <= 255).all()
    wi = np.zeros(m.shape, dtype=np.int64)
    wi[t] = table[m[t].astype(np.int64)]
    return wi


def _shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx], ``fill`` outside"""
    H, W = a.shape
    p = np.full((H + 2, W + 2), fill, dtype=a.dtype)
    p[1:-1, 1:-1] = a
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def moves(wi):
    """bool (8, H, W): [k, y, x] where the move from neighbour k of (x, y) onto (x, y) is allowed"""
    t = wi > 0
    out = []
    for k, (dx, dy) in enumerate(OFFS):
        ok = t & _shift(t, dx, dy, False)
        if k >= 4:
            ok = ok & _shift(t, dx, 0, False) & _shift(t, 0, dy, False)       # the two cells a diagonal cuts
        out.append(ok)
    return np.stack(out)


def route(m, seeds, free_max=0, w=None, limit=0):
    """(keys (H, W) uint32, seeds_used).  Sweeps in which every cell takes the minimum over its eight neighbours, until a sweep lowers
    nothing; a sweep only visits the bounding box, grown by one cell, of the cells the sweep before lowered (no other cell has a
    neighbour that changed)."""
    m = np.asarray(m, dtype=np.int8)
    H, W = m.shape
    wi = weight_image(m, free_max, w)
    mv = moves(wi)
    step = [(COST[k] * wi) << 4 for k in range(8)]
    lim_key = ((limit if limit else MAX_DIST) << 4) | 15
    K = np.full((H + 2, W + 2), _INF, dtype=np.int64)          # (with a border, so that a window's neighbours are slices)
    used = []
    for i, (x, y) in enumerate(seeds):
        if 0 <= x < W and 0 <= y < H and wi[y, x] > 0:
            used.append((x, y))
            K[y + 1, x + 1] = min(K[y + 1, x + 1], i)
    if used:
        xs, ys = [x for x, _ in used], [y for _, y in used]
        x0, x1, y0, y1 = max(min(xs) - 1, 0), min(max(xs) + 2, W), max(min(ys) - 1, 0), min(max(ys) + 2, H)
        while True:
            sub = K[y0 + 1:y1 + 1, x0 + 1:x1 + 1]
            new = sub.copy()
            for k, (dx, dy) in enumerate(OFFS):
                nb = K[y0 + 1 + dy:y1 + 1 + dy, x0 + 1 + dx:x1 + 1 + dx]
                cand = nb + step[k][y0:y1, x0:x1]
                new = np.minimum(new, np.where(mv[k][y0:y1, x0:x1] & (nb < _INF) & (cand <= lim_key), cand, _INF))
            cy, cx = np.nonzero(new < sub)
            if cy.size == 0:
                break
            K[y0 + 1:y1 + 1, x0 + 1:x1 + 1] = new
            x0, x1, y0, y1 = max(x0 + cx.min() - 1, 0), min(x0 + cx.max() + 2, W), max(y0 + cy.min() - 1, 0), min(y0 + cy.max() + 2, H)
    K = K[1:-1, 1:-1]
    return np.where(K < _INF, K, NONE).astype(np.uint32), len(used)


def goals(keys, labels, records):
    """tsd_route_goals: one GOAL_DTYPE entry per frontier record"""
    H, W = keys.shape
    out = np.zeros(records.size, dtype=GOAL_DTYPE)
    flat_k, flat_l = keys.ravel().astype(np.uint64), labels.ravel()
    for n, r in enumerate(records):
        cells = np.nonzero((flat_l == int(r["root_y"]) * W + int(r["root_x"])) & (flat_k != NONE))[0]
        if cells.size == 0:
            out[n] = (NONE, NONE, -1, 0)
            continue
        best = int(((flat_k[cells] << np.uint64(32)) | cells.astype(np.uint64)).min())
        out[n] = (best & 0xFFFFFFFF, best >> 36, (best >> 32) & 15, 0)
    return out


def trace(keys, wi, goal_cells, max_len):
    """tsd_route_trace: (list of paths -- each cut at max_len, goal first --, lengths)"""
    H, W = keys.shape
    paths, lens = [], []
    for b in goal_cells:
        b = int(b)
        path, n = [], 0
        if b < W * H and keys[b // W, b % W] != NONE:
            while True:
                path.append(b)
                n += 1
                x, y = b % W, b // W
                kb = int(keys[y, x])
                if kb >> 4 == 0:
                    break
                for k, (dx, dy) in enumerate(OFFS):
                    ax, ay = x - dx, y - dy                    # a = b - offset_k
                    if not (0 <= ax < W and 0 <= ay < H and wi[ay, ax] > 0):
                        continue
                    if k >= 4 and not (wi[y, ax] > 0 and wi[ay, x] > 0):
                        continue
                    ka = int(keys[ay, ax])
                    if ka != NONE and ka + ((COST[k] * int(wi[y, x])) << 4) == kb:
                        b = ay * W + ax
                        break
                else:
                    n = -1
                    break
        paths.append(path[:max_len])
        lens.append(n)
    return paths, np.array(lens, dtype=np.int32)


# ---- the maps
def serpentine(n=256):
    """a one-cell corridor of free cells in unknown space through every tile, turning at alternate ends"""
    src = np.full((n, n), U, dtype=np.int8)
    rows = list(range(16, n, 32))
    for k, y in enumerate(rows):
        src[y, 8:n - 8] = 0
        if k + 1 < len(rows):
            src[y:rows[k + 1] + 1, (n - 9) if k % 2 == 0 else 8] = 0
    return src


def corner_wall(W, H, anti):
    """two rooms whose only opening is the diagonal across the corner of four tiles at (32, 32): the wall runs down one column above
    y = 32 and down the next one below"""
    src = np.zeros((H, W), dtype=np.int8)
    src[:32, 32 if anti else 31] = O
    src[32:, 31 if anti else 32] = O
    return src


def random_map(W, H, density, seed):
    """obstacles at ``density``, 2 % unknown cells, costs 0 .. 55 elsewhere (above free_max = 50: not traversable)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 56, size=(H, W)).astype(np.int8)
    r = rng.random((H, W))
    src[r < density] = O
    src[r > 0.98] = U
    return src


def random_weights(seed, free_max=50):
    return np.random.default_rng(seed).integers(1, 256, size=free_max + 1).astype(np.uint8)


SHAPES = [(1, 300, 1), (300, 1, 300), (33, 33, 33), (64, 64, 72), (97, 130, 97), (256, 256, 256)]      # width, height, stride


def cases():
    """[(name, map, stride, dict(seeds, free_max, w, limit, max_rounds))]: every map of the route tests but the frame's"""
    out = []

    def add(name, src, stride=None, seeds=(), free_max=0, w=None, limit=0, max_rounds=0):
        out.append((name, src, src.shape[1] if stride is None else stride,
                    dict(seeds=list(seeds), free_max=free_max, w=w, limit=limit, max_rounds=max_rounds)))

    for W, H, stride in SHAPES:
        add(f"open_{W}x{H}", np.zeros((H, W), dtype=np.int8), stride, [(W // 3, H // 3)])
    seam = np.zeros((64, 64), dtype=np.int8)
    seam[:, 32] = O
    seam[40, 32] = 0
    add("seam_wall_one_gap_64x64", seam, 72, [(5, 5)])
    seam = np.zeros((130, 97), dtype=np.int8)
    seam[64, :] = O
    seam[64, 50] = 0
    add("seam_wall_one_gap_97x130", seam, 97, [(90, 3)])
    for W, H, stride in ((64, 64, 72), (97, 130, 97)):
        for anti in (False, True):
            add(f"corner_{'anti' if anti else ''}diagonal_{W}x{H}", corner_wall(W, H, anti), stride, [(5, 5)])
    add("serpentine", serpentine(), 256, [(8, 16)], max_rounds=1024)
    add("equidistant_column", np.zeros((33, 33), dtype=np.int8), 33, [(28, 16), (4, 16)])
    add("two_seeds_one_cell", np.zeros((33, 33), dtype=np.int8), 33, [(10, 10), (10, 10), (20, 20)])
    src = np.zeros((64, 64), dtype=np.int8)
    src[3, 3], src[4, 4] = O, U
    add("seeds_ignored", src, 72, [(3, 3), (4, 4), (-1, 5), (64, 5), (5, 64), (30, 30)])
    src = random_map(97, 130, 0.05, 160)
    ys, xs = np.nonzero((src >= 0) & (src <= 50))
    pick = np.random.default_rng(16).choice(xs.size, size=16, replace=False)
    add("sixteen_seeds", src, 97, [(int(xs[i]), int(ys[i])) for i in pick], free_max=50, w=random_weights(161))
    add("limit_100", np.zeros((33, 33), dtype=np.int8), 33, [(0, 0)], limit=100)
    add("weights_255_1x300", np.zeros((300, 1), dtype=np.int8), 1, [(0, 0)], w=np.array([255], dtype=np.uint8))
    band = np.zeros((130, 97), dtype=np.int8)
    band[:, 47:50] = O
    band[20:23, 47:50] = 50
    band[120, 47:50] = 0
    add("cost_band", band, 97, [(10, 21)], free_max=50, w=weights(50, 255))
    for W, H, stride in ((33, 33, 33), (64, 64, 72), (97, 130, 97)):
        for n, density in enumerate((0.05, 0.15, 0.30)):
            rng = np.random.default_rng(1000 + 10 * W + n)
            seeds = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(3)] + [(W + 3, 2)]
            add(f"random_{density}_{W}x{H}", random_map(W, H, density, 7 * W + n), stride, seeds, free_max=50, w=random_weights(W + n),
                limit=20000 if n == 1 else 0)
    return out
