"""The view rule of include/tsd_hip.h (tsd_view_*) restated in numpy, written from the rule and not from the kernel: all 8R rays of a
candidate advance one step at a time as arrays, every test in the rule's order.  ``gains`` returns what tsd_view_gains writes,
``claim`` what tsd_view_claim leaves in the claims image, ``assign`` what tsd_view_assign answers.  The maps and candidates the CPU
and the GPU tests share are drawn here as well (``cases``)."""
import numpy as np

from tests import route_ref as RR

NONE = 0xFFFFFFFF
MAX_RADIUS = 511
MAX_CELLS = 4096
GAIN_DTYPE = np.dtype([("cell", "<u4"), ("gain", "<u4"), ("unknown", "<u4"), ("visible", "<u4")])
U, O = -1, 100


def targets(R):
    """(8R, 2) int64: the cells of the Chebyshev ring of radius R as offsets (tx, ty), in the rule's order"""
    top = [(x, -R) for x in range(-R, R + 1)]
    right = [(R, y) for y in range(-R + 1, R + 1)]
    bottom = [(x, R) for x in range(R - 1, -R - 1, -1)]
    left = [(-R, y) for y in range(R - 1, -R, -1)]
    t = np.array(top + right + bottom + left, dtype=np.int64)
    assert t.shape == (8 * R, 2)
    return t


def view(m, cell, R, free_max=0, unknown_depth=0):
    """bool (H, W): V(cell)"""
    m = np.asarray(m, dtype=np.int8)
    H, W = m.shape
    seen = np.zeros((H, W), dtype=bool)
    cell = int(cell)
    if cell >= W * H:
        return seen
    cx, cy = cell % W, cell // W
    if m[cy, cx] > free_max:
        return seen
    seen[cy, cx] = True
    t = targets(R)
    sx, sy, ax, ay = np.sign(t[:, 0]), np.sign(t[:, 1]), np.abs(t[:, 0]), np.abs(t[:, 1])
    blocking = m > free_max
    alive = np.ones(8 * R, dtype=bool)
    unknowns = np.zeros(8 * R, dtype=np.int64)
    px, py = np.full(8 * R, cx, dtype=np.int64), np.full(8 * R, cy, dtype=np.int64)
    for j in range(1, R + 1):
        ox, oy = (2 * j * ax + R) // (2 * R), (2 * j * ay + R) // (2 * R)
        x, y = cx + sx * ox, cy + sy * oy
        alive &= ox * ox + oy * oy <= R * R                                        # 1: the range is a disc
        alive &= (x >= 0) & (x < W) & (y >= 0) & (y < H)                           # 2: outside the map
        i = np.nonzero(alive)[0]
        if i.size == 0:
            break
        # 3: a diagonal step between two blocking cells (the step before was seen, so both cut cells are inside the map)
        cut = (x[i] != px[i]) & (y[i] != py[i]) & blocking[py[i], x[i]] & blocking[y[i], px[i]]
        alive[i[cut]] = False
        i = i[~cut]
        wall = blocking[y[i], x[i]]                                                # 4: the cell is blocking
        alive[i[wall]] = False
        i = i[~wall]
        seen[y[i], x[i]] = True
        if unknown_depth > 0:
            u = i[m[y[i], x[i]] < 0]
            unknowns[u] += 1
            alive[u[unknowns[u] >= unknown_depth]] = False
        px, py = x, y
    return seen


def gains(m, cells, R, free_max=0, unknown_depth=0, claims=None):
    """GAIN_DTYPE[n]: tsd_view_gains (claims: the uint8 image where they are in use)"""
    m = np.asarray(m, dtype=np.int8)
    out = np.zeros(len(cells), dtype=GAIN_DTYPE)
    memo = {}
    for n, c in enumerate(cells):
        c = int(c)
        if c not in memo:
            v = view(m, c, R, free_max, unknown_depth)
            unk = v & (m < 0)
            memo[c] = (int(np.count_nonzero(unk if claims is None else unk & (claims == 0))), int(np.count_nonzero(unk)),
                       int(np.count_nonzero(v)))
        out[n] = (c,) + memo[c]
    return out


def claim(m, claims, cells, R, free_max=0, unknown_depth=0):
    """tsd_view_claim: 1 on every unknown cell of V(c) for every c, in place"""
    m = np.asarray(m, dtype=np.int8)
    for c in cells:
        claims[view(m, c, R, free_max, unknown_depth) & (m < 0)] = 1
    return claims


def assign(m, goals, n_robots, R, gain_weight, free_max=0, unknown_depth=0):
    """tsd_view_assign: (goal_of_robot int32[n_robots], picked GAIN_DTYPE[n_robots], rounds, the claims image it leaves).  goals: a
    structured array with cell, dist, seed (RR.GOAL_DTYPE)."""
    m = np.asarray(m, dtype=np.int8)
    claims = np.zeros(m.shape, dtype=np.uint8)
    goal_of = np.full(n_robots, -1, dtype=np.int32)
    picked = np.zeros(n_robots, dtype=GAIN_DTYPE)
    picked["cell"] = NONE
    remaining = [k for k, g in enumerate(goals) if int(g["cell"]) != NONE and 0 <= int(g["seed"]) < n_robots]
    rounds = 0
    while remaining:
        rounds += 1
        rec = gains(m, [int(goals[k]["cell"]) for k in remaining], R, free_max, unknown_depth, claims)
        best, best_score = -1, None
        for i, k in enumerate(remaining):                                          # (ascending goal index: the first of a tie stays)
            score = int(rec[i]["gain"]) * int(gain_weight) - int(goals[k]["dist"])
            if best_score is None or score > best_score:
                best, best_score = i, score
        if rec[best]["gain"] == 0:
            break
        k = remaining[best]
        seed = int(goals[k]["seed"])
        goal_of[seed] = k
        picked[seed] = rec[best]
        claim(m, claims, [int(goals[k]["cell"])], R, free_max, unknown_depth)
        remaining = [q for q in remaining if int(goals[q]["seed"]) != seed]
    return goal_of, picked, rounds, claims


# ---- the maps
def open_map(W, H, cx, cy):
    """all unknown but a clear (cx, cy)"""
    m = np.full((H, W), U, dtype=np.int8)
    m[cy, cx] = 0
    return m


def disc_cells(W, H, cx, cy, R):
    """the map cells with dx^2 + dy^2 <= R^2"""
    dx, dy = np.arange(W)[None, :] - cx, np.arange(H)[:, None] - cy
    return int(np.count_nonzero(dx * dx + dy * dy <= R * R))


def room(door=False):
    """21 x 21 unknown; [5 .. 15]^2 clear with a wall of 100 as its outline; the door opens (15, 10)"""
    m = np.full((21, 21), U, dtype=np.int8)
    m[5:16, 5:16] = O
    m[6:15, 6:15] = 0
    if door:
        m[10, 15] = 0
    return m


def diagonal_wall(n=41, anti=True):
    """n x n clear with an 8-connected wall on the (anti-)diagonal"""
    m = np.zeros((n, n), dtype=np.int8)
    i = np.arange(n)
    m[i, (n - 1 - i) if anti else i] = O
    return m


def two_rooms():
    """64 x 48: a clear corridor along y = 40 .. 44, walled in, with two robots side by side at its left end, each below a doorway
    (x = 14 .. 16 and x = 24 .. 26) that leads up into the same unknown room; a third doorway at x = 56 .. 58 leads into unknown
    space further off, walled off from the first room at x = 36.  Returns (map, seeds, goals): the goals are the route's own
    (frontiers, cost-to-go field and goals of the restatements), one per doorway: the first two nearest to robot 0 and to robot 1,
    the third nearest to robot 1."""
    from tests import frontier_ref as FR
    m = np.full((48, 64), U, dtype=np.int8)
    m[39:46, :] = O
    m[40:45, 1:63] = 0
    for x0 in (14, 24, 56):
        m[36:40, x0:x0 + 3] = 0              # a doorway, open into the unknown above
        m[36:40, x0 - 1], m[36:40, x0 + 3] = O, O
    m[:39, 36] = O
    seeds = [(15, 42), (25, 42)]
    rec, lab, _ = FR.frontiers(m, 0, 1, seeds)
    keys, _ = RR.route(m, seeds)
    return m, seeds, RR.goals(keys, lab, rec)


def standard_cells(m, rng=None):
    """the candidates every map is asked about: the four corners, an edge cell, a clear, an unknown and a blocking cell where the map
    has one (free_max 50 decides), the cell behind the last, 0xFFFFFFFE, and the first of them once more"""
    H, W = m.shape
    cells = [0, W - 1, (H - 1) * W, H * W - 1, (H // 2) * W, (H - 1) * W + W // 2]
    flat = m.ravel()
    for sel in ((flat >= 0) & (flat <= 50), flat < 0, flat > 50):
        i = np.nonzero(sel)[0]
        if i.size:
            cells.append(int(i[i.size // 2]))
    cells += [W * H, 0xFFFFFFFE, cells[0]]
    return cells


def cases():
    """[(name, map, stride, dict(cells, R, free_max, unknown_depth))]: every generic call of the view tests"""
    out = []

    def add(name, m, stride, cells, R, free_max=0, unknown_depth=0):
        out.append((name, m, m.shape[1] if stride is None else stride, dict(cells=[int(c) for c in cells], R=R, free_max=free_max,
                                                                             unknown_depth=unknown_depth)))

    # every shape: all-unknown at a small and a word-edge radius; a random map with costs at free_max 50
    for k, (W, H, stride) in enumerate(RR.SHAPES):
        c = (H // 2) * W + W // 2
        m = open_map(W, H, W // 2, H // 2)
        for R in (1, 2, 16, 33):
            add(f"open_{W}x{H}_R{R}", m, stride, standard_cells(m) + [c], R)
        rm = RR.random_map(W, H, 0.05, 300 + k)
        add(f"random_0.05_{W}x{H}_R15", rm, stride, standard_cells(rm), 15, 50)
    # every radius on two maps: sparse and dense obstacles, the depth knob at 0, 1, 3
    sparse, dense = RR.random_map(97, 130, 0.02, 41), RR.random_map(64, 64, 0.30, 42)
    for n, R in enumerate((1, 2, 15, 16, 31, 32, 33, 64)):
        add(f"random_0.02_97x130_R{R}", sparse, 97, standard_cells(sparse), R, 50, (0, 1, 3)[n % 3])
        add(f"random_0.30_64x64_R{R}", dense, 72, standard_cells(dense), R, 50, (3, 0, 1)[n % 3])
    # mostly unknown with a few walls: long rays through unknown space, the depth knob matters
    rng = np.random.default_rng(77)
    fog = np.full((130, 97), U, dtype=np.int8)
    fog[rng.random(fog.shape) < 0.03] = O
    fog[60:70, 40:60] = 0
    for depth in (0, 1, 3):
        add(f"fog_97x130_R64_depth{depth}", fog, 97, standard_cells(fog) + [65 * 97 + 50, 60 * 97 + 40], 64, 0, depth)
    add("fog_97x130_R511", fog, 97, [65 * 97 + 50, 0, 129 * 97 + 96], 511)
    add("open_97x130_R511", open_map(97, 130, 48, 65), 97, [65 * 97 + 48], 511)
    # the diagonal walls, both ways: the route tests' corner walls and a full diagonal
    for anti in (False, True):
        cw = RR.corner_wall(64, 64, anti)
        add(f"corner_wall_{'anti' if anti else 'main'}_R33", cw, 72, standard_cells(cw) + [30 * 64 + 30, 34 * 64 + 34, 33 * 64 + 30], 33)
        dw = diagonal_wall(41, anti)
        add(f"diagonal_wall_{'anti' if anti else 'main'}_R31", dw, 41, [5 * 41 + (5 if anti else 35), 20 * 41 + 19, 35 * 41 + (35 if anti else 5)], 31)
    for door in (False, True):
        for depth in (0, 2):
            add(f"room_{'door' if door else 'closed'}_depth{depth}", room(door), 21, [10 * 21 + 10, 10 * 21 + 14, 0], 20, 0, depth)
    # a cost map: 51 .. 99 block at free_max 50
    cost = np.full((64, 64), U, dtype=np.int8)
    cost[8:56, 8:56] = 20
    cost[30:34, 8:40] = 51
    cost[40, 20:56] = 99
    cost[20, 10:30] = 50
    add("costmap_free_max_50", cost, 72, standard_cells(cost) + [25 * 64 + 25, 36 * 64 + 30, 20 * 64 + 12], 32, 50)
    add("costmap_free_max_0", cost, 72, [25 * 64 + 25, 20 * 64 + 12], 32, 0)
    return out
