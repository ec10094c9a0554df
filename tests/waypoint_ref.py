"""The waypoint rule of include/tsd_hip.h (tsd_route_waypoints) restated in plain Python on top of route_ref, written from the rule
and not from the kernel: the trace reversed into driving order, the line's closed form step by step, the segment test under the
routes' move rule, and the greedy choice of the largest candidate of the look-ahead window.  Cells are (x, y) pairs here; the
results hold linear indices like the library's."""
import numpy as np

from tests import route_ref as R

INFO_DTYPE = np.dtype([("len", "<i4"), ("n_way", "<i4"), ("cost", "<u4"), ("dist", "<u4")])
MAX_LOOKAHEAD = 1024


def _sgn(v):
    return (v > 0) - (v < 0)


def line(p, q):
    """the cells of steps 1 .. N of the line p -> q, N = max(|dx|, |dy|) >= 1; the last one is q"""
    dx, dy = q[0] - p[0], q[1] - p[1]
    ax, ay = abs(dx), abs(dy)
    N = max(ax, ay)
    assert N >= 1
    return [(p[0] + _sgn(dx) * ((2 * j * ax + N) // (2 * N)), p[1] + _sgn(dy) * ((2 * j * ay + N) // (2 * N))) for j in range(1, N + 1)]


def segment(wi, p, q, bound=None):
    """(passes, cost) of the segment p -> q on the weight image: every step a move of the routes' rule -- the cell entered
    traversable, and on a diagonal step BOTH cells it cuts --, the cost the sum of c * w[cell entered].  Where a step is refused the
    answer is (False, the cost up to that step).  bound: a segment that costs more does not pass either, and the walk ends at the
    step that exceeds it (the costs are positive)."""
    cost, prev = 0, p
    for c in line(p, q):
        w = int(wi[c[1], c[0]])
        diag = c[0] != prev[0] and c[1] != prev[1]
        if w == 0 or (diag and (wi[prev[1], c[0]] == 0 or wi[c[1], prev[0]] == 0)):
            return False, cost
        cost += (7 if diag else 5) * w
        if bound is not None and cost > bound:
            return False, cost
        prev = c
    return True, cost


def waypoints(keys, wi, goal_cells, lookahead, slack, max_len):
    """tsd_route_waypoints: (list of uint32 arrays of linear cell indices, seed first and goal last, NOT cut at any max_way; info as
    INFO_DTYPE[n_goals])"""
    assert 1 <= lookahead <= MAX_LOOKAHEAD and max_len >= 1 and slack >= 0
    H, W = keys.shape
    goal_cells = [int(g) for g in goal_cells]
    paths, lens = R.trace(keys, wi, goal_cells, 1 << 30)
    ways, info = [], np.zeros(len(goal_cells), dtype=INFO_DTYPE)
    for g, b in enumerate(goal_cells):
        n = int(lens[g])
        dist = int(keys[b // W, b % W]) >> 4 if b < W * H and keys[b // W, b % W] != R.NONE else R.NONE
        way, cost = [], 0
        if 0 < n <= max_len:
            p = [(c % W, c // W) for c in reversed(paths[g])]
            d = [int(keys[y, x]) >> 4 for x, y in p]
            a = 0
            way.append(a)
            while a < n - 1:
                best = None
                for j in range(min(a + lookahead, n - 1), a, -1):          # (descending: the first hit is the largest j)
                    ok, c = segment(wi, p[a], p[j], d[j] - d[a] + slack)
                    if ok:
                        best = (j, c)
                        break
                assert best is not None, "a traced step always qualifies"
                a = best[0]
                cost += best[1]
                way.append(a)
            way = [p[i][1] * W + p[i][0] for i in way]
        ways.append(np.array(way, dtype=np.uint32))
        info[g] = (n, len(way), cost & 0xFFFFFFFF, dist)
    return ways, info
