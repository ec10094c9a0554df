"""The fields rule of include/tsd_hip.h (tsd_route_fields_*, tsd_view_assign_fields) restated on top of route_ref, frontier_ref,
view_ref and waypoint_ref, written from the rule and not from the kernels: a layer is route_ref.route with every other seed moved
outside the map, the goal matrix is route_ref.goals per layer, the assignment is the header's nine steps in plain Python."""
import numpy as np

from tests import frontier_ref as FR
from tests import route_ref as RR
from tests import view_ref as VR
from tests import waypoint_ref as WR

NONE = RR.NONE
MAX_SEEDS = 16


def fields(m, seeds, free_max=0, w=None, limit=0):
    """(keys (L, H, W) uint32, used: list of 0 / 1 per seed): layer r is the routes' key image of the list with every seed but r
    moved to (-1, -1), so seed r keeps its index in the key's low four bits"""
    seeds = [tuple(s) for s in seeds]
    layers, used = [], []
    for r in range(len(seeds)):
        alone = [seeds[i] if i == r else (-1, -1) for i in range(len(seeds))]
        keys, n = RR.route(m, alone, free_max, w, limit)
        layers.append(keys)
        used.append(n)
    return np.stack(layers), used


def goal_matrix(keys, labels, records):
    """tsd_route_fields_goals: RR.GOAL_DTYPE (L, n), row r the routes' goals on layer r"""
    out = np.zeros((keys.shape[0], records.size), dtype=RR.GOAL_DTYPE)
    for r in range(keys.shape[0]):
        out[r] = RR.goals(keys[r], labels, records)
    return out


def trace(keys, wi, goal_cells, goal_layers, max_len):
    """tsd_route_fields_trace: the routes' trace of goal g on layer goal_layers[g]"""
    paths, lens = [], []
    for c, l in zip(goal_cells, goal_layers):
        p, n = RR.trace(keys[int(l)], wi, [int(c)], max_len)
        paths.append(p[0])
        lens.append(int(n[0]))
    return paths, np.array(lens, dtype=np.int32)


def waypoints(keys, wi, goal_cells, goal_layers, lookahead, slack, max_len):
    """tsd_route_fields_waypoints: the routes' waypoints of goal g on layer goal_layers[g]"""
    ways, info = [], np.zeros(len(goal_cells), dtype=WR.INFO_DTYPE)
    for g, (c, l) in enumerate(zip(goal_cells, goal_layers)):
        w, i = WR.waypoints(keys[int(l)], wi, [int(c)], lookahead, slack, max_len)
        ways.append(w[0])
        info[g] = i[0]
    return ways, info


def assign_fields(m, goals, R, gain_weight, free_max=0, unknown_depth=0, gains=None):
    """tsd_view_assign_fields on the goal matrix goals[r][f] (RR.GOAL_DTYPE, shape (n_robots, n_frontiers)):
    (goal_of_robot int32[n_robots] -- a frontier index or -1 --, picked GAIN_DTYPE[n_robots], rounds, the claims image it leaves).
    gains: a stand-in for view_ref.gains with the same signature (the tests of the rule's order use one)."""
    gains = VR.gains if gains is None else gains
    m = np.asarray(m, dtype=np.int8)
    goals = np.asarray(goals, dtype=RR.GOAL_DTYPE)
    n_robots, n_frontiers = goals.shape
    claims = np.zeros(m.shape, dtype=np.uint8)                                     # 1. the claims are reset at the map's size
    goal_of = np.full(n_robots, -1, dtype=np.int32)
    picked = np.zeros(n_robots, dtype=VR.GAIN_DTYPE)
    picked["cell"] = NONE
    # 2. every pair with a cell is remaining
    remaining = [(r, f) for r in range(n_robots) for f in range(n_frontiers) if int(goals[r, f]["cell"]) != NONE]
    rounds = 0
    while remaining:                                                               # 9. while pairs remain
        rounds += 1
        # 3. the gains of the cells of all remaining pairs, claims in use, each distinct cell once
        cells = sorted({int(goals[r, f]["cell"]) for r, f in remaining})
        rec = {int(g["cell"]): g for g in gains(m, cells, R, free_max, unknown_depth, claims)}
        # 4., 5. only pairs with a gain compete; the highest score, then the lower f, then the lower r
        best = None
        for r, f in remaining:
            g = rec[int(goals[r, f]["cell"])]
            if int(g["gain"]) == 0:
                continue
            score = int(g["gain"]) * int(gain_weight) - int(goals[r, f]["dist"])
            key = (-score, f, r)
            if best is None or key < best[0]:
                best = (key, r, f, g)
        if best is None:                                                           # 6. no pair competes
            break
        _, r, f, g = best
        goal_of[r] = f                                                             # 7.
        picked[r] = g
        VR.claim(m, claims, [int(goals[r, f]["cell"])], R, free_max, unknown_depth)
        remaining = [(q, k) for q, k in remaining if q != r and k != f]           # 8.
    return goal_of, picked, rounds, claims


def convoy():
    """view_ref.two_rooms()'s corridor with its three doorways, the two robots one behind the other at its left end: robot 0 at
    (12, 42) is nearer to every doorway than robot 1 at (4, 42).  Returns (map, seeds, joint goals, goal matrix): the goals of the
    restatements on the joint field and on a field per robot."""
    m, _, _ = VR.two_rooms()
    seeds = [(12, 42), (4, 42)]
    rec, lab, _ = FR.frontiers(m, 0, 1, seeds)
    joint = RR.goals(RR.route(m, seeds)[0], lab, rec)
    keys, _ = fields(m, seeds)
    return m, seeds, joint, goal_matrix(keys, lab, rec)
