"""The drive rule of include/tsd_hip.h (tsd_drive_rollout, tsd_drive_fields_rollout, tsd_drive_advance) restated in numpy and plain
Python, written from the rule and not from the kernel.  Everything is int64; the direction table is read through tsd_drive_table
(host code of the library), so no cosine is computed here.  ``sample`` is the rule for one sample, step by step; ``rollout`` is the
same rule for all samples of a pose at once (numpy over the samples and the body points, a Python loop over the steps), which is
what the tests compare the device against.  The maps the CPU and the GPU tests share are drawn here as well (``cases``)."""
import numpy as np

from ohm_tsd_slam_amd import capi
from tests import route_fields_ref as RF
from tests import route_ref as RR

H = 4096
NONE = RR.NONE
DRIVE_NONE = 0xFFFFFFFFFFFFFFFF
CHOICE_DTYPE = np.dtype([("speed", "<i4"), ("turn", "<i4"), ("admissible", "<i4"), ("end_cell", "<u4"), ("d_end", "<u4"),
                         ("d_nose", "<u4"), ("cost", "<u4"), ("reserved", "<u4"), ("score", "<u8")])
_TABLE = None


def table():
    """int64 (H, 2): (cx, cy) per heading, from tsd_drive_table"""
    global _TABLE
    if _TABLE is None:
        _TABLE = capi.drive_table().astype(np.int64)
        _TABLE.setflags(write=False)
    return _TABLE


def _q16(v):
    return (v + 32768) >> 16


def advance(pose, step_q16, turn, n_steps):
    """tsd_drive_advance: (x, y, fx, fy, heading) after n_steps steps"""
    D = table()
    x0, y0, fx, fy, h0 = (int(v) for v in pose[:5])
    X, Y = fx, fy
    for k in range(1, n_steps + 1):
        h = (h0 + k * turn) % H
        X += _q16(step_q16 * int(D[h, 0]))
        Y += _q16(step_q16 * int(D[h, 1]))
    return (x0 + (X >> 16), y0 + (Y >> 16), X & 65535, Y & 65535, (h0 + n_steps * turn) % H)


def trajectory(pose, s, t, T):
    """[(X_k, Y_k, h_k, cell x, cell y)] for k = 0 .. T"""
    D = table()
    x0, y0, fx, fy, h0 = (int(v) for v in pose[:5])
    out, X, Y = [(fx, fy, h0, x0, y0)], fx, fy
    for k in range(1, T + 1):
        h = (h0 + k * t) % H
        X += _q16(s * int(D[h, 0]))
        Y += _q16(s * int(D[h, 1]))
        out.append((X, Y, h, x0 + (X >> 16), y0 + (Y >> 16)))
    return out


def sample(keys, wi, pose, s, t, T, body=(), weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0):
    """one sample by the letter of the rule: (why, score or DRIVE_NONE, (end_cell, d_end, d_nose, cost) or None)"""
    D = table()
    Hh, W = keys.shape
    x0, y0 = int(pose[0]), int(pose[1])

    def w_at(x, y):
        return int(wi[y, x]) if 0 <= x < W and 0 <= y < Hh else None

    tr = trajectory(pose, s, t, T)
    cost = 0
    for k in range(1, T + 1):
        X, Y, h, x, y = tr[k]
        px, py = tr[k - 1][3], tr[k - 1][4]
        cx, cy = int(D[h, 0]), int(D[h, 1])
        w = w_at(x, y)
        if w is None:
            return (1 << 12) | k, DRIVE_NONE, None
        if w == 0:
            return (2 << 12) | k, DRIVE_NONE, None
        if x != px and y != py and (not w_at(px, y) or not w_at(x, py)):
            return (3 << 12) | k, DRIVE_NONE, None
        for bx, by in body:
            ux, uy = X + _q16(bx * cx - by * cy), Y + _q16(bx * cy + by * cx)
            if not w_at(x0 + (ux >> 16), y0 + (uy >> 16)):
                return (4 << 12) | k, DRIVE_NONE, None
        cost += w
    X, Y, h, x, y = tr[T]
    if int(keys[y, x]) == NONE:
        return (5 << 12) | T, DRIVE_NONE, None
    d_end = int(keys[y, x]) >> 4
    nx, ny = x0 + ((X + _q16(nose_q16 * int(D[h, 0]))) >> 16), y0 + ((Y + _q16(nose_q16 * int(D[h, 1]))) >> 16)
    d_nose = d_end + nose_miss
    if 0 <= nx < W and 0 <= ny < Hh and int(keys[ny, nx]) != NONE:
        d_nose = int(keys[ny, nx]) >> 4
    a_end, a_nose, a_cost, a_turn = weights
    return 0, a_end * d_end + a_nose * d_nose + a_cost * cost + a_turn * abs(t), (y * W + x, d_end, d_nose, cost)


def rollout(keys, wi, pose, steps, step_q16, turn, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0):
    """all samples of one pose on one key image: (choice: one CHOICE_DTYPE record, scores uint64 (V, Wn), why uint16 (V, Wn))"""
    D = table()
    Hh, W = keys.shape
    wi = np.asarray(wi, dtype=np.int64)
    x0, y0, fx, fy, h0 = (int(v) for v in pose[:5])
    s = np.asarray(step_q16, dtype=np.int64).reshape(-1, 1)
    t = np.asarray(turn, dtype=np.int64).reshape(1, -1)
    V, Wn = s.shape[0], t.shape[1]
    body = np.zeros((0, 2), dtype=np.int64) if body is None else np.asarray(body, dtype=np.int64).reshape(-1, 2)

    def w_at(x, y):
        """w of the cells, 0 outside the map; and where they lie inside"""
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < Hh)
        w = np.zeros(x.shape, dtype=np.int64)
        w[inside] = wi[y[inside], x[inside]]
        return w, inside

    X, Y = np.full((V, Wn), fx, dtype=np.int64), np.full((V, Wn), fy, dtype=np.int64)
    px, py = np.full((V, Wn), x0, dtype=np.int64), np.full((V, Wn), y0, dtype=np.int64)
    why, alive, cost = np.zeros((V, Wn), dtype=np.int64), np.ones((V, Wn), dtype=bool), np.zeros((V, Wn), dtype=np.int64)
    h = np.zeros((1, Wn), dtype=np.int64)
    for k in range(1, steps + 1):
        h = (h0 + k * t) % H
        cx, cy = D[h, 0], D[h, 1]                                      # (1, Wn)
        X = X + _q16(s * cx)
        Y = Y + _q16(s * cy)
        x, y = x0 + (X >> 16), y0 + (Y >> 16)
        w, inside = w_at(x, y)
        reason = np.where(~inside, 1, np.where(w == 0, 2, 0))
        cut = (x != px) & (y != py) & ((w_at(px, y)[0] == 0) | (w_at(x, py)[0] == 0))
        reason = np.where((reason == 0) & cut, 3, reason)
        if body.shape[0]:
            bx, by = body[:, 0].reshape(1, 1, -1), body[:, 1].reshape(1, 1, -1)
            ux = X[..., None] + _q16(bx * cx[..., None] - by * cy[..., None])
            uy = Y[..., None] + _q16(bx * cy[..., None] + by * cx[..., None])
            hit = (w_at(x0 + (ux >> 16), y0 + (uy >> 16))[0] == 0).any(axis=-1)
            reason = np.where((reason == 0) & hit, 4, reason)
        new = alive & (reason != 0)
        why[new] = ((reason << 12) | k)[new]
        alive &= reason == 0
        cost += np.where(alive, w, 0)
        px, py = x, y
    xe, ye = np.where(alive, px, 0), np.where(alive, py, 0)
    ke = keys[ye, xe].astype(np.int64)
    new = alive & (ke == NONE)
    why[new] = (5 << 12) | steps
    alive &= ke != NONE
    d_end = ke >> 4
    cx, cy = D[h, 0], D[h, 1]
    nx, ny = x0 + ((X + _q16(nose_q16 * cx)) >> 16), y0 + ((Y + _q16(nose_q16 * cy)) >> 16)
    inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < Hh)
    kn = np.full((V, Wn), NONE, dtype=np.int64)
    kn[inside] = keys[ny[inside], nx[inside]]
    d_nose = np.where(kn != NONE, kn >> 4, d_end + nose_miss)
    a_end, a_nose, a_cost, a_turn = (int(v) for v in weights)
    score = a_end * d_end + a_nose * d_nose + a_cost * cost + a_turn * np.abs(t)
    scores = np.where(alive, score, 0).astype(np.uint64)
    scores[~alive] = DRIVE_NONE
    choice = np.zeros(1, dtype=CHOICE_DTYPE)
    if alive.any():
        idx = np.arange(V * Wn, dtype=np.int64).reshape(V, Wn)
        best = int(((score << 16) | idx)[alive].min()) & 0xFFFF
        i, j = best // Wn, best % Wn
        choice[0] = (i, j, int(alive.sum()), int(ye[i, j]) * W + int(xe[i, j]), int(d_end[i, j]), int(d_nose[i, j]), int(cost[i, j]), 0,
                     int(score[i, j]))
    else:
        choice[0] = (-1, -1, 0, NONE, NONE, NONE, 0, 0, DRIVE_NONE)
    return choice[0], scores, why.astype(np.uint16)


def rollout_all(keys, wi, poses, steps, step_q16, turn, **kw):
    """tsd_drive_rollout (keys (H, W); the poses' layers are ignored) or tsd_drive_fields_rollout (keys (L, H, W)): (choice [n],
    scores (n, V, Wn), why (n, V, Wn))"""
    out = [rollout(keys if keys.ndim == 2 else keys[int(p[5])], wi, p, steps, step_q16, turn, **kw) for p in poses]
    return np.array([o[0] for o in out], dtype=CHOICE_DTYPE), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def turns(n):
    """0, then by ascending magnitude: 0, 1, -1, 2, -2, ... n, -n"""
    return [0] + [v for m in range(1, n + 1) for v in (m, -m)]


# ---- the maps
def door_map():
    """96 x 64, a wall down column 48 with a doorway of four cells at y = 30 .. 33, and the goal behind it"""
    m = np.zeros((64, 96), dtype=np.int8)
    m[:, 48] = RR.O
    m[30:34, 48] = 0
    return m, (80, 12)


def cases():
    """{name: dict(map, wi, keys (H, W) of a route call, goals -- its seeds --, fields (L, H, W) of a fields call with the same seeds)}:
    the goal fields are the restatements' (route_ref, route_fields_ref), computed once"""
    out = {}

    def add(name, m, goals, free_max=0, w=None, limit=0):
        keys, _ = RR.route(m, goals, free_max, w, limit)
        layers, _ = RF.fields(m, goals, free_max, w, limit)
        for a in (keys, layers):
            a.setflags(write=False)
        out[name] = dict(map=m, wi=RR.weight_image(m, free_max, w), keys=keys, fields=layers, goals=list(goals), free_max=free_max, w=w, limit=limit)

    m, goal = door_map()
    add("door_96x64", m, [goal, (10, 50)])
    add("open_45x37", np.zeros((37, 45), dtype=np.int8), [(40, 30), (2, 3), (-1, -1)])
    add("limited_45x37", np.zeros((37, 45), dtype=np.int8), [(40, 30)], limit=60)
    add("random_67x50", RR.random_map(67, 50, 0.08, 4711), [(60, 40), (5, 5), (33, 25)], free_max=50, w=RR.random_weights(12))
    return out


# ---- the closed loop: a robot that faces away from its way turns, drives through the door and arrives
LOOP = dict(steps=12, step_q16=[65536, 32768, 16384, 4096, 0], turn=turns(6), body=[(65536, 0), (-65536, 0), (0, 65536), (0, -65536)],
            weights=(1, 1, 0, 0), nose_q16=3 * 65536, nose_miss=200)
LOOP_TURN_UNIT = 16                                                    # the loop's turn list is turns(6) in units of 16 headings
LOOP_START = (20, 50, 32768, 32768, H // 2, 0)                         # left of the wall, looking along -x: away from the door
LOOP_ARRIVED = 3 * 5


def loop_params():
    p = dict(LOOP)
    p["turn"] = [LOOP_TURN_UNIT * t for t in LOOP["turn"]]
    return p


def closed_loop(roll, step, max_commands, keys, wi):
    """roll(pose) -> (choice, scores, why) of one pose; step(pose, step_q16, turn) -> the pose one step on.  Applies the first step
    of every choice until the robot stands on a cell with d <= LOOP_ARRIVED: the list of (pose, speed index, turn index), the poses
    visited.  Asserts the rule's promises on the way."""
    p = loop_params()
    pose, log = tuple(LOOP_START), []
    while True:
        assert wi[pose[1], pose[0]] > 0, ("the robot stands on a cell that is not traversable", pose, len(log))
        k = int(keys[pose[1], pose[0]])
        if k != NONE and (k >> 4) <= LOOP_ARRIVED:
            return log
        assert len(log) < max_commands, ("the robot did not arrive", pose, len(log))
        choice, _, why = roll(pose)
        assert choice["admissible"] > 0 and choice["speed"] >= 0, (pose, len(log))
        assert why[choice["speed"], choice["turn"]] == 0, "the chosen sample is refused at some step"
        log.append((pose, int(choice["speed"]), int(choice["turn"])))
        pose = tuple(int(v) for v in step(pose, p["step_q16"][choice["speed"]], p["turn"][choice["turn"]]))[:5] + (0,)
