"""The fleet rule of include/tsd_hip.h (tsd_drive_fleet_rollout) restated on top of tests/drive_ref.py: the robots decide one after
the other in the order of their ranks, each one against the chosen arcs of those decided before it (the parked robots first of all).
Everything is int64 (Python integers in ``sample``).  ``sample`` is the rule for one sample, step by step, on drive_ref.sample and
drive_ref.trajectory; ``rollout`` is the same rule for all samples of all robots (numpy over the samples and the steps), which is
what the tests compare the device against; ``violations`` is the rule read backwards: the steps at which two finished tracks break
it."""
import numpy as np

from tests import drive_ref as DR

H = DR.H
NONE = DR.NONE
DRIVE_NONE = DR.DRIVE_NONE
FAR = 1 << 62                                                          # "far": larger than any D, 2 sep^2 < 2^47
SEP_MAX = 128 * 65536


def absolute(pose, tr):
    """the absolute Q16 positions [(x0 << 16) + X_k, (y0 << 16) + Y_k] of a drive_ref.trajectory of `pose`"""
    x0, y0 = int(pose[0]), int(pose[1])
    return [((x0 << 16) + c[0], (y0 << 16) + c[1]) for c in tr]


def standing(pose, T):
    """the track of a robot that is parked or found no admissible sample: its pose in every slot, int64 (T + 1, 2)"""
    x0, y0, fx, fy = (int(v) for v in pose[:4])
    return np.tile(np.array([[(x0 << 16) + fx, (y0 << 16) + fy]], dtype=np.int64), (T + 1, 1))


def dist(p, q, sep):
    """D of two positions: dx^2 + dy^2 where |dx| < sep and |dy| < sep, else FAR"""
    dx, dy = int(p[0]) - int(q[0]), int(p[1]) - int(q[1])
    return dx * dx + dy * dy if abs(dx) < sep and abs(dy) < sep else FAR


def conflict(P, Q, k, sep):
    """reason 6 of the track P against the track Q at step k >= 1"""
    d = dist(P[k], Q[k], sep)
    return d != FAR and d < sep * sep and d <= dist(P[k - 1], Q[k - 1], sep)


def sample(keys, wi, pose, s, t, T, others, sep, **kw):
    """one sample by the letter of the rule against the tracks `others` of the robots decided before: (why, score or DRIVE_NONE,
    record or None) as drive_ref.sample"""
    why, score, rec = DR.sample(keys, wi, pose, s, t, T, **kw)
    first = why & 0xFFF if 1 <= why >> 12 <= 4 else T + 1            # the map's first refusal; reason 5 stays behind step T
    P = absolute(pose, DR.trajectory(pose, s, t, T))
    for k in range(1, min(first - 1, T) + 1):                        # at the map's own step the map's reason goes first
        if any(conflict(P, Q, k, sep) for Q in others):
            return (6 << 12) | k, DRIVE_NONE, None
    return why, score, rec


def _tracks(pose, step_q16, turn, T):
    """the absolute positions of all samples of a pose: int64 (V, Wn, T + 1, 2)"""
    D = DR.table()
    x0, y0, fx, fy, h0 = (int(v) for v in pose[:5])
    s = np.asarray(step_q16, dtype=np.int64).reshape(-1, 1, 1)
    t = np.asarray(turn, dtype=np.int64).reshape(-1, 1)
    h = (h0 + np.arange(1, T + 1, dtype=np.int64).reshape(1, -1) * t) % H                     # (Wn, T)
    out = np.zeros((s.shape[0], t.shape[0], T + 1, 2), dtype=np.int64)
    for a, f, c0 in ((0, fx, x0), (1, fy, y0)):
        out[:, :, 0, a] = (c0 << 16) + f
        out[:, :, 1:, a] = (c0 << 16) + f + np.cumsum((s * D[h, a][None] + 32768) >> 16, axis=2)
    return out


def first_conflict(P, others, sep):
    """P int64 (..., T + 1, 2) against each track of `others` (T + 1, 2): the smallest k at which reason 6 holds, T + 1 without one"""
    T = P.shape[-2] - 1
    hit = np.zeros(P.shape[:-2] + (T,), dtype=bool)
    for Q in others:
        d = P - np.asarray(Q, dtype=np.int64)
        near = (np.abs(d[..., 0]) < sep) & (np.abs(d[..., 1]) < sep)
        Dk = np.where(near, d[..., 0] ** 2 + d[..., 1] ** 2, FAR)
        hit |= near[..., 1:] & (Dk[..., 1:] < sep * sep) & (Dk[..., 1:] <= Dk[..., :-1])
    k = np.where(hit.any(axis=-1), hit.argmax(axis=-1) + 1, T + 1)
    return k


def rollout(keys, wi, poses, steps, step_q16, turn, order, sep_q16, **kw):
    """tsd_drive_fleet_rollout on the key images keys (L, H, W): (choice [n], scores (n, V, Wn), why (n, V, Wn), tracks int64
    (n, T + 1, 2), blocked [n]: the samples refused by reason 6)"""
    n, T, sep = len(poses), int(steps), int(sep_q16)
    V, Wn = len(step_q16), len(turn)
    assert sorted(int(r) for r in order) == list(range(n)) and 0 <= sep <= SEP_MAX
    choice = np.zeros(n, dtype=DR.CHOICE_DTYPE)
    scores = np.full((n, V, Wn), DRIVE_NONE, dtype=np.uint64)
    why = np.zeros((n, V, Wn), dtype=np.uint16)
    tracks = np.stack([standing(p, T) for p in poses])
    blocked = np.zeros(n, dtype=np.int64)
    none = (-1, -1, 0, NONE, NONE, NONE, 0, 0, DRIVE_NONE)
    parked = [r for r in range(n) if int(poses[r][5]) == -1]
    for r in parked:
        choice[r] = none
    decided = list(parked)
    sample_kw = {k: v for k, v in kw.items() if k != "body"}
    body = [tuple(int(c) for c in b) for b in np.asarray(kw.get("body") if kw.get("body") is not None else [], dtype=np.int64).reshape(-1, 2)]
    for r in (int(r) for r in order):
        if r in parked:
            continue
        pose = poses[r]
        layer = keys if keys.ndim == 2 else keys[int(pose[5])]
        _, sc, wm = DR.rollout(layer, wi, pose, T, step_q16, turn, **kw)
        wm = wm.astype(np.int64)
        first = np.where((wm >> 12 >= 1) & (wm >> 12 <= 4), wm & 0xFFF, T + 1)
        P = _tracks(pose, step_q16, turn, T)
        kc = first_conflict(P, [tracks[q] for q in decided], sep)
        six = kc < first
        why[r] = np.where(six, (6 << 12) | kc, wm).astype(np.uint16)
        scores[r] = np.where(six, np.uint64(DRIVE_NONE), sc)
        blocked[r] = int(six.sum())
        alive = why[r] == 0
        if alive.any():
            idx = np.arange(V * Wn, dtype=np.int64).reshape(V, Wn)
            best = int(((scores[r].astype(np.int64) << 16) | idx)[alive].min()) & 0xFFFF
            i, j = best // Wn, best % Wn
            w, score, rec = DR.sample(layer, wi, pose, int(step_q16[i]), int(turn[j]), T, body=body, **sample_kw)
            assert w == 0 and score == int(scores[r, i, j])
            choice[r] = (i, j, int(alive.sum())) + rec + (0, score)
            tracks[r] = P[i, j]
        else:
            choice[r] = none
        decided.append(r)
    return choice, scores, why, tracks, blocked


def violations(tracks, sep_q16, pairs=None):
    """[(q, r, k)]: the steps k >= 1 at which the finished tracks of the robots q < r break the rule (closer than sep and not moving
    apart)"""
    n, sep = len(tracks), int(sep_q16)
    out = []
    for q in range(n):
        for r in range(q + 1, n):
            if pairs is not None and (q, r) not in pairs:
                continue
            out += [(q, r, k) for k in range(1, len(tracks[r])) if conflict(tracks[r], tracks[q], k, sep)]
    return out


def track_of(pose, choice, step_q16, turn, T):
    """the track of a drive_ref choice record: the chosen arc, or the pose in every slot"""
    if int(choice["speed"]) < 0:
        return standing(pose, T)
    return np.array(absolute(pose, DR.trajectory(pose, int(step_q16[int(choice["speed"])]), int(turn[int(choice["turn"])]), T)), dtype=np.int64)
