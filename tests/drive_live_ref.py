"""The live layer of include/tsd_hip.h (tsd_drive_live_set and reason 7 of the three rollouts) restated on top of tests/drive_ref.py
and tests/drive_fleet_ref.py, written from the rule and not from the kernels.  Everything is int64 or Python integers.  ``stamp`` is
the layer in numpy over the points and the rows of their discs (the half-width of a row from math.isqrt, a difference image per
row); ``stamp_slow`` is the rule's inequality point by point and cell by cell.  ``sample`` is reason 7 for one sample, step by step,
on drive_ref.sample; ``rollout`` is the same for all samples of a pose (numpy over the samples and the body points), which is what
the tests compare the device against; ``fleet_sample`` and ``fleet_rollout`` put reason 6 behind it as drive_fleet_ref does."""
import math

import numpy as np

from tests import drive_fleet_ref as FR
from tests import drive_ref as DR

H = DR.H
NONE = DR.NONE
DRIVE_NONE = DR.DRIVE_NONE
MAX_POINTS, MAX_SKIP, MAX_RADIUS = 32768, 16, 64
MAX_COORD, MAX_SKIP_RADIUS = 1 << 30, 1 << 15


# ---- the layer
def _points(points):
    return np.asarray(points if points is not None else [], dtype=np.int64).reshape(-1, 2)


def _discs(skip):
    return np.asarray(skip if skip is not None else [], dtype=np.int64).reshape(-1, 3)


def kept(points, skip=None):
    """bool per point: it lies in no skip disc (a point on a disc's rim is dropped)"""
    p = _points(points)
    keep = np.ones(p.shape[0], dtype=bool)
    for ox, oy, ro in _discs(skip):
        keep &= (p[:, 0] - ox) ** 2 + (p[:, 1] - oy) ** 2 > ro * ro
    return keep


def stamp(points, radius, width, height, skip=None):
    """(the live set as bool (height, width), the number of points not dropped)"""
    p = _points(points)
    keep = kept(p, skip)
    p, r = p[keep], int(radius)
    assert 0 <= r <= MAX_RADIUS and p.shape[0] <= MAX_POINTS and len(_discs(skip)) <= MAX_SKIP
    edge = np.zeros((height, width + 1), dtype=np.int64)              # +1 where a span begins, -1 behind its end
    for dy in range(-r, r + 1):
        hw = math.isqrt(r * r - dy * dy)
        y, x0, x1 = p[:, 1] + dy, np.maximum(p[:, 0] - hw, 0), np.minimum(p[:, 0] + hw, width - 1)
        ok = (y >= 0) & (y < height) & (x0 <= x1)
        np.add.at(edge, (y[ok], x0[ok]), 1)
        np.add.at(edge, (y[ok], x1[ok] + 1), -1)
    return np.cumsum(edge, axis=1)[:, :width] > 0, int(keep.sum())


def stamp_slow(points, radius, width, height, skip=None):
    """the same by the letter of the rule: every point against every disc, every cell of the map near it against the inequality"""
    img, n, r = np.zeros((height, width), dtype=bool), 0, int(radius)
    for px, py in ((int(a), int(b)) for a, b in _points(points)):
        if any((px - int(ox)) ** 2 + (py - int(oy)) ** 2 <= int(ro) ** 2 for ox, oy, ro in _discs(skip)):
            continue
        n += 1
        for y in range(max(py - r - 1, 0), min(py + r + 2, height)):
            for x in range(max(px - r - 1, 0), min(px + r + 2, width)):
                if (x - px) ** 2 + (y - py) ** 2 <= r * r:
                    img[y, x] = True
    return img, n


def stride_words(width):
    return (width + 31) // 32


def pack(img):
    """the bit image: uint32 (height, stride_words), bit x & 31 of word x >> 5; the tail bits 0"""
    Hh, W = img.shape
    bits = np.zeros((Hh, stride_words(W) * 32), dtype=np.uint8)
    bits[:, :W] = img
    return np.packbits(bits.reshape(Hh, -1, 32), axis=-1, bitorder="little").reshape(Hh, -1, 4).copy().view("<u4").reshape(Hh, -1)


def unpack(words, width):
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=-1, bitorder="little")[:, :width].astype(bool)


# ---- the shapes the CPU and the GPU tests share
# (width, height): one cell, below / at / above a word, several words with a tail, and a long row
STAMP_MAPS = [(1, 1), (31, 5), (32, 32), (33, 7), (97, 64), (4096, 64)]


def stamp_points(W, Hh, r):
    """the corners, the word edges, points outside the map by less than r, by r and by r + 1, far points, duplicates"""
    pts = [(0, 0), (W - 1, 0), (0, Hh - 1), (W - 1, Hh - 1), (W - 1, Hh // 2), (W - 1, Hh // 2)]
    pts += [(x, Hh // 3) for x in (31, 32, 63, 64) if x < W + r]
    pts += [(-r + 1, 2), (-r, Hh // 2), (-r - 1, 1), (W - 1 + r, 0), (W + r, Hh - 1), (W // 2, -r), (W // 2, -r - 1), (W // 3, Hh - 1 + r), (W // 3, Hh + r)]
    pts += [(1 << 30, 0), (-(1 << 30), Hh - 1), (0, 1 << 30), (W - 1, -(1 << 30)), (1 << 30, -(1 << 30))]
    return pts


# ---- reason 7
def _in(live, x, y):
    return 0 <= x < live.shape[1] and 0 <= y < live.shape[0] and bool(live[y, x])


def sample(keys, wi, live, pose, s, t, T, body=(), **kw):
    """one sample by the letter of the rule: drive_ref.sample, and reason 7 at every step before the map's first refusal (at the
    map's own step 1 .. 4 go first; reason 5 stays behind step T).  ``live`` None: no layer"""
    why, score, rec = DR.sample(keys, wi, pose, s, t, T, body=body, **kw)
    if live is None:
        return why, score, rec
    D = DR.table()
    x0, y0 = int(pose[0]), int(pose[1])
    first = why & 0xFFF if 1 <= why >> 12 <= 4 else T + 1
    tr = DR.trajectory(pose, s, t, T)
    for k in range(1, min(first - 1, T) + 1):
        X, Y, h, x, y = tr[k]
        cx, cy = int(D[h, 0]), int(D[h, 1])
        hit = _in(live, x, y)
        for bx, by in body:
            ux, uy = X + DR._q16(bx * cx - by * cy), Y + DR._q16(bx * cy + by * cx)
            hit = hit or _in(live, x0 + (ux >> 16), y0 + (uy >> 16))
        if hit:
            return (7 << 12) | k, DRIVE_NONE, None
    return why, score, rec


def first_live(live, pose, steps, step_q16, turn, body=None):
    """int64 (V, Wn): the smallest k in 1 .. steps at which the centre cell or a body point's cell lies in the live set, steps + 1
    without one (a cell outside the map is in no live set)"""
    D = DR.table()
    Hh, W = live.shape
    x0, y0, fx, fy, h0 = (int(v) for v in pose[:5])
    s = np.asarray(step_q16, dtype=np.int64).reshape(-1, 1)
    t = np.asarray(turn, dtype=np.int64).reshape(1, -1)
    V, Wn = s.shape[0], t.shape[1]
    body = np.zeros((0, 2), dtype=np.int64) if body is None else np.asarray(body, dtype=np.int64).reshape(-1, 2)

    def at(x, y):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < Hh)
        out = np.zeros(x.shape, dtype=bool)
        out[inside] = live[y[inside], x[inside]]
        return out

    X, Y = np.full((V, Wn), fx, dtype=np.int64), np.full((V, Wn), fy, dtype=np.int64)
    k7 = np.full((V, Wn), steps + 1, dtype=np.int64)
    for k in range(1, steps + 1):
        h = (h0 + k * t) % H
        cx, cy = D[h, 0], D[h, 1]
        X = X + DR._q16(s * cx)
        Y = Y + DR._q16(s * cy)
        hit = at(x0 + (X >> 16), y0 + (Y >> 16))
        if body.shape[0]:
            bx, by = body[:, 0].reshape(1, 1, -1), body[:, 1].reshape(1, 1, -1)
            ux = X[..., None] + DR._q16(bx * cx[..., None] - by * cy[..., None])
            uy = Y[..., None] + DR._q16(bx * cy[..., None] + by * cx[..., None])
            hit = hit | at(x0 + (ux >> 16), y0 + (uy >> 16)).any(axis=-1)
        k7 = np.where(hit & (k7 > steps), k, k7)
    return k7


def _choose(keys, wi, pose, steps, step_q16, turn, scores, why, kw):
    """the choice record from the samples' final scores and `why`: the minimum of (score << 16) | index over the admissible ones"""
    V, Wn = why.shape
    alive = why == 0
    if not alive.any():
        return (-1, -1, 0, NONE, NONE, NONE, 0, 0, DRIVE_NONE)
    idx = np.arange(V * Wn, dtype=np.int64).reshape(V, Wn)
    best = int(((scores.astype(np.int64) << 16) | idx)[alive].min()) & 0xFFFF
    i, j = best // Wn, best % Wn
    body = [tuple(int(c) for c in b) for b in np.asarray(kw.get("body") if kw.get("body") is not None else [], dtype=np.int64).reshape(-1, 2)]
    w, score, rec = DR.sample(keys, wi, pose, int(step_q16[i]), int(turn[j]), steps, body=body, **{k: v for k, v in kw.items() if k != "body"})
    assert w == 0 and score == int(scores[i, j])
    return (i, j, int(alive.sum())) + rec + (0, score)


def rollout(keys, wi, live, pose, steps, step_q16, turn, **kw):
    """all samples of one pose on one key image with the layer ``live`` (bool (H, W), or None: no layer): (choice, scores, why) as
    drive_ref.rollout"""
    choice, scores, why = DR.rollout(keys, wi, pose, steps, step_q16, turn, **kw)
    if live is None:
        return choice, scores, why
    assert live.shape == keys.shape
    wm = why.astype(np.int64)
    first = np.where((wm >> 12 >= 1) & (wm >> 12 <= 4), wm & 0xFFF, steps + 1)
    k7 = first_live(live, pose, steps, step_q16, turn, kw.get("body"))
    seven = k7 < first
    why = np.where(seven, (7 << 12) | k7, wm).astype(np.uint16)
    scores = np.where(seven, np.uint64(DRIVE_NONE), scores)
    out = np.zeros(1, dtype=DR.CHOICE_DTYPE)
    out[0] = _choose(keys, wi, pose, steps, step_q16, turn, scores, why, kw)
    return out[0], scores, why


def rollout_all(keys, wi, live, poses, steps, step_q16, turn, **kw):
    """tsd_drive_rollout (keys (H, W)) or tsd_drive_fields_rollout (keys (L, H, W)) with a layer: (choice [n], scores, why (n, V, Wn))"""
    out = [rollout(keys if keys.ndim == 2 else keys[int(p[5])], wi, live, p, steps, step_q16, turn, **kw) for p in poses]
    return np.array([o[0] for o in out], dtype=DR.CHOICE_DTYPE), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def blocked_live(why):
    """the samples refused by reason 7, over the last two axes"""
    return (np.asarray(why) >> 12 == 7).sum(axis=(-2, -1))


# ---- the fleet form: at one step 1, 2, 3, 4, 7, 6
def fleet_sample(keys, wi, live, pose, s, t, T, others, sep, **kw):
    """drive_fleet_ref.sample with the layer: reason 6 at every step before the first refusal by 1 .. 4 or 7"""
    why, score, rec = sample(keys, wi, live, pose, s, t, T, **kw)
    first = why & 0xFFF if why >> 12 in (1, 2, 3, 4, 7) else T + 1
    P = FR.absolute(pose, DR.trajectory(pose, s, t, T))
    for k in range(1, min(first - 1, T) + 1):
        if any(FR.conflict(P, Q, k, sep) for Q in others):
            return (6 << 12) | k, DRIVE_NONE, None
    return why, score, rec


def fleet_rollout(keys, wi, live, poses, steps, step_q16, turn, order, sep_q16, **kw):
    """tsd_drive_fleet_rollout with the layer ``live`` (None: drive_fleet_ref.rollout itself): (choice [n], scores, why (n, V, Wn),
    tracks int64 (n, T + 1, 2), blocked [n]: the samples refused by reason 6)"""
    if live is None:
        return FR.rollout(keys, wi, poses, steps, step_q16, turn, order, sep_q16, **kw)
    n, T, sep = len(poses), int(steps), int(sep_q16)
    V, Wn = len(step_q16), len(turn)
    assert sorted(int(r) for r in order) == list(range(n)) and 0 <= sep <= FR.SEP_MAX
    choice = np.zeros(n, dtype=DR.CHOICE_DTYPE)
    scores = np.full((n, V, Wn), DRIVE_NONE, dtype=np.uint64)
    why = np.zeros((n, V, Wn), dtype=np.uint16)
    tracks = np.stack([FR.standing(p, T) for p in poses])
    blocked = np.zeros(n, dtype=np.int64)
    parked = [r for r in range(n) if int(poses[r][5]) == -1]
    for r in parked:
        choice[r] = (-1, -1, 0, NONE, NONE, NONE, 0, 0, DRIVE_NONE)
    decided = list(parked)
    for r in (int(r) for r in order):
        if r in parked:
            continue
        pose = poses[r]
        layer = keys if keys.ndim == 2 else keys[int(pose[5])]
        _, sc, wm = rollout(layer, wi, live, pose, T, step_q16, turn, **kw)
        wm = wm.astype(np.int64)
        reason = wm >> 12
        first = np.where(((reason >= 1) & (reason <= 4)) | (reason == 7), wm & 0xFFF, T + 1)
        P = FR._tracks(pose, step_q16, turn, T)
        kc = FR.first_conflict(P, [tracks[q] for q in decided], sep)
        six = kc < first
        why[r] = np.where(six, (6 << 12) | kc, wm).astype(np.uint16)
        scores[r] = np.where(six, np.uint64(DRIVE_NONE), sc)
        blocked[r] = int(six.sum())
        choice[r] = _choose(layer, wi, pose, T, step_q16, turn, scores[r], why[r], kw)
        if choice[r]["speed"] >= 0:
            tracks[r] = P[int(choice[r]["speed"]), int(choice[r]["turn"])]
        decided.append(r)
    return choice, scores, why, tracks, blocked
