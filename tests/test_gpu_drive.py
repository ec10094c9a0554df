"""The rollout on the device (csrc/drive.hip; tsd_drive_rollout, tsd_drive_fields_rollout) against the restatement of
tests/drive_ref.py: every comparison is byte for byte -- the choice records, the scores and `why` of every sample, and the words of
sentinel-filled outputs the call must not write.  The goal fields are the device's own route and fields results of the maps of
drive_ref.cases(), which the restatements of the routes give as well."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import drive_ref as DR
from tests import route_ref as RR

pytestmark = pytest.mark.gpu

H = DR.H
S64, S16, TAIL = 0xA5A5A5A5A5A5A5A5, 0xA5A5, 8


@pytest.fixture(scope="module")
def grid():
    g = capi.TsdGridDevice(8, 0.1, 0.3)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cases():
    return DR.cases()


def _load(grid, c, route=True, fields=True):
    """the route and the fields result of case c on the context, seeded at the case's goals; both must be the restatements'"""
    m = c["map"]
    Hh, W = m.shape
    stride = W + 3
    padded = np.full((Hh, stride), -1, dtype=np.int8)
    padded[:, :W] = m
    buf = capi.DeviceBuffer(grid, padded.size)
    buf.upload(padded)
    try:
        kw = dict(seeds=c["goals"], free_max=c["free_max"], weights=c["w"], limit=c["limit"])
        if route:
            assert np.array_equal(grid.route_of(buf.ptr, W, Hh, stride, **kw)[0], c["keys"])
        if fields:
            assert np.array_equal(grid.route_fields_of(buf.ptr, W, Hh, stride, **kw)[0], c["fields"])
    finally:
        buf.free()


def _raw(grid, form, poses, steps, step_q16, turn, body=None, weights=(1, 1, 0, 0), nose_q16=0, nose_miss=0, scores=True, why=True):
    """one call into sentinel-filled outputs: (rc, choice, scores, why), the last two with TAIL words behind the call's own"""
    prm, keep = grid._drive_params(steps, step_q16, turn, body, weights, nose_q16, nose_miss)
    p = capi.drive_poses(poses)
    n = p.size * prm.n_speeds * prm.n_turns
    choice = np.frombuffer(bytes([0xA5]) * (40 * p.size), dtype=capi.DRIVE_CHOICE_DTYPE).copy()
    sc, wh = np.full(n + TAIL, S64, dtype=np.uint64), np.full(n + TAIL, S16, dtype=np.uint16)
    fn = grid.lib.tsd_drive_rollout if form == "route" else grid.lib.tsd_drive_fields_rollout
    rc = fn(grid.h, C.byref(prm), p.ctypes.data, int(p.size), choice.ctypes.data, sc.ctypes.data if scores else None, wh.ctypes.data if why else None)
    return rc, choice, sc, wh


def _check(grid, c, form, poses, steps, step_q16, turn, what="", **kw):
    keys = c["keys"] if form == "route" else c["fields"]
    want = DR.rollout_all(keys, c["wi"], poses, steps, step_q16, turn, **kw)
    rc, choice, sc, wh = _raw(grid, form, poses, steps, step_q16, turn, **kw)
    n = want[1].size
    assert rc == 0, (what, grid.lib.tsd_last_error(grid.h))
    assert wh[:n].tobytes() == want[2].tobytes(), (what, "why", np.argwhere(wh[:n].reshape(want[2].shape) != want[2])[:4])
    assert sc[:n].tobytes() == want[1].tobytes(), (what, "scores", np.argwhere(sc[:n].reshape(want[1].shape) != want[1])[:4])
    assert choice.tobytes() == want[0].tobytes(), (what, choice, want[0])
    assert (sc[n:] == S64).all() and (wh[n:] == S16).all(), (what, "words beyond the samples were written")
    return want


def _free_cells(c, n, seed):
    ys, xs = np.nonzero(c["wi"] > 0)
    pick = np.random.default_rng(seed).choice(xs.size, size=n, replace=False)
    return [(int(xs[i]), int(ys[i])) for i in pick]


def _poses(c, layers=1):
    """the border heading out and along it, the far corner, offsets of 65535, the headings H - 1 and 0, and seeded free cells"""
    Hh, W = c["wi"].shape
    out = [(0, Hh // 2, 100, 100, H // 2), (0, 3, 0, 30000, H // 4), (W - 1, Hh - 1, 65535, 65535, 0), (W - 1, 2, 65535, 0, 3 * H // 4)]
    for k, (x, y) in enumerate(_free_cells(c, 4, 99)):
        out.append((x, y, 65535, 65535, (H - 1, 0, 700 * k + 13, H // 8)[k]))
    return [p + (k % layers,) for k, p in enumerate(out)]


def _body(B, radius_q16=98304):
    """B points on rings round the centre, from the table: no trigonometry here either"""
    D = DR.table()
    return [((radius_q16 * (1 + b % 2) * int(D[(b * H) // max(B, 1), 0])) >> 16, (radius_q16 * (1 + b % 2) * int(D[(b * H) // max(B, 1), 1])) >> 16)
            for b in range(B)]


def _speeds(V):
    return [65536 - (65536 * i) // max(V - 1, 1) for i in range(V)] if V > 1 else [65536]


def _turns(Wn, unit):
    t = [unit * v for v in DR.turns(Wn // 2)]
    return t if len(t) == Wn else t + [H // 8]               # (an even count: one more, the largest turn)


# (T, B, V, Wn, the turns' unit): T at the wave's edges, B at its limits, one sample, the most samples, counts that are no multiple of 4 or 64
SHAPES = [(1, 0, 1, 1, 1), (63, 1, 3, 5, 8), (64, 63, 2, 3, 3), (65, 64, 2, 3, 5), (128, 0, 7, 9, 10), (256, 1, 3, 5, 2), (65, 1, 64, 129, 8),
          (256, 64, 1, 2, 512), (20, 4, 5, 13, 40)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_B%d_V%d_W%d" % s[:4])
@pytest.mark.parametrize("name,form", [("door_96x64", "route"), ("random_67x50", "fields"), ("open_45x37", "fields")])
def test_rollout_equals_the_restatement(grid, cases, name, form, shape):
    T, B, V, Wn, unit = shape
    c = cases[name]
    _load(grid, c, route=form == "route", fields=form == "fields")
    poses = _poses(c, 1 if form == "route" else c["fields"].shape[0])
    radius = 20000 if name.startswith("random") else 98304          # (in the clutter a wide body would refuse every sample)
    kw = dict(body=_body(B, radius) if B else None, weights=(3, 2, 1, 5), nose_q16=3 * 65536 + 77, nose_miss=123)
    want = _check(grid, c, form, poses, T, _speeds(V), _turns(Wn, unit), f"{name} {shape}", **kw)
    reasons = sorted(set((want[2] >> 12).ravel().tolist()))
    print(f"{name} {form} {shape}: reasons {reasons}, admissible {want[0]['admissible'].tolist()}")
    assert want[2][0, 0, 0] == (1 << 12) | 1 or V * Wn == 1 and T == 1          # the robot on the border heading out: outside at k = 1
    if name == "open_45x37":
        assert (want[2][2::3] >> 12 >= 1).all()             # layer 2 holds no key at all: reason 5 where nothing else refuses


def test_every_sample_refused(grid, cases):
    c = cases["limited_45x37"]
    _load(grid, c)
    poses = [(3, 3, 0, 0, 0, 0), (0, 20, 5, 5, H // 2, 0)]
    want = _check(grid, c, "route", poses, 5, [65536, 30000], [0, 4, -4], "no key / outside")
    assert (want[2][0] == (5 << 12) | 5).all() and (want[2][1] >> 12 == 1).all()
    assert (want[0]["speed"] == -1).all() and (want[0]["turn"] == -1).all() and (want[0]["score"] == DR.DRIVE_NONE).all()
    assert (want[0]["admissible"] == 0).all() and (want[1] == DR.DRIVE_NONE).all()


def _rows_map():
    """96 x 64, free but for single cells on the rows a robot at x = 2 drives along at one cell per step"""
    m = np.zeros((64, 96), dtype=np.int8)
    m[10, 66] = RR.O                                          # k = 64: the last lane of the first round
    m[20, 67] = RR.O                                          # k = 65: the first lane of the second
    m[30, 66] = m[30, 67] = RR.O                              # both
    m[40, 12] = m[40, 22] = RR.O                              # k = 10 and k = 20 in one round
    m[51, 7] = m[50, 11] = RR.O                               # a body point at k = 5 before the centre at k = 9
    m[58, 90] = RR.O                                          # k = 88, and the map's end at k = 94
    return dict(map=m, wi=RR.weight_image(m), keys=RR.route(m, [(94, 1)])[0], goals=[(94, 1)], free_max=0, w=None, limit=0)


def test_refusals_at_the_round_edges_the_smaller_step_wins(grid):
    c = _rows_map()
    _load(grid, c, fields=False)
    poses = [(2, y, 32768, 32768, 0, 0) for y in (10, 20, 30, 40, 50, 58, 5)]
    want = _check(grid, c, "route", poses, 100, [65536, 32768], [0], "rows", body=[(0, 65536)])
    assert want[2][:, 0, 0].tolist() == [(2 << 12) | 64, (2 << 12) | 65, (2 << 12) | 64, (2 << 12) | 10, (4 << 12) | 5, (2 << 12) | 88, (1 << 12) | 94]
    assert want[2][:2, 1, 0].tolist() == [0, 0] and want[2][3, 1, 0] == (2 << 12) | 19       # at half speed the cell x + 10 is entered at k = 19
    for T, why in ((63, [0, 0]), (64, [(2 << 12) | 64, 0]), (65, [(2 << 12) | 64, (2 << 12) | 65])):
        assert _check(grid, c, "route", poses[:2], T, [65536], [0], f"rows T {T}")[2].ravel().tolist() == why


def test_the_nose_outside_the_map_and_on_a_cell_without_a_key(grid, cases):
    c = cases["limited_45x37"]                                # keys only within 60 of (40, 30): 12 cells
    _load(grid, c)
    poses = [(43, 30, 32768, 32768, 0, 0),                    # the nose 3 cells ahead at x = 46: outside the map
             (31, 30, 32768, 32768, H // 2, 0),               # the nose at x = 28, d = 60: the last key ...
             (30, 30, 32768, 32768, H // 2, 0)]               # ... and at x = 27: a cell without one
    want = _check(grid, c, "route", poses, 4, [0], [0], "nose", weights=(1, 1, 0, 0), nose_q16=3 * 65536, nose_miss=1000)
    assert want[0]["d_end"].tolist() == [15, 45, 50] and want[0]["d_nose"].tolist() == [1015, 60, 1050]
    assert want[0]["score"].tolist() == [1030, 105, 1100]


def test_one_and_sixteen_robots_with_mixed_layers(grid, cases):
    c = cases["open_45x37"]                                   # goals (40, 30), (2, 3) and one outside the map: layer 2 is TSD_ROUTE_NONE only
    _load(grid, c)
    cells = _free_cells(c, 15, 5)
    poses = [(x, y, (977 * k) % 65536, (313 * k) % 65536, (257 * k) % H, k % 3) for k, (x, y) in enumerate(cells)]
    poses.append(poses[4][:5] + (0,))                         # two robots on one cell, pose and all, on two layers
    kw = dict(body=_body(5, 30000), weights=(2, 1, 1, 3), nose_q16=2 * 65536, nose_miss=50)
    prm = (20, _speeds(4), _turns(7, 30))
    all16 = _check(grid, c, "fields", poses, *prm, "16 robots", **kw)
    assert (all16[2][2::3] == (5 << 12) | 20).any() and (all16[2][2::3] != 0).all() and (all16[0]["speed"][2::3] == -1).all()
    assert (all16[0]["admissible"][0::3] > 0).all()
    for r in (0, 4, 7, 15):                                   # each robot equal to its own single call
        rc, choice, sc, wh = _raw(grid, "fields", [poses[r]], *prm, **kw)
        n = all16[1][r].size
        assert rc == 0 and choice[0].tobytes() == all16[0][r].tobytes()
        assert sc[:n].tobytes() == all16[1][r].tobytes() and wh[:n].tobytes() == all16[2][r].tobytes()
    # the route form beside the fields form on the same map: it ignores the poses' layers and reads the joint field
    both = _check(grid, c, "route", poses, *prm, "the route form", **kw)
    assert np.array_equal(c["keys"], c["fields"].min(axis=0)) and (both[0]["admissible"] > 0).all()
    _check(grid, c, "fields", poses, *prm, "the fields form again", **kw)


def test_a_repeated_call_allocates_nothing_and_null_outputs_change_nothing(grid, cases):
    c = cases["random_67x50"]
    _load(grid, c)
    poses = [p + (k % 3,) for k, p in enumerate(_poses(c))]
    args = (poses, 65, _speeds(9), _turns(21, 20))
    kw = dict(body=_body(7), weights=(1, 1, 1, 1), nose_q16=65536, nose_miss=9)
    first = _check(grid, c, "fields", *args, "first", **kw)
    block = grid.drive_dev_ptrs()
    for form in ("fields", "route", "fields"):
        _check(grid, c, form, *args, "again", **kw)
        assert grid.drive_dev_ptrs() == block                 # the same block at the same size: nothing was allocated
    _check(grid, c, "fields", poses[:2], 10, _speeds(2), [0], "a smaller call", **kw)
    assert grid.drive_dev_ptrs() == block
    tab = np.zeros((H, 2), dtype=np.int32)
    grid._check(grid.lib.tsd_dev_copy(grid.h, tab.ctypes.data, block[0], tab.nbytes, 0), "tsd_dev_copy")
    assert np.array_equal(tab, capi.drive_table())            # the table the kernel reads is the library's
    for scores, why in ((False, False), (True, False), (False, True)):
        rc, choice, sc, wh = _raw(grid, "fields", *args, scores=scores, why=why, **kw)
        assert rc == 0 and choice.tobytes() == first[0].tobytes()
        assert (sc == S64).all() if not scores else sc[:first[1].size].tobytes() == first[1].tobytes()
        assert (wh == S16).all() if not why else wh[:first[2].size].tobytes() == first[2].tobytes()
    assert grid.drive_rollout(poses, 65, _speeds(9), _turns(21, 20), **kw).tobytes() == DR.rollout_all(c["keys"], c["wi"], *args, **kw)[0].tobytes()
    ch, sc, wh = grid.drive_fields_rollout(poses, 65, _speeds(9), _turns(21, 20), want_scores=True, **kw)
    assert ch.tobytes() == first[0].tobytes() and np.array_equal(sc, first[1]) and np.array_equal(wh, first[2])


def test_refusals_leave_everything_in_place(grid, cases):
    c = cases["open_45x37"]
    _load(grid, c)
    lib, h = grid.lib, grid.h
    good = dict(poses=[(5, 5, 0, 0, 0, 1), (44, 36, 65535, 65535, H - 1, 2)], steps=8, step_q16=[65536, 0], turn=[0, 512, -512],
                body=[(64 * 65536, -64 * 65536)], weights=(255, 255, 255, 255), nose_q16=64 * 65536, nose_miss=RR.MAX_DIST)
    choice = np.frombuffer(bytes([0xA5]) * 80, dtype=capi.DRIVE_CHOICE_DTYPE).copy()
    sc, wh = np.full(12, S64, dtype=np.uint64), np.full(12, S16, dtype=np.uint16)

    def call(form="fields", n=None, null=(), raw=None, **over):
        a = dict(good, **over)
        prm, keep = grid._drive_params(a["steps"], a["step_q16"], a["turn"], a["body"], a["weights"], a["nose_q16"], a["nose_miss"])
        for field, value in (raw or {}).items():
            setattr(prm, field, value)
        p = capi.drive_poses(a["poses"])
        fn = lib.tsd_drive_rollout if form == "route" else lib.tsd_drive_fields_rollout
        return fn(h, None if "params" in null else C.byref(prm), None if "poses" in null else p.ctypes.data, p.size if n is None else n,
                  None if "choice" in null else choice.ctypes.data, sc.ctypes.data, wh.ctypes.data)

    pose = good["poses"][0]
    bad = [dict(null=("params",)), dict(null=("poses",)), dict(null=("choice",)), dict(n=0), dict(n=17), dict(steps=0), dict(steps=257),
           dict(raw=dict(n_speeds=0)), dict(raw=dict(n_speeds=65)), dict(raw=dict(n_turns=0)), dict(raw=dict(n_turns=130)), dict(raw=dict(n_body=-1)),
           dict(raw=dict(n_body=65)), dict(raw=dict(step_q16=None)), dict(raw=dict(turn=None)), dict(raw=dict(body_q16=None)),
           dict(step_q16=[65537]), dict(step_q16=[0, -1]), dict(turn=[0, 513]), dict(turn=[-513]), dict(body=[(64 * 65536 + 1, 0)]),
           dict(body=[(0, 0), (0, -64 * 65536 - 1)]), dict(weights=(256, 0, 0, 0)), dict(weights=(0, -1, 0, 0)), dict(weights=(0, 0, 256, 0)),
           dict(weights=(0, 0, 0, 256)), dict(nose_q16=-1), dict(nose_q16=64 * 65536 + 1), dict(nose_miss=RR.MAX_DIST + 1),
           dict(poses=[(45, 5, 0, 0, 0, 0)]), dict(poses=[(5, 37, 0, 0, 0, 0)]), dict(poses=[pose, (-1, 5, 0, 0, 0, 0)]), dict(poses=[(5, 5, 65536, 0, 0, 0)]),
           dict(poses=[(5, 5, 0, -1, 0, 0)]), dict(poses=[(5, 5, 0, 0, H, 0)]), dict(poses=[(5, 5, 0, 0, -1, 0)]), dict(poses=[(5, 5, 0, 0, 0, 3)]),
           dict(poses=[(5, 5, 0, 0, 0, -1)])]
    for kw in bad:
        assert call(**kw) == -1 and b"tsd_drive_fields_rollout" in lib.tsd_last_error(h), (kw, lib.tsd_last_error(h))
    assert call(form="route", n=0) == -1 and b"tsd_drive_rollout" in lib.tsd_last_error(h)
    assert choice.tobytes() == bytes([0xA5]) * 80 and (sc == S64).all() and (wh == S16).all()
    assert np.array_equal(grid.route_fields_keys(), c["fields"]) and np.array_equal(grid.route_keys(), c["keys"])
    assert call() == 0 and call(form="route", poses=[(5, 5, 0, 0, 0, 99)]) == 0      # the values at their limits pass; the route form ignores the layer
    kw = {k: v for k, v in good.items() if k != "poses"}
    _check(grid, c, "fields", good["poses"], what="after the refusals", **kw)
    fresh = capi.TsdGridDevice(8, 0.1, 0.3)
    choice = np.frombuffer(bytes([0xA5]) * 80, dtype=capi.DRIVE_CHOICE_DTYPE).copy()
    try:
        prm, keep = fresh._drive_params(8, [0], [0], None, (1, 1, 0, 0), 0, 0)
        p = capi.drive_poses([(5, 5, 0, 0, 0, 0)])
        for fn, why in ((fresh.lib.tsd_drive_rollout, b"no route result"), (fresh.lib.tsd_drive_fields_rollout, b"no fields result")):
            assert fn(fresh.h, C.byref(prm), p.ctypes.data, 1, choice.ctypes.data, None, None) == -1 and why in fresh.lib.tsd_last_error(fresh.h)
        assert fresh.lib.tsd_drive_dev_ptrs(fresh.h, None, None) == -1 and choice.tobytes() == bytes([0xA5]) * 80
    finally:
        fresh.close()


def test_a_pose_on_a_blocked_cell_is_legal(grid, cases):
    c = cases["door_96x64"]
    _load(grid, c, fields=False)
    want = _check(grid, c, "route", [(48, 10, 32768, 32768, 0, 0), (48, 10, 32768, 32768, H // 2, 0)], 6, [65536, 0], [0], "on the wall")
    assert want[2][:, 0, 0].tolist() == [0, 0] and want[2][:, 1, 0].tolist() == [(2 << 12) | 1] * 2       # it can drive off, it cannot stay


def test_closed_loop_equals_the_restatements(grid, cases):
    """the first 20 commands of the loop of tests/test_cpu_drive.py, rolled out on the device: the same sequence"""
    c = cases["door_96x64"]
    _load(grid, c, route=False)
    keys, wi = c["fields"][0], c["wi"]
    p = DR.loop_params()
    step = lambda pose, s, t: tuple(int(v) for v in capi.drive_advance(pose, s, t, 1))
    want = DR.closed_loop(lambda pose: DR.rollout(keys, wi, pose, **p), step, 120, keys, wi)[:20]

    def roll(pose):
        ch, sc, wh = grid.drive_fields_rollout([pose], p["steps"], p["step_q16"], p["turn"], body=p["body"], weights=p["weights"],
                                               nose_q16=p["nose_q16"], nose_miss=p["nose_miss"], want_scores=True)
        return ch[0], sc[0], wh[0]

    class Enough(Exception):
        pass

    got = []

    def roll20(pose):
        if len(got) == 20:
            raise Enough
        out = roll(pose)
        got.append((tuple(pose), int(out[0]["speed"]), int(out[0]["turn"])))
        return out

    with pytest.raises(Enough):
        DR.closed_loop(roll20, step, 120, keys, wi)
    assert got == want


# ---- the facade: SlamNode.explore_drive, SlamFleet.explore_drive on the two-node scene of test_gpu_route_fields.py
def _scene(**over):
    from ohm_tsd_slam_amd import synth
    gc, geo, scene = synth.CONFIGS["cfg1"]
    off = (-6.0, -4.5)
    world = synth.World(scene, gc, start_xy=[0.5 * gc.width + off[0], 0.5 * gc.width + off[1]])
    scans = synth.scans_for(world, geo, synth.trajectory(world, 4))
    over.update(occ_grid_time_interval=1000.0)
    over.update({"tsd_slam/max_range": 4.0, "tsd_slam/local_offset_x": off[0], "tsd_slam/local_offset_y": off[1]})
    return gc, geo, scans, over


def _xyt(node):
    p = node.pose_msg()
    q = p["orientation_xyzw"]
    return (float(p["position"][0]), float(p["position"][1]), 2.0 * float(np.arctan2(q[2], q[3])))


def _drive_pose(xyt, m, layer=0):
    """the facade's conversion, restated: cell, Q16 offset and heading index of a pose in the map's frame"""
    import math
    ux, uy = ((xyt[a] - m["origin_position"][a]) / m["resolution"] for a in (0, 1))
    cx, cy = math.floor(ux), math.floor(uy)
    h = round(math.remainder(xyt[2], 2 * math.pi) * H / (2 * math.pi)) % H
    return (cx, cy, min(65535, int(math.floor((ux - cx) * 65536.0))), min(65535, int(math.floor((uy - cy) * 65536.0))), h, layer)


DRIVE = dict(v_max=0.5, horizon_s=1.2, n_speeds=5, weights=(1, 1, 0, 1), nose_m=0.3, nose_miss=300, margin=2000)


def _lists(res, w_max, foot):
    """the facade's sample lists, restated"""
    import math
    dt = res / DRIVE["v_max"]
    T = min(256, math.ceil(DRIVE["horizon_s"] / dt))
    V = DRIVE["n_speeds"]
    n = math.floor(w_max * dt * H / (2 * math.pi) + 0.5)
    body = [(round(x / res * 65536.0), round(y / res * 65536.0)) for x, y in foot]
    return dt, dict(steps=T, step_q16=[round(65536.0 * (V - 1 - i) / (V - 1)) for i in range(V)], turn=DR.turns(n), body=body,
                    weights=DRIVE["weights"], nose_q16=round(DRIVE["nose_m"] / res * 65536.0), nose_miss=DRIVE["nose_miss"])


def _check_answer(out, want, lists, dt, pose, m, W, d_start):
    assert out["choice"].tobytes() == want.tobytes(), (out["choice"], want)
    assert out["admissible"] == want["admissible"] > 0 and want["speed"] >= 0
    assert want["d_end"] < d_start, "the command's arc must end nearer to the goal than it starts"
    s, t = lists["step_q16"][want["speed"]], lists["turn"][want["turn"]]
    res = m["resolution"]
    assert out["v"] == s / 65536.0 * res / dt and out["w"] == t * (2 * np.pi) / (H * dt) and 0 <= out["v"] <= DRIVE["v_max"]
    end = int(want["end_cell"])
    assert np.array_equal(out["end_xy"], [((end % W) + 0.5) * res + m["origin_position"][0], ((end // W) + 0.5) * res + m["origin_position"][1]])
    nxt = capi.drive_advance(pose, s, t, 1)
    assert np.array_equal(out["next_pose"], [(int(nxt["x"]) + int(nxt["fx"]) / 65536.0) * res + m["origin_position"][0],
                                             (int(nxt["y"]) + int(nxt["fy"]) / 65536.0) * res + m["origin_position"][1],
                                             int(nxt["heading"]) * (2 * np.pi) / H])
    assert (out["steps"], out["n_speeds"], out["n_turns"], out["n_body"], out["dt"]) == (
        lists["steps"], len(lists["step_q16"]), len(lists["turn"]), len(lists["body"]), dt)


def test_node_explore_drive():
    from ohm_tsd_slam_amd import facade
    gc, geo, scans, over = _scene(frontier_min_size=3)
    node = facade.SlamNode(facade.node_params(gc, geo, **over), synchronous=True)
    try:
        with pytest.raises(capi.TsdError):
            node.explore_drive(0, (0.0, 0.0, 0.0), 0.5, 0.5, 1.0)         # no plan yet
        for s in scans:
            node.laser(s, geo.angle_min, geo.angle_increment)
        node.publish_map()
        m = node.map_msg()
        data, W, res = m["data"], m["width"], m["resolution"]
        plan = node.explore_plan()
        goal = int(np.nonzero(plan["goals"]["cell"] != RR.NONE)[0][0])
        g = plan["goals"][goal]
        xyt = _xyt(node)
        foot = [(res, 0.0), (-res, 0.0), (0.0, res), (0.0, -res)]
        w_max = 40 * 2 * np.pi / (H * res / DRIVE["v_max"])                  # 40 headings per step: 81 turns
        dt, lists = _lists(res, w_max, foot)
        assert len(lists["turn"]) == 81
        out = node.explore_drive(goal, xyt, w_max=w_max, footprint=foot, **DRIVE)
        # the restatement: the field seeded at the goal on the published map, the rollout on it
        keys, _ = RR.route(data, [(int(g["cell"]) % W, int(g["cell"]) // W)], limit=int(g["dist"]) + DRIVE["margin"])
        assert np.array_equal(node.grid().route_keys(), keys)                 # the goal's field took the place of the plan's
        pose = _drive_pose(xyt, m)
        want, _, _ = DR.rollout(keys, RR.weight_image(data), pose, **lists)
        _check_answer(out, want, lists, dt, pose, m, W, int(keys[pose[1], pose[0]]) >> 4)
        assert node.explore_drive(goal, xyt, w_max=w_max, footprint=foot, **DRIVE)["choice"].tobytes() == want.tobytes()      # again
        with pytest.raises(capi.TsdError):
            node.explore_waypoints(2.0)                                       # the plan's field is gone
        for kw in (dict(goal=len(plan["goals"])), dict(goal=-1), dict(w_max=100 * w_max), dict(v_max=0.0), dict(horizon_s=-1.0),
                   dict(n_speeds=1), dict(n_speeds=65), dict(pose=(1e6, 0.0, 0.0)), dict(pose=(float("nan"), 0.0, 0.0)), dict(weights=(256, 0, 0, 0)),
                   dict(footprint=[(100.0, 0.0)]), dict(nose_m=100.0)):
            a = dict(DRIVE, goal=goal, pose=xyt, w_max=w_max, footprint=foot)
            a.update(kw)
            with pytest.raises(capi.TsdError):
                node.explore_drive(**a)
        node.explore_plan()
        node.explore_waypoints(2.0)
        node.publish_map()
        with pytest.raises(capi.TsdError):
            node.explore_drive(goal, xyt, w_max=w_max, footprint=foot, **DRIVE)      # the plan is of the map published before
    finally:
        node.close()


def test_fleet_explore_drive():
    from ohm_tsd_slam_amd import facade
    from tests import route_fields_ref as RF
    gc, geo, scans, over = _scene(frontier_min_size=2)
    offsets = [(0.0, 0.0), (24 * gc.cell_size, -16 * gc.cell_size)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, x_offset=xo, y_offset=yo, **over), synchronous=True, name=f"tsd_slam_{i}")
             for i, (xo, yo) in enumerate(offsets)]
    fleet = facade.SlamFleet(nodes)
    try:
        for s in scans:
            for n in nodes:
                n.laser(s, geo.angle_min, geo.angle_increment)
        m = fleet.publish_merged_map()
        data, W, res = m["data"], m["width"], m["resolution"]
        poses = [_xyt(n) for n in nodes]
        w_max = 40 * 2 * np.pi / (H * res / DRIVE["v_max"])
        with pytest.raises(capi.TsdError):
            fleet.explore_drive(poses, w_max=w_max, **DRIVE)                  # no dispatch yet
        d = fleet.explore_dispatch(view_radius_m=1.0, gain_weight=3, lookahead_m=1.5, unknown_depth=2, min_size=3, max_len=2048, max_way=64)
        assert (d["goal_of_robot"] >= 0).all()
        dt, lists = _lists(res, w_max, [])
        # as the nodes stand: the answer is the restatement's whatever it is (a node that faces away from its way is told to turn on
        # the spot, d_end == d at the start: the closed loop of test_cpu_drive.py)
        asis = fleet.explore_drive(poses, w_max=w_max, **DRIVE)
        # and with every node facing along the first segment of its way, as after that turn
        for r in range(2):
            way = d["waypoints"][r]
            assert len(way) >= 2
            poses[r] = poses[r][:2] + (float(np.arctan2(way[1][1] - way[0][1], way[1][0] - way[0][0])),)
        out = fleet.explore_drive(poses, w_max=w_max, **DRIVE)
        seeds = [(int(c) % W, int(c) // W) for c in d["goal"]["cell"]]
        keys, _ = RF.fields(data, seeds, limit=int(d["goal"]["dist"].max()) + DRIVE["margin"])
        assert np.array_equal(nodes[0].grid().route_fields_keys(), keys)      # layer r is seeded at node r's goal now
        for r in range(2):
            pose = _drive_pose(poses[r], m, r)
            want, _, _ = DR.rollout(keys[r], RR.weight_image(data), pose, **lists)
            _check_answer(out[r], want, lists, dt, pose, m, W, int(keys[r][pose[1], pose[0]]) >> 4)
            pose = _drive_pose(_xyt(nodes[r]), m, r)
            assert asis[r]["choice"].tobytes() == DR.rollout(keys[r], RR.weight_image(data), pose, **lists)[0].tobytes()
        with pytest.raises(capi.TsdError):
            fleet.explore_drive(poses[:1], w_max=w_max, **DRIVE)
        with pytest.raises(capi.TsdError):
            fleet.explore_drive(poses, w_max=100 * w_max, **DRIVE)
        fleet.publish_merged_map()
        with pytest.raises(capi.TsdError):
            fleet.explore_drive(poses, w_max=w_max, **DRIVE)                  # the dispatch is of the merged map published before
    finally:
        fleet.close()
        for n in nodes:
            n.close()
