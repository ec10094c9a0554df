#!/usr/bin/env python3
"""The rollout (tsd_drive_fields_rollout, csrc/drive.hip) on a SLAM-built map, behind the goal-seeded fields call it reads: for 1 and
16 robots, each driving to a goal of its own drawn with its start from the map's free cells by a fixed generator,
  the fields call seeded at the robots' goals (tsd_route_fields_dev, unit weights): the navigation potentials, one layer per robot;
  the rollout at two shapes: "default" -- what the facade's explore_drive makes of v_max 0.5 m/s, w_max 1 rad/s, a horizon of 2 s,
  its default of 5 speeds and a footprint of 8 points on a circle of 0.2 m at the map's cell size (cfg 2: T 40, 5 x 67, 8 body
  points) -- and "limits" (T 256, 64 x 129, 64 body points);
  the same two shapes with every sample refused at step 1: the robots stand deep in unknown space, where every neighbour has w = 0.
Last the facade's own call, SlamNode.explore_drive with the same request on the node's published map: the goal-seeded route call and
the rollout together, as a user pays them.
In one process, warmed.  One JSON line per robot count: the host's time per call (median, min, max over the repeats), the admissible
samples, and the stream time of "drive_rollout" from the project's HIP-event profile.

    python tools/drive_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--robots 1,16] [--only fields|default|limits]

--only runs one part alone, for a run under rocprofv3 --kernel-trace --stats.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, facade, synth  # noqa: E402

H = capi.DRIVE_HEADINGS


def turns(n, unit):
    return [0] + [unit * v for m in range(1, n + 1) for v in (m, -m)]


def ring(B, radius_q16):
    D = capi.drive_table().astype(np.int64)
    return [((radius_q16 * int(D[(b * H) // B, 0])) >> 16, (radius_q16 * int(D[(b * H) // B, 1])) >> 16) for b in range(B)]


FACADE = dict(v_max=0.5, w_max=1.0, horizon_s=2.0, n_speeds=5, radius_m=0.2)


def facade_shape(res):
    """the lists ThreadGrid's driveSamples makes of FACADE at a cell size"""
    dt = res / FACADE["v_max"]
    V = FACADE["n_speeds"]
    n = int(math.floor(FACADE["w_max"] * dt * H / (2 * math.pi) + 0.5))
    return dict(steps=min(256, int(math.ceil(FACADE["horizon_s"] / dt))), step_q16=[round(65536.0 * (V - 1 - i) / (V - 1)) for i in range(V)],
                turn=turns(n, 1), body=ring(8, round(FACADE["radius_m"] / res * 65536.0)))


LIMITS = dict(steps=256, step_q16=[65536 - 1024 * i for i in range(64)], turn=turns(64, 8), body=ring(64, 3 * 65536))
RATE = dict(weights=(1, 1, 0, 1), nose_q16=4 * 65536, nose_miss=200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--robots", default="1,16")
    ap.add_argument("--only", default="", choices=("", "fields", "default", "limits"))
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    N = gc.cells
    SHAPES = {"default": facade_shape(gc.cell_size), "limits": LIMITS}
    free = np.argwhere(occ == 0)
    pick = np.random.default_rng(2025).choice(len(free), size=32, replace=False)
    goals = [(int(free[i][1]), int(free[i][0])) for i in pick[:16]]
    starts = [(int(free[i][1]), int(free[i][0])) for i in pick[16:]]
    # cells whose 3 x 3 neighbourhood holds no traversable cell: every sample is refused at step 1 there
    t = np.pad(occ == 0, 1)
    near = sum(t[1 + dy:1 + dy + N, 1 + dx:1 + dx + N] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    deep = np.argwhere(near == 0)
    dpick = np.random.default_rng(7).choice(len(deep), size=16, replace=False)
    blocked = [(int(deep[i][1]), int(deep[i][0])) for i in dpick]
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), goals=goals, starts=starts)), flush=True)
    d_map = capi.DeviceBuffer(g, N * N)
    d_map.upload(occ)
    lib, h, ptr = g.lib, g.h, C.c_void_p(d_map.ptr)
    for R in [int(v) for v in a.robots.split(",")]:
        prm, keep = g._route_params(goals[:R], 0, None, 0, 0)
        fi = capi.RouteFieldsInfo()

        def fields():
            assert lib.tsd_route_fields_dev(h, ptr, N, N, N, C.byref(prm), C.byref(fi)) == 0, lib.tsd_last_error(h)

        def poses(cells):
            return capi.drive_poses([(x, y, 32768, 32768, (997 * k) % H, k) for k, (x, y) in enumerate(cells[:R])])

        out = dict(cfg=a.cfg, robots=R, reps=a.reps)
        fields()
        fields()
        if a.only in ("", "fields"):
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fields()
                ts.append(1e3 * (time.perf_counter() - t0))
            out["fields"] = dict(host_ms_median=round(float(np.median(ts)), 4), host_ms_min=round(min(ts), 4), host_ms_max=round(max(ts), 4),
                                 rounds=fi.rounds, converged=fi.converged, seeds_used=fi.seeds_used)
        for name, shape in SHAPES.items():
            if a.only not in ("", name):
                continue
            for tag, cells in (("", starts), ("_refused", blocked)):
                p = poses(cells)
                dp, keep2 = g._drive_params(shape["steps"], shape["step_q16"], shape["turn"], shape["body"], RATE["weights"], RATE["nose_q16"],
                                            RATE["nose_miss"])
                choice = np.zeros(R, dtype=capi.DRIVE_CHOICE_DTYPE)

                def roll():
                    assert lib.tsd_drive_fields_rollout(h, C.byref(dp), p.ctypes.data, R, choice.ctypes.data, None, None) == 0, lib.tsd_last_error(h)

                roll()
                roll()
                g.profile(True, "drive_rollout")
                g.profile_reset()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    roll()
                    ts.append(1e3 * (time.perf_counter() - t0))
                ms, launches = g.profile_get("drive_rollout")
                g.profile(False)
                ch, sc, why = g.drive_fields_rollout(p, shape["steps"], shape["step_q16"], shape["turn"], body=shape["body"], want_scores=True, **RATE)
                assert ch.tobytes() == choice.tobytes()
                if tag:
                    assert ((why & 4095) == 1).all() and (ch["speed"] == -1).all()
                out[name + tag] = dict(samples=R * dp.n_speeds * dp.n_turns, steps=dp.steps, body=dp.n_body,
                                       host_ms_median=round(float(np.median(ts)), 4), host_ms_min=round(min(ts), 4), host_ms_max=round(max(ts), 4),
                                       stream_ms_per_call=round(ms / max(launches, 1), 4), admissible=ch["admissible"].tolist(),
                                       refused_by={str(r): int(((why >> 12) == r).sum()) for r in range(6) if ((why >> 12) == r).any()})
        print(json.dumps(out), flush=True)
    d_map.free()
    if not a.only:
        # the facade: plan on the published map, then the drive call towards the plan's first goal from the node's own pose
        node.publish_map()
        plan = node.explore_plan()
        goal = int(np.nonzero(plan["goals"]["cell"] != capi.ROUTE_NONE)[0][0])
        p = node.pose_msg()
        xyt = (float(p["position"][0]), float(p["position"][1]), 2.0 * math.atan2(p["orientation_xyzw"][2], p["orientation_xyzw"][3]))
        D = capi.drive_table().astype(np.float64) / 65536.0
        foot = [(FACADE["radius_m"] * D[(b * H) // 8, 0], FACADE["radius_m"] * D[(b * H) // 8, 1]) for b in range(8)]
        kw = dict(v_max=FACADE["v_max"], w_max=FACADE["w_max"], horizon_s=FACADE["horizon_s"], n_speeds=FACADE["n_speeds"], footprint=foot,
                  weights=RATE["weights"], nose_m=4 * gc.cell_size, nose_miss=RATE["nose_miss"])
        out = node.explore_drive(goal, xyt, **kw)
        node.explore_drive(goal, xyt, **kw)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            node.explore_drive(goal, xyt, **kw)
            ts.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(facade="SlamNode.explore_drive", goal_dist=int(plan["goals"]["dist"][goal]), steps=out["steps"],
                              samples=out["n_speeds"] * out["n_turns"], body=out["n_body"], admissible=out["admissible"], v=out["v"], w=out["w"],
                              host_ms_median=round(float(np.median(ts)), 4), host_ms_min=round(min(ts), 4), host_ms_max=round(max(ts), 4))),
              flush=True)
    node.close()


if __name__ == "__main__":
    main()
