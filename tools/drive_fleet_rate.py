#!/usr/bin/env python3
"""The fleet rollout (tsd_drive_fleet_rollout, csrc/drive.hip) beside the independent one (tsd_drive_fields_rollout) on a SLAM-built
map, behind the goal-seeded fields call both read: for 1, 2, 4, 8 and 16 robots, goals and starts drawn as tools/drive_rate.py draws
them, at its two shapes -- "default", what the facade's explore_drive makes of its request (cfg 2: T 40, 5 x 67, 8 body points), and
"limits" (T 256, 64 x 129, 64 body points).  Per shape and robot count
  fields     tsd_drive_fields_rollout, every robot alone on the map;
  fleet_sep0 the fleet call with sep_q16 = 0: the same results through the launch chain (init, map pass, a launch pair per rank), no
             conflict test -- the chain's own cost;
  fleet      the fleet call with a separation of 0.5 m, identity order, the robots at the drawn starts (far apart: every pair is
             "far" at every step, the conflict loop runs over all T steps of every sample);
  fleet_near the same with the robots on the 16 free cells nearest to the second start, where the rule bites.
In one process, warmed.  One JSON line per robot count: the host's time per call (median, min, max over the repeats), the stream time
of "drive_rollout" / "drive_fleet" from the project's HIP-event profile, the admissible samples and those refused by reason 6.

    python tools/drive_fleet_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--robots 1,2,4,8,16] [--only default|limits]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, facade, synth  # noqa: E402
from tools.drive_rate import LIMITS, RATE, facade_shape  # noqa: E402

H = capi.DRIVE_HEADINGS
SEPARATION_M = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--robots", default="1,2,4,8,16")
    ap.add_argument("--only", default="", choices=("", "default", "limits"))
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
    d2 = (free[:, 1] - starts[1][0]) ** 2 + (free[:, 0] - starts[1][1]) ** 2     # (the first start lies beside a wall: its footprint refuses every sample)
    near = [(int(free[i][1]), int(free[i][0])) for i in np.argsort(d2, kind="stable")[:16]]
    sep = int(round(SEPARATION_M / gc.cell_size * 65536.0))
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), sep_q16=sep, goals=goals, starts=starts, near=near)), flush=True)
    d_map = capi.DeviceBuffer(g, N * N)
    d_map.upload(occ)
    lib, h, ptr = g.lib, g.h, C.c_void_p(d_map.ptr)
    for R in [int(v) for v in a.robots.split(",")]:
        prm, keep = g._route_params(goals[:R], 0, None, 0, 0)
        fi = capi.RouteFieldsInfo()
        assert lib.tsd_route_fields_dev(h, ptr, N, N, N, C.byref(prm), C.byref(fi)) == 0, lib.tsd_last_error(h)
        order = np.arange(R, dtype=np.int32)
        out = dict(cfg=a.cfg, robots=R, reps=a.reps)
        for name, shape in SHAPES.items():
            if a.only not in ("", name):
                continue
            dp, keep2 = g._drive_params(shape["steps"], shape["step_q16"], shape["turn"], shape["body"], RATE["weights"], RATE["nose_q16"],
                                        RATE["nose_miss"])
            choice = np.zeros(R, dtype=capi.DRIVE_CHOICE_DTYPE)
            for tag, cells, s in (("fields", starts, None), ("fleet_sep0", starts, 0), ("fleet", starts, sep), ("fleet_near", near, sep)):
                p = capi.drive_poses([(x, y, 32768, 32768, (997 * k) % H, k) for k, (x, y) in enumerate(cells[:R])])
                fl = capi.DriveFleetParams(order.ctypes.data_as(C.POINTER(C.c_int32)), int(s or 0), 0)

                def roll():
                    if s is None:
                        rc = lib.tsd_drive_fields_rollout(h, C.byref(dp), p.ctypes.data, R, choice.ctypes.data, None, None)
                    else:
                        rc = lib.tsd_drive_fleet_rollout(h, C.byref(dp), C.byref(fl), p.ctypes.data, R, choice.ctypes.data, None, None, None)
                    assert rc == 0, lib.tsd_last_error(h)

                kernel = "drive_rollout" if s is None else "drive_fleet"
                roll()
                roll()
                g.profile(True, kernel)
                g.profile_reset()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    roll()
                    ts.append(1e3 * (time.perf_counter() - t0))
                ms, launches = g.profile_get(kernel)
                g.profile(False)
                lists = dict(body=shape["body"], want_scores=True, **RATE)
                if s is None:
                    ch, sc, why = g.drive_fields_rollout(p, shape["steps"], shape["step_q16"], shape["turn"], **lists)
                    alone = ch
                else:
                    ch, sc, why = g.drive_fleet_rollout(p, shape["steps"], shape["step_q16"], shape["turn"], order, s, **lists)
                assert ch.tobytes() == choice.tobytes()
                if tag == "fleet_sep0":
                    assert ch.tobytes() == alone.tobytes()        # without a separation the fleet call IS the independent one
                out[f"{name}_{tag}"] = dict(samples=R * dp.n_speeds * dp.n_turns, steps=dp.steps, body=dp.n_body,
                                            host_ms_median=round(float(np.median(ts)), 4), host_ms_min=round(min(ts), 4),
                                            host_ms_max=round(max(ts), 4), stream_ms_per_call=round(ms / max(launches, 1), 4),
                                            admissible=int(ch["admissible"].sum()), blocked=int(((why >> 12) == 6).sum()))
        print(json.dumps(out), flush=True)
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
