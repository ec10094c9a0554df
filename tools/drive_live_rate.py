#!/usr/bin/env python3
"""The live layer (tsd_drive_live_set and reason 7 of the rollouts, csrc/drive.hip) on a SLAM-built map: one robot on the route result
seeded at a goal drawn as tools/drive_rate.py draws it, at its two shapes -- "default", what the facade's explore_drive makes of its
request (cfg 2: T 40, 5 x 67, 8 body points), and "limits" (T 256, 64 x 129, 64 body points).
  rollout    tsd_drive_rollout without a layer: the instantiation every call took before there was one;
  live_r*    the same call with a layer of the 1 081 end points of a scan taken at the robot's pose, each a disc of 0, 8 and 64
             cells, the robot's own disc skipped;
  set        tsd_drive_live_set alone for 1 081 and 32 768 points at radius 8 and 64 on a 4096^2 and a 16384^2 image.
In one process, warmed.  JSON lines: the host's time per call (median, min, max over the repeats) and the stream time of
"drive_rollout" / "drive_live" from the project's HIP-event profile.  On a build without the live layer the first part runs alone:
that is the parent's column.

    python tools/drive_live_rate.py [--cfg cfg2] [--scans 300] [--reps 20] [--passes 3] [--only rollout|set]
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
BEAMS = 1081


def timed(g, kernel, call, reps):
    """(host ms per call: median, min, max; stream ms per call) of `call`, warmed twice"""
    call()
    call()
    g.profile(True, kernel)
    g.profile_reset()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    ms, launches = g.profile_get(kernel)
    g.profile(False)
    return dict(host_ms_median=round(float(np.median(ts)), 4), host_ms_min=round(min(ts), 4), host_ms_max=round(max(ts), 4),
                stream_ms_per_call=round(ms / max(launches, 1), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="", choices=("", "rollout", "set"))
    ap.add_argument("--passes", type=int, default=1, help="the rollout part that many times over, one JSON line per shape and pass")
    a = ap.parse_args()
    has_live = hasattr(capi.TsdGridDevice, "drive_live_set")
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    N = gc.cells
    free = np.argwhere(occ == 0)
    pick = np.random.default_rng(2025).choice(len(free), size=32, replace=False)
    goal = (int(free[pick[0]][1]), int(free[pick[0]][0]))
    start = (int(free[pick[17]][1]), int(free[pick[17]][0]))              # (tools/drive_fleet_rate.py: the first start lies beside a wall)
    # a scan of BEAMS beams taken at the start on the map itself: the first cell that is not free along each beam, 12 m at most
    ang = np.linspace(-0.75 * np.pi, 0.75 * np.pi, BEAMS)
    pts = []
    for th in ang:
        for k in range(1, int(12.0 / gc.cell_size)):
            x, y = int(np.floor(start[0] + 0.5 + k * np.cos(th))), int(np.floor(start[1] + 0.5 + k * np.sin(th)))
            if not (0 <= x < N and 0 <= y < N) or occ[y, x] != 0:
                break
        pts.append((x, y))
    pts = np.asarray(pts, dtype=np.int32)
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), goal=goal, start=start, beams=BEAMS, live=has_live)), flush=True)
    lib, h = g.lib, g.h
    if a.only in ("", "rollout"):
        d_map = capi.DeviceBuffer(g, N * N)
        d_map.upload(occ)
        g.route_of(d_map.ptr, N, N, N, seeds=[goal])
        p = capi.drive_poses([(start[0], start[1], 32768, 32768, 997 % H, 0)])
        shapes = (("default", facade_shape(gc.cell_size)), ("limits", LIMITS))
        for n_pass, (name, shape) in ((k, s) for k in range(a.passes) for s in shapes):
            dp, keep = g._drive_params(shape["steps"], shape["step_q16"], shape["turn"], shape["body"], RATE["weights"], RATE["nose_q16"], RATE["nose_miss"])
            choice = np.zeros(1, dtype=capi.DRIVE_CHOICE_DTYPE)
            why = np.zeros(dp.n_speeds * dp.n_turns, dtype=np.uint16)

            def roll():
                assert lib.tsd_drive_rollout(h, C.byref(dp), p.ctypes.data, 1, choice.ctypes.data, None, why.ctypes.data) == 0, lib.tsd_last_error(h)

            out = dict(cfg=a.cfg, shape=name, n_pass=n_pass, samples=dp.n_speeds * dp.n_turns, steps=dp.steps, body=dp.n_body, reps=a.reps)
            out["rollout"] = dict(timed(g, "drive_rollout", roll, a.reps), admissible=int(choice[0]["admissible"]))
            bare = choice.tobytes()
            for r in (0, 8, 64) if has_live else ():
                kept = g.drive_live_set(pts, r, skip=[(start[0], start[1], r + 4)], size=(N, N))
                out[f"live_r{r}"] = dict(timed(g, "drive_rollout", roll, a.reps), admissible=int(choice[0]["admissible"]), kept=kept,
                                         blocked_live=int(((why >> 12) == 7).sum()), live_cells=int(g.drive_live().sum()))
                g.drive_live_clear()
                roll()
                assert choice.tobytes() == bare                                 # cleared: the call without a layer again
            print(json.dumps(out), flush=True)
        d_map.free()
    if has_live and a.only in ("", "set"):
        rng = np.random.default_rng(7)
        for side in (4096, 16384):
            clouds = {BEAMS: np.clip(pts.astype(np.int64) * side // N, 0, side - 1).astype(np.int32),
                      32768: np.stack([rng.integers(0, side, 32768), rng.integers(0, side, 32768)], axis=1).astype(np.int32)}
            for n, cloud in clouds.items():
                for r in (8, 64):
                    out = dict(side=side, image_bytes=side * ((side + 31) // 32) * 4, points=n, radius=r, reps=a.reps)
                    prm = capi.DriveLiveParams(r, 0, None)

                    def put():
                        assert lib.tsd_drive_live_set(h, C.byref(prm), cloud.ctypes.data, n, side, side, None) == 0, lib.tsd_last_error(h)

                    out["set"] = timed(g, "drive_live", put, a.reps)
                    print(json.dumps(out), flush=True)
        g.drive_live_clear()
    node.close()


if __name__ == "__main__":
    main()
