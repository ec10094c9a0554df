#!/usr/bin/env python3
"""The view pass (tsd_view_gains / tsd_view_claim / tsd_view_assign, csrc/view.hip) on a SLAM-built map: the goals of the map's plan
(frontiers of at least 8 cells, one seed at the robot) rated at each radius.  Per radius: the stream time of one tsd_view_gains call
over all goals and of one tsd_view_claim call from the project's HIP-event profile ("view_gain", "view_claim"), the host's time per
call, one tsd_view_assign for one robot, and two synthetic maps of the same size that take the kernel's phases apart -- "walled":
every candidate stands alone between blocking cells, so every ray ends at its first step and what is left is the mask's clearing
and the closing pass over the window; "open": all clear, so every ray runs its full length and sets its bits, and nothing is unknown.
One JSON line per radius.

    python tools/view_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--radius 140 511]
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


def timed(g, name, reps, call):
    g.profile(True, name)
    g.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    host = (time.perf_counter() - t0) / reps
    ms, launches = g.profile_get(name)
    mn, mx, _ = g.profile_spread(name)
    g.profile(False)
    return dict(us_per_call=round(1e3 * ms / max(launches, 1), 2), min_us=round(1e3 * mn, 2), max_us=round(1e3 * mx, 2),
                host_us_per_call=round(1e6 * host, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--radius", type=int, nargs="+", default=[140, 511])
    ap.add_argument("--gain-weight", type=int, default=4)
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    N = gc.cells
    free = np.argwhere(occ == 0)
    seed = tuple(int(v) for v in free[np.argmin(((free - N // 2) ** 2).sum(axis=1))][::-1]) if len(free) else (0, 0)
    d_map = capi.DeviceBuffer(g, N * N)
    d_map.upload(occ)
    g.frontiers_of(d_map.ptr, N, N, N, 0, 8, [seed])
    g.route_of(d_map.ptr, N, N, N, [seed])
    goals = g.route_goals()
    goals = goals[goals["cell"] != capi.ROUTE_NONE]
    cells = np.ascontiguousarray(goals["cell"])
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), unknown=int((occ < 0).sum()),
                          occupied=int((occ == 100).sum()), goals=int(cells.size), seed=seed)), flush=True)
    walled = np.full((N, N), 100, dtype=np.int8)
    walled.ravel()[cells] = 0
    d_alt = capi.DeviceBuffer(g, N * N)
    g.view_claims_reset(N, N)
    for R in a.radius:
        rec = g.view_gains_of(d_map.ptr, N, N, N, cells, R)           # scratch and the LDS limit (first use)
        out = dict(cfg=a.cfg, radius=R, goals=int(cells.size), lds_bytes=(2 * R + 1) * ((2 * R + 32) // 32) * 4,
                   visible_mean=round(float(rec["visible"].mean()), 1), unknown_mean=round(float(rec["unknown"].mean()), 1),
                   visible_max=int(rec["visible"].max()), window_cells=(2 * R + 1) ** 2)
        out["gains"] = timed(g, "view_gain", a.reps, lambda: g.view_gains_of(d_map.ptr, N, N, N, cells, R))
        out["gains_depth_8"] = timed(g, "view_gain", a.reps, lambda: g.view_gains_of(d_map.ptr, N, N, N, cells, R, 0, 8))
        out["gains_one_goal"] = timed(g, "view_gain", a.reps, lambda: g.view_gains_of(d_map.ptr, N, N, N, cells[:1], R))
        out["claim"] = timed(g, "view_claim", a.reps, lambda: g.view_claim_of(d_map.ptr, N, N, N, cells, R))
        g.view_claims_reset(N, N)
        t0 = time.perf_counter()
        of, picked, rounds = g.view_assign_of(d_map.ptr, N, N, N, goals, 1, R, a.gain_weight)
        out["assign_one_robot"] = dict(host_us=round(1e6 * (time.perf_counter() - t0), 1), rounds=rounds, goal=int(of[0]),
                                       gain=int(picked[0]["gain"]))
        d_alt.upload(walled)
        out["walled_closing_only"] = timed(g, "view_gain", a.reps, lambda: g.view_gains_of(d_alt.ptr, N, N, N, cells, R))
        d_alt.upload(np.zeros((N, N), dtype=np.int8))
        out["open_full_rays"] = timed(g, "view_gain", a.reps, lambda: g.view_gains_of(d_alt.ptr, N, N, N, cells, R))
        print(json.dumps(out), flush=True)
    d_alt.free()
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
