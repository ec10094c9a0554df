#!/usr/bin/env python3
"""The waypoint pass (tsd_route_waypoints, csrc/waypoint.hip) on a SLAM-built map: the paths to the goals of the map's plan (frontiers
of at least 8 cells, one seed at the robot) straightened at each look-ahead -- on the map a frame staged (unit weights, slack 0) and on
the cost map made of it (free_max 98, tsd_route_weights(98, --max-weight)) at each slack.  Two synthetic maps of the same size take
the kernel apart: an empty one, where every far candidate passes, and a one-cell staircase corridor in unknown space, where nothing
beyond the next path cell passes.  Per case: the stream time of the trace and of the waypoint kernel from the project's HIP-event
profile ("route_trace", "route_waypoints"), the host's time per call, the paths' cells and the waypoints emitted (one anchor each),
over enough calls for a window of --window seconds after a warm-up.  One JSON line per case.

    python tools/waypoints_rate.py [--cfg cfg2] [--scans 300] [--radius 22] [--max-weight 20] [--window 0.5]
                                   [--only map|costmap|empty|staircase] [--lookaheads 128,1024]

--only and --lookaheads cut the run down to one case, for a run under rocprofv3 --kernel-trace --stats whose k_route_waypoints row is
then that case's kernel time.
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

PASSES = ("route_trace", "route_waypoints")


def measure(g, cells, lookahead, slack, max_len, max_way, window):
    cells = np.ascontiguousarray(cells, dtype=np.uint32)
    way = np.zeros((cells.size, max_way), dtype=np.uint32)
    info = np.zeros(cells.size, dtype=capi.WAYPOINT_INFO_DTYPE)
    prm = capi.WaypointParams(lookahead, slack, max_len, max_way)

    def call():
        rc = g.lib.tsd_route_waypoints(g.h, cells.ctypes.data, int(cells.size), C.byref(prm), way.ctypes.data, info.ctypes.data)
        assert rc == 0, g.lib.tsd_last_error(g.h)

    call()                                                         # scratch (first use), and the duration of one call
    t0 = time.perf_counter()
    call()
    reps = max(3, int(np.ceil(window / max(time.perf_counter() - t0, 1e-6))))
    g.profile(True, ",".join(PASSES))
    g.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    host = time.perf_counter() - t0
    out = dict(lookahead=lookahead, slack=slack, goals=int(cells.size), reps=reps, host_ms_per_call=round(1e3 * host / reps, 4))
    for name in PASSES:
        ms, launches = g.profile_get(name)
        mn, mx, _ = g.profile_spread(name)
        out[name] = dict(ms_per_call=round(ms / reps, 4), samples_per_call=launches / reps, min_ms=round(mn, 4), max_ms=round(mx, 4))
    g.profile(False)
    has = info["len"] > 0
    lens, n_way = info["len"][has].astype(np.int64), info["n_way"][has].astype(np.int64)
    out.update(paths=int(has.sum()), path_cells=int(lens.sum()), longest_path_cells=int(lens.max()) if lens.size else 0,
               waypoints=int(n_way.sum()), most_waypoints=int(n_way.max()) if n_way.size else 0,
               cost_over_dist=round(float(info["cost"][has].sum()) / max(float(info["dist"][has].sum()), 1.0), 6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--radius", type=int, default=22, help="the cost map's inflation radius in cells")
    ap.add_argument("--max-weight", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--max-way", type=int, default=256)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per case")
    ap.add_argument("--only", default="", help="map, costmap, empty or staircase: that case alone")
    ap.add_argument("--lookaheads", default="128,1024")
    a = ap.parse_args()
    lookaheads = tuple(int(v) for v in a.lookaheads.split(","))
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    _, cost, _ = g.costmap(a.radius)
    N = gc.cells
    free = np.argwhere(occ == 0)
    pose = node.pose_msg()["position"]
    m = node.map_msg() if node.map_frames() else None
    centre = np.array([N // 2, N // 2]) if m is None else np.floor((pose[:2] - m["origin_position"][:2]) / m["resolution"])[::-1]
    seed = tuple(int(v) for v in free[np.argmin(((free - centre) ** 2).sum(axis=1))][::-1]) if len(free) else (0, 0)
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), unknown=int((occ < 0).sum()),
                          occupied=int((occ == 100).sum()), seed=seed, max_len=a.max_len, max_way=a.max_way)), flush=True)
    d_map = capi.DeviceBuffer(g, N * N)
    d_map.upload(occ)
    rec, _, _ = g.frontiers_of(d_map.ptr, N, N, N, 0, 8, [seed])
    reach_map = None
    for source, src, free_max, w, slacks in (("map", occ, 0, None, (0,)), ("costmap", cost, 98, g.route_weights(98, a.max_weight), (0, 200))):
        d_map.upload(src)
        g.route_of(d_map.ptr, N, N, N, [seed], free_max, w)
        goals = g.route_goals()
        reach = goals["cell"][goals["cell"] != capi.ROUTE_NONE]
        if reach_map is None:
            reach_map = reach
        for lookahead in lookaheads if a.only in ("", source) else ():
            for slack in slacks:
                out = dict(cfg=a.cfg, source=source, frontiers=int(rec.size))
                out.update(measure(g, reach, lookahead, slack, a.max_len, a.max_way, a.window))
                print(json.dumps(out), flush=True)
    # every far candidate passes: an empty map, the plan's goal cells
    d_map.upload(np.zeros((N, N), dtype=np.int8))
    g.route_of(d_map.ptr, N, N, N, [seed])
    for lookahead in lookaheads if a.only in ("", "empty") else ():
        out = dict(cfg=a.cfg, source="synthetic: empty")
        out.update(measure(g, reach_map, lookahead, 0, a.max_len, a.max_way, a.window))
        print(json.dumps(out), flush=True)
    # nothing beyond a + 1 passes: a staircase one cell wide, as many goals along it as the plan has, the farthest as far as the plan's
    stairs = np.full((N, N), -1, dtype=np.int8)
    i = np.arange(8, N - 8)
    stairs[i, i] = 0
    stairs[i, i + 1] = 0
    d_map.upload(stairs)
    g.route_of(d_map.ptr, N, N, N, [(8, 8)])
    longest = 820
    k = 8 + np.linspace(1, longest // 2, num=max(int(reach_map.size), 1)).astype(np.int64)
    for lookahead in lookaheads if a.only in ("", "staircase") else ():
        out = dict(cfg=a.cfg, source="synthetic: staircase")
        out.update(measure(g, k * N + k, lookahead, 0, a.max_len, a.max_len, a.window))
        print(json.dumps(out), flush=True)
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
