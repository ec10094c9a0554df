#!/usr/bin/env python3
"""The route passes (tsd_route_dev / _goals / _trace, csrc/route.hip) on a SLAM-built map with one seed at the robot: on the map a
frame staged (unit weights, free_max 0) and on the cost map made of it (free_max 98, tsd_route_weights(98, --max-weight)).  Per case:
the rounds and the workgroups that found their tile active (mean per round), each pass's stream time from the project's HIP-event
profile ("route_init", "route_relax" -- one sample per batch of rounds --, "route_goals", "route_trace"), the host's time per call and
how often it waited for the device, beside the bytes the field cannot avoid -- the map read once, the keys written once -- over the
stream rate measured in the same process.  The goals are those of the map's frontiers (min_size 8).  One JSON line per case.

    python tools/route_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--radius 22] [--max-weight 20]
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

PASSES = ("route_init", "route_relax", "route_goals", "route_trace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--radius", type=int, default=22, help="the cost map's inflation radius in cells")
    ap.add_argument("--max-weight", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=4096)
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    _, cost, _ = g.costmap(a.radius)
    N = gc.cells
    cells, tiles = N * N, ((N + 31) // 32) ** 2
    stream_best, stream_mean = g.measure_stream(1 << 25, 5)         # 512 MiB of footprint: beyond the Infinity Cache
    free = np.argwhere(occ == 0)
    pose = node.pose_msg()["position"]
    m = node.map_msg() if node.map_frames() else None
    centre = np.array([N // 2, N // 2]) if m is None else np.floor((pose[:2] - m["origin_position"][:2]) / m["resolution"])[::-1]
    seed = tuple(int(v) for v in free[np.argmin(((free - centre) ** 2).sum(axis=1))][::-1]) if len(free) else (0, 0)
    print(json.dumps(dict(cfg=a.cfg, cells=N, tiles=tiles, scans=a.scans, free=int((occ == 0).sum()), unknown=int((occ < 0).sum()),
                          occupied=int((occ == 100).sum()), cost_below_99=int(((cost >= 0) & (cost <= 98)).sum()),
                          stream_gbs_best=round(stream_best, 1), stream_gbs_mean=round(stream_mean, 1), seed=seed)), flush=True)
    d_map = capi.DeviceBuffer(g, cells)
    floor_bytes = 5 * cells
    floor_ms = 1e3 * floor_bytes / (stream_best * 1e9)
    for source, src, free_max, w in (("map", occ, 0, None), ("costmap", cost, 98, g.route_weights(98, a.max_weight))):
        d_map.upload(src)
        d_occ = capi.DeviceBuffer(g, cells)
        d_occ.upload(occ)
        rec, _, _ = g.frontiers_of(d_occ.ptr, N, N, N, 0, 8, [seed])      # (the frontiers are the map's in both cases)
        d_occ.free()
        keys, info = g.route_of(d_map.ptr, N, N, N, [seed], free_max, w)           # scratch (first use)
        goals = g.route_goals()
        reach = goals["cell"][goals["cell"] != capi.ROUTE_NONE]
        _, lens = g.route_paths(reach, a.max_len)
        prm, keep = g._route_params([seed], free_max, w, 0, 0)
        ri, n = capi.RouteInfo(), C.c_int(0)
        paths = np.zeros((max(reach.size, 1), a.max_len), dtype=np.uint32)
        plen = np.zeros(max(reach.size, 1), dtype=np.int32)
        g.profile(True, ",".join(PASSES))
        g.profile_reset()
        host = dict(route=0.0, goals=0.0, trace=0.0)
        visits = waits = 0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rc = g.lib.tsd_route_dev(g.h, C.c_void_p(d_map.ptr), N, N, N, C.byref(prm), C.byref(ri))
            t1 = time.perf_counter()
            assert rc == 0, g.lib.tsd_last_error(g.h)
            v, wt = g.route_counts()
            visits, waits = visits + v, waits + wt
            assert g.lib.tsd_route_goals(g.h, C.byref(n)) == 0
            t2 = time.perf_counter()
            if reach.size:
                assert g.lib.tsd_route_trace(g.h, reach.ctypes.data, int(reach.size), a.max_len, paths.ctypes.data, plen.ctypes.data) == 0
            t3 = time.perf_counter()
            host["route"] += t1 - t0
            host["goals"] += t2 - t1
            host["trace"] += t3 - t2
        out = dict(cfg=a.cfg, source=source, free_max=free_max, max_weight=1 if w is None else a.max_weight, rounds=ri.rounds,
                   converged=ri.converged, reached=ri.reached, tile_visits_per_call=visits / a.reps,
                   active_tiles_per_round=round(visits / a.reps / max(ri.rounds, 1), 2), host_waits_per_call=waits / a.reps,
                   frontiers=int(rec.size), goals_with_a_cell=int(reach.size), longest_path_cells=int(lens.max()) if lens.size else 0,
                   path_cells=int(np.minimum(np.maximum(lens, 0), a.max_len).sum()),
                   farthest_goal_d=int(goals["dist"][goals["cell"] != capi.ROUTE_NONE].max()) if reach.size else 0, floor_bytes=floor_bytes, floor_ms=round(floor_ms, 5))
        for name in PASSES:
            ms, launches = g.profile_get(name)
            mn, mx, _ = g.profile_spread(name)
            out[name] = dict(ms_per_call=round(ms / a.reps, 4), samples_per_call=launches / a.reps, min_ms=round(mn, 4), max_ms=round(mx, 4))
        g.profile(False)
        field_ms = out["route_init"]["ms_per_call"] + out["route_relax"]["ms_per_call"]
        out["field_stream_ms_per_call"] = round(field_ms, 4)
        out["floor_over_field_time"] = round(floor_ms / field_ms, 4) if field_ms else None
        out["host_ms_per_call"] = {k: round(1e3 * v / a.reps, 4) for k, v in host.items()}
        print(json.dumps(out), flush=True)
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
