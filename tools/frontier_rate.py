#!/usr/bin/env python3
"""The frontier pipeline (tsd_frontiers_dev, csrc/frontier.hip) on a SLAM-built map: each pass's stream time from the project's
HIP-event profile ("frontier_tile", "frontier_seam", "frontier_flatten", "frontier_rank", "frontier_stats") without seeds and with one
seed (the robot's cell: the regions are labelled as well, so tile / seam / flatten run twice), beside the frame that produced the
map in the same run (host time per tsd_map_frame; the profile has no name for k_map_frame, whose own time a `rocprofv3 --kernel-trace
--stats -- python tools/frontier_rate.py ...` pass lists next to the k_fr_* kernels), the bytes each pass has to move over the stream
rate measured in the same process, and what the map holds: frontier cells, frontiers, unions across tile seams.  One JSON line per
case.

    python tools/frontier_rate.py [--cfg cfg2] [--scans 300] [--reps 20] [--max-range 0]
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

PASSES = ("frontier_tile", "frontier_seam", "frontier_flatten", "frontier_rank", "frontier_stats")


def tiles_with(mask):
    H, W = mask.shape
    th, tw = (H + 31) // 32, (W + 31) // 32
    pad = np.zeros((th * 32, tw * 32), dtype=bool)
    pad[:H, :W] = mask
    return int(pad.reshape(th, 32, tw, 32).any(axis=(1, 3)).sum())


def floors(cells, n_seg, tiles_f, tiles_t, seeds):
    """bytes each pass cannot avoid: the map read once and every label written (tile); the labels of the edge cells of the tiles that
    hold a labelled cell (seam); those tiles' labels read once (flatten, stats), twice plus the segment counts written, scanned and
    read (rank); with seeds the regions' tiles on top"""
    t = tiles_f + (tiles_t if seeds else 0)
    return {"frontier_tile": 5 * cells * (2 if seeds else 1), "frontier_seam": 64 * 4 * t, "frontier_flatten": 4096 * t,
            "frontier_rank": 2 * 4096 * tiles_f + 16 * n_seg, "frontier_stats": 4096 * tiles_f * (2 if seeds else 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-range", type=float, default=0.0, help="tsd_slam/max_range override (0: the configuration's)")
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    over = {"tsd_slam/max_range": a.max_range} if a.max_range > 0 else {}
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0, **over), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    g.map_frame()                                  # staging and tables (first use)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        occ, _, _ = g.map_frame()
    frame_host_ms = 1e3 * (time.perf_counter() - t0) / a.reps
    N = gc.cells
    cells, n_seg = N * N, N * ((N + 31) // 32)
    stream_best, stream_mean = g.measure_stream(1 << 25, 5)         # 512 MiB of footprint: beyond the Infinity Cache
    d_map = capi.DeviceBuffer(g, cells)
    d_map.upload(occ)
    free = np.argwhere(occ == 0)
    pose = node.pose_msg()["position"]
    m = node.map_msg() if node.map_frames() else None
    centre = np.array([N // 2, N // 2]) if m is None else np.floor((pose[:2] - m["origin_position"][:2]) / m["resolution"])[::-1]
    seed = tuple(int(v) for v in free[np.argmin(((free - centre) ** 2).sum(axis=1))][::-1]) if len(free) else (0, 0)
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, free=int((occ == 0).sum()), unknown=int((occ < 0).sum()),
                          occupied=int((occ == 100).sum()), map_frame_host_ms=round(frame_host_ms, 3),
                          stream_gbs_best=round(stream_best, 1), stream_gbs_mean=round(stream_mean, 1), seed=seed)), flush=True)
    for seeds in ((), (seed,)):
        rec, lab, used = g.frontiers_of(d_map.ptr, N, N, N, 0, 1, seeds)          # scratch (first use)
        n_all, unions, region_unions = g.frontiers_counts()
        tiles_f, tiles_t = tiles_with(lab != capi.FRONTIER_NONE), tiles_with(occ == 0)
        prm, xy = g._frontier_params(0, 1, seeds)
        n, u = C.c_int(0), C.c_int(0)
        g.profile(True, ",".join(PASSES))
        g.profile_reset()
        for _ in range(a.reps):
            rc = g.lib.tsd_frontiers_dev(g.h, C.c_void_p(d_map.ptr), N, N, N, C.byref(prm), C.byref(n), C.byref(u))
            assert rc == 0, g.lib.tsd_last_error(g.h)
        fl = floors(cells, n_seg, tiles_f, tiles_t, bool(seeds))
        out = dict(cfg=a.cfg, seeds=len(seeds), seeds_used=used, frontier_cells=int((lab != capi.FRONTIER_NONE).sum()), frontiers=n_all,
                   reachable=int((rec["reachable"] == 1).sum()), seam_unions=unions, region_seam_unions=region_unions,
                   tiles=((N + 31) // 32) ** 2, tiles_with_frontier=tiles_f, tiles_with_free=tiles_t)
        total = 0.0
        for name in PASSES:
            ms, launches = g.profile_get(name)
            mn, mx, _ = g.profile_spread(name)
            per_call = ms / a.reps
            total += per_call
            floor_ms = 1e3 * fl[name] / (stream_best * 1e9)
            out[name] = dict(ms_per_call=round(per_call, 4), launches_per_call=launches / a.reps, min_ms=round(mn, 4), max_ms=round(mx, 4),
                             floor_bytes=fl[name], floor_ms=round(floor_ms, 5), floor_over_time=round(floor_ms / per_call, 3) if per_call else None)
        g.profile(False)
        out["kernels_ms_per_call"] = round(total, 4)
        print(json.dumps(out), flush=True)
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
