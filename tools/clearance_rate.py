#!/usr/bin/env python3
"""The clearance field and cost map (tsd_clearance_dev: k_clear_mask + k_clear_field) on a SLAM-built map: the two kernels' stream
time from the project's HIP-event profile ("clearance") per radius, with the tile skip on and off, beside the frame that produced the
map (host time per tsd_map_frame here; k_map_frame's own time comes from a `rocprofv3 --kernel-trace --stats -- python
tools/clearance_rate.py ...` pass, which also lists k_clear_mask / k_clear_field).  Prints the share of workgroups the skip takes, and
the byte bound -- map read once, 3 bytes per cell written -- over the stream rate measured in the same process.  One JSON line per case.

    python tools/clearance_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--radii 22,64,255]
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


def skipped_share(occ, R):
    """share of k_clear_field's workgroups (64 x 32 cells) with no obstacle tile within R of their area: the kernel's own rule"""
    H, W = occ.shape
    th, tw = (H + 31) // 32, (W + 31) // 32
    pad = np.zeros((th * 32, tw * 32), dtype=bool)
    pad[:H, :W] = occ == 100
    tiles = pad.reshape(th, 32, tw, 32).any(axis=(1, 3))
    acc = np.zeros((th + 1, tw + 1), dtype=np.int64)
    acc[1:, 1:] = tiles.cumsum(0).cumsum(1)
    skipped = total = 0
    for by in range(0, H, 32):
        y0, y1 = max(0, by - R) >> 5, min(H - 1, by + 31 + R) >> 5
        for bx in range(0, W, 64):
            x0, x1 = max(0, bx - R) >> 5, min(W - 1, bx + 63 + R) >> 5
            n = acc[y1 + 1, x1 + 1] - acc[y0, x1 + 1] - acc[y1 + 1, x0] + acc[y0, x0]
            skipped += n == 0
            total += 1
    return skipped / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--radii", default="22,64,255")
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    g.map_frame()                                  # staging and tables (first use)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        occ, _, n_surface = g.map_frame()
    frame_host_ms = 1e3 * (time.perf_counter() - t0) / a.reps
    N = gc.cells
    cells = N * N
    stream_best, stream_mean = g.measure_stream(1 << 25, 5)         # 512 MiB of footprint: beyond the Infinity Cache
    bound_ms = 1e3 * 4 * cells / (stream_best * 1e9)
    d_map, d_d2, d_cost = capi.DeviceBuffer(g, cells), capi.DeviceBuffer(g, 2 * cells), capi.DeviceBuffer(g, cells)
    d_map.upload(occ)
    print(json.dumps(dict(cfg=a.cfg, cells=N, scans=a.scans, occupied=int((occ == 100).sum()), surface=n_surface,
                          map_frame_host_ms=round(frame_host_ms, 3), stream_gbs_best=round(stream_best, 1),
                          stream_gbs_mean=round(stream_mean, 1), byte_bound_ms=round(bound_ms, 4))), flush=True)
    for R in (int(r) for r in a.radii.split(",")):
        tab = g.costmap_table(R, 0.25, 10.0)
        share = skipped_share(occ, R)
        for skip in (True, False):
            g.set_clearance_skip(skip)

            def call():
                rc = g.lib.tsd_clearance_dev(g.h, C.c_void_p(d_map.ptr), N, N, N, None, R, tab.ctypes.data_as(C.POINTER(C.c_int8)),
                                             C.c_void_p(d_d2.ptr), C.c_void_p(d_cost.ptr))
                assert rc == 0, g.lib.tsd_last_error(g.h)
            call()                                 # scratch, LDS attribute (first use)
            g.profile(True, "clearance")
            g.profile_reset()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                call()
            host_ms = 1e3 * (time.perf_counter() - t0) / a.reps
            total_ms, launches = g.profile_get("clearance")
            mn, mx, _ = g.profile_spread("clearance")
            g.profile(False)
            mean_ms = total_ms / max(launches, 1)
            print(json.dumps(dict(cfg=a.cfg, R=R, tile_skip=skip, launches=launches, kernels_ms_mean=round(mean_ms, 4),
                                  kernels_ms_min=round(mn, 4), kernels_ms_max=round(mx, 4), host_ms_per_call=round(host_ms, 3),
                                  workgroups_skipped=round(share, 4), fraction_of_byte_bound=round(bound_ms / mean_ms, 3) if mean_ms else None)),
                  flush=True)
        g.set_clearance_skip(True)
    for b in (d_map, d_d2, d_cost):
        b.free()
    node.close()


if __name__ == "__main__":
    main()
