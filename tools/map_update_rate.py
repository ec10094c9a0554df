#!/usr/bin/env python3
"""The windowed map update (tsd_map_update_*) against the full frame (tsd_map_frame_*) on the bench trajectory.

Part 1, one JSON line: a SLAM-built grid is driven on --updates times --stride scans at a time; after each stride one update and
then one full frame are taken and timed on the host (begin to wait, copies included), and the update's window gives the bytes copied
and the share of the tiles its kernels ran over.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times
(k_map_frame_window against k_map_frame).
Part 2, one JSON line per case: façade scans per second while publishing every 100 ms with publish_map_updates off and on, the
loop of tools/map_publish_rate.py (whose figures in profiles/map_publish_rate.txt are the comparison).

    python tools/map_update_rate.py [--cfg cfg2] [--scans 200] [--updates 20] [--stride 10] [--seconds 6]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import facade, synth  # noqa: E402


def windows(gc, geo, scans, n_built, updates, stride):
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    try:
        node.play([scans], 0, n_built, geo.angle_min, geo.angle_increment)
        g = node.grid()
        g.map_update()                                 # staging, tables and the first (full) frame
        cells, tiles = gc.cells * gc.cells, (gc.cells // 32) ** 2
        t_upd, t_full, win_cells, pos = [], [], [], n_built
        for _ in range(updates):
            node.play([scans], pos, stride, geo.angle_min, geo.angle_increment)
            pos += stride
            node.lib.tsd_node_grid_lock(node.h)
            try:
                t0 = time.perf_counter()
                win, occ, rgb, _ = g.map_update()
                t1 = time.perf_counter()
                occ_f, rgb_f, _ = g.map_frame()
                t2 = time.perf_counter()
            finally:
                node.lib.tsd_node_grid_unlock(node.h)
            assert np.array_equal(occ, occ_f) and np.array_equal(rgb, rgb_f), "the patched buffers differ from a full frame"
            t_upd.append(t1 - t0); t_full.append(t2 - t1); win_cells.append(win[2] * win[3])
        wc = float(np.mean(win_cells))
        return dict(part="windows", updates=updates, stride=stride, window_cells_mean=round(wc), window_share=round(wc / cells, 5),
                    window_tiles_mean=round(wc / 1024), tiles=tiles, bytes_update=round(4 * wc), bytes_full=4 * cells,
                    host_ms_update=round(1e3 * float(np.median(t_upd)), 3), host_ms_full=round(1e3 * float(np.median(t_full)), 3),
                    note="host times include the wrapper's copy of the full buffers out of pinned memory, the same for both")
    finally:
        node.close()


def rate(gc, geo, loop, updates_on, seconds, warmup):
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.1, publish_map_updates=bool(updates_on)), synchronous=True)
    try:
        n = loop.shape[0]
        node.play([loop], 0, warmup, geo.angle_min, geo.angle_increment)
        f0, u0, done, pos = node.map_frames(), node.map_updates(), 0, warmup
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            count = min(n - pos, 500)
            node.play([loop], pos, count, geo.angle_min, geo.angle_increment)
            done += count
            pos = (pos + count) % n
        dt = time.perf_counter() - t0
        return dict(part="rate", interval_s=0.1, publish_map_updates=bool(updates_on), scans=done, seconds=round(dt, 3),
                    scans_per_s=round(done / dt, 1), full_maps=node.map_frames() - f0, updates=node.map_updates() - u0)
    finally:
        node.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=200, help="scans the grid is built from before the updates are measured")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--stride", type=int, default=10, help="scans between two updates")
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    total = a.scans + a.updates * a.stride
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, total)), dtype=np.float32)
    r = windows(gc, geo, scans, a.scans, a.updates, a.stride)
    r.update(cfg=a.cfg, cells=gc.cells)
    print(json.dumps(r), flush=True)
    if a.seconds > 0:
        loop = np.ascontiguousarray(np.concatenate([scans[:300], scans[298:0:-1]]), dtype=np.float32)
        for on in (False, True):
            r = rate(gc, geo, loop, on, a.seconds, a.warmup)
            r.update(cfg=a.cfg, cells=gc.cells, beams=geo.beams)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
