#!/usr/bin/env python3
"""Façade scans per second with and without ThreadGrid's publication (tsd_map_frame_*: the occupancy map and the colour image
copied to the host every occ_grid_time_interval beside the scans).  One synchronous SlamNode per case replays the same trajectory
back and forth (the poses stay continuous) from the native publisher thread for --seconds; the cases are the reference's default
interval (2 s), 100 ms and no publication (occ_grid_time_interval 0: no timer).  One JSON line per case.
--costmap: what <node>/costmap costs instead -- 100 ms with publish_map_updates on, publish_costmap off and on in turn, twice.

    python tools/map_publish_rate.py [--cfg cfg2] [--seconds 6] [--scans 300] [--costmap]
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


def run(gc, geo, loop, interval, seconds, warmup, **over):
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=float(interval), **over), synchronous=True)
    try:
        n = loop.shape[0]
        node.play([loop], 0, warmup, geo.angle_min, geo.angle_increment)
        f0, done, pos = node.map_frames(), 0, warmup
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            count = min(n - pos, 500)
            node.play([loop], pos, count, geo.angle_min, geo.angle_increment)
            done += count
            pos = (pos + count) % n
        dt = time.perf_counter() - t0
        return dict(interval_s=interval, scans=done, seconds=round(dt, 3), scans_per_s=round(done / dt, 1),
                    frames=node.map_frames() - f0, processed=node.processed(), costmaps=node.costmaps(), **over)
    finally:
        node.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--scans", type=int, default=300, help="length of the trajectory replayed back and forth")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--costmap", action="store_true", help="100 ms with map updates, publish_costmap off / on in turn")
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    loop = np.ascontiguousarray(np.concatenate([scans, scans[-2:0:-1]]), dtype=np.float32)     # 0 .. n-1 .. 1, then 0 again
    cases = [(i, {}) for i in (2.0, 0.1, 0.0)]
    if a.costmap:
        cases = [(0.1, dict(publish_map_updates=True, publish_costmap=on)) for on in (False, True, False, True)]
    for interval, over in cases:
        r = run(gc, geo, loop, interval, a.seconds, a.warmup, **over)
        r.update(cfg=a.cfg, cells=gc.cells, beams=geo.beams)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
