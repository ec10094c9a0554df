#!/usr/bin/env python3
"""ThreadGrid's publication on a SLAM-built grid: --reps frames (tsd_map_frame_*: k_map_frame + k_occ_mark) and, for comparison,
the same number of tsd_occupancy + tsd_color_image calls (k_occ_cells + k_occ_mark + k_color_image).  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/map_frame_kernels.py --cfg cfg2`; prints the host-side time per publication
and the bytes a frame must move (grid read once, map read and written, image written) for the roofline.

    python tools/map_frame_kernels.py [--cfg cfg2] [--scans 200] [--reps 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    init, _ = g.download_tile_state()
    g.map_frame()                                  # staging and tables (first use)
    g.occupancy(); g.color_image()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        occ, rgb, n = g.map_frame()
    t_frame = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        occ2, n2 = g.occupancy()
        rgb2 = g.color_image()
    t_old = (time.perf_counter() - t0) / a.reps
    assert n == n2 and np.array_equal(occ, occ2) and np.array_equal(rgb, rgb2)
    cells = gc.cells * gc.cells
    tiles_init = int(init.sum())
    cell_bytes = 8 if g.lib.tsd_storage_bits() == 64 else 4
    # one read of the initialised tiles' interior + the persistent map read and written + map and image written (+ the marks' re-read)
    frame_bytes = tiles_init * 1024 * cell_bytes + 2 * cells + cells + 3 * cells
    print(json.dumps(dict(cfg=a.cfg, cells=gc.cells, tiles_initialized=tiles_init, surface=n, reps=a.reps,
                          host_ms_per_frame=round(1e3 * t_frame, 3), host_ms_occupancy_plus_image=round(1e3 * t_old, 3),
                          frame_min_bytes=frame_bytes)), flush=True)
    node.close()


if __name__ == "__main__":
    main()
