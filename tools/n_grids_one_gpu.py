#!/usr/bin/env python3
"""N robots, N grids, ONE GPU: N synchronous SlamNodes on device 0, each with its own cfg-2 grid (4096^2 cells) and its own replay
thread, robot r starting multigpu.robot_offset_x(r) from the grid centre, and every --merge-every scans one merge of the N occupancy
maps by the same-device merge group (multigpu.LocalOccupancyGroup): begun while the robots stand between two chunks, waited for while
they run the next one.  This is co-residency on one chip, never a scaling curve: compare the per-robot rate at N > 1 with the N = 1
rate of the same tool on the same commit.

Run it once per N (each in a process of its own); every run adds its record under "runs" in --out:

    python tools/n_grids_one_gpu.py --n 1
    python tools/n_grids_one_gpu.py --n 2
    python tools/n_grids_one_gpu.py --n 8
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import facade, multigpu, synth  # noqa: E402


def robot_scans(world, geo, r, n):
    poses = synth.trajectory(world, n)
    poses[:, 0] += multigpu.robot_offset_x(r) - multigpu.robot_offset_x(0)
    return np.ascontiguousarray(synth.scans_for(world, geo, poses), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300, help="timed scans per robot")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--merge-every", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "n_grids_one_gpu.json"))
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    # the scene keeps a pillar-free 1.5 m around robot 0's start only: the pillars within 1 m of any of EIGHT robots' starts are taken
    # out, whatever --n is, so that every run of this tool sees the same world
    for r in range(8):
        x = world.start[0] + multigpu.robot_offset_x(r) - multigpu.robot_offset_x(0)
        d = np.hypot(world.circles[:, 0] - x, world.circles[:, 1] - world.start[1]) - world.circles[:, 2]
        world.circles = world.circles[d >= 1.0]
    total = a.warmup + a.scans
    scans = [robot_scans(world, geo, r, total) for r in range(a.n)]
    nodes = [facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0,
                                                **{"tsd_slam/local_offset_x": multigpu.robot_offset_x(r)}), synchronous=True)
             for r in range(a.n)]
    views = [n.grid() for n in nodes]
    grp = multigpu.LocalOccupancyGroup(views)
    grp.profile(True)
    chunks = [(k, min(a.merge_every, total - k)) for k in range(a.warmup, total, a.merge_every)]
    gate = threading.Barrier(a.n + 1)
    busy = [0.0] * a.n
    failed = []

    def robot(r):
        try:
            nodes[r].play([scans[r]], 0, a.warmup, geo.angle_min, geo.angle_increment)
            views[r].profile(True, "icp/2")
            views[r].profile_reset()
            gate.wait()
            for k, count in chunks:
                t = time.perf_counter()
                nodes[r].play([scans[r]], k, count, geo.angle_min, geo.angle_increment)
                busy[r] += time.perf_counter() - t
                gate.wait()           # every robot stands still: the merge is begun ...
                gate.wait()           # ... and the robots go on while it runs
        except Exception as e:       # noqa: BLE001
            failed.append(repr(e))
            gate.abort()

    threads = [threading.Thread(target=robot, args=(r,)) for r in range(a.n)]
    for t in threads:
        t.start()
    merges, occupied, begin_ms = 0, 0, 0.0
    try:
        gate.wait()
        t0 = time.perf_counter()
        for _ in chunks:
            gate.wait()
            if merges:
                occupied = grp.wait()             # (long done: it ran beside the chunk that just ended)
            tb = time.perf_counter()
            grp.merge_async()
            begin_ms += (time.perf_counter() - tb) * 1e3
            merges += 1
            gate.wait()
        occupied = grp.wait()
        wall = time.perf_counter() - t0
    except threading.BrokenBarrierError:
        wall = float("nan")
    for t in threads:
        t.join()
    if failed:
        raise SystemExit("; ".join(failed))
    icp = [v.profile_samples("icp") for v in views]
    allicp = np.concatenate(icp) if icp else np.zeros(1)
    ext_ms, mrg_ms, timed = grp.merge_times()
    processed = [n.processed() for n in nodes]
    rec = {
        "n_robots": a.n, "n_gpus": 1, "cfg": a.cfg, "cells": gc.cells, "scans_per_robot": a.scans, "merge_every": a.merge_every,
        "wall_s": round(wall, 4), "total_scans_per_s": round(a.n * a.scans / wall, 1),
        "per_robot_scans_per_s": [round(a.scans / b, 1) for b in busy],
        "per_robot_scans_per_s_min": round(min(a.scans / b for b in busy), 1),
        "k_icp_ms": {"p50": round(float(np.percentile(allicp, 50)), 4), "p99": round(float(np.percentile(allicp, 99)), 4),
                     "min": round(float(allicp.min()), 4), "max": round(float(allicp.max()), 4), "samples": int(allicp.size),
                     "per_robot_p50": [round(float(np.percentile(x, 50)), 4) for x in icp]},
        "merges": merges, "merges_timed": timed,
        "ms_per_merge": {"extract_sum_over_members": round(ext_ms / max(timed, 1), 4), "merge_kernel": round(mrg_ms / max(timed, 1), 4),
                         "host_begin": round(begin_ms / max(merges, 1), 4)},
        "merged_window": [grp.width, grp.height], "merged_occupied_cells": occupied, "processed": processed,
        "hw_queues_env": os.environ.get("GPU_MAX_HW_QUEUES"),
    }
    grp.close()
    for n in nodes:
        n.close()
    doc = {"what": "N SlamNodes with one cfg-2 grid each on ONE GPU, one same-device merge every merge_every scans "
                   "(tools/n_grids_one_gpu.py); co-residency on one chip, not a scaling curve", "n_gpus": 1, "runs": {}}
    if os.path.exists(a.out):
        try:
            doc = json.load(open(a.out))
        except ValueError:
            pass
    doc["runs"][str(a.n)] = rec
    base = doc["runs"].get("1")
    if base:
        for k, r in doc["runs"].items():
            r["per_robot_rate_vs_n1"] = round(r["per_robot_scans_per_s_min"] / base["per_robot_scans_per_s_min"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
