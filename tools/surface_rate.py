#!/usr/bin/env python3
"""What the surface list costs (tsd_surface_extract: k_surface_count, k_surface_scan, k_surface_emit): a cfg-2 grid (4096^2 cells at
0.025 m, pillars world) after --scans pushed scans, --reps extractions with and without normals, and in the same process and on the
same grid as many tsd_occupancy calls -- k_occ_cells + k_occ_mark read the same cells and find the same events, so that pair is the
yardstick.  Kernel times come from `rocprofv3 --kernel-trace --stats` in a run of its own (this script starts itself as the profiled
child; no counters); the host-clock time of the calls from an unprofiled loop.
Writes profiles/surface.txt.  Nothing here is a threshold.

    python tools/surface_rate.py [--out profiles/surface.txt] [--trace-dir DIR]
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, synth  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

MAX_RANGE, MIN_RANGE, LOW_REFL = 30.0, 0.001, 2.0


def setup(scans):
    gc, geo, scene = synth.CONFIGS["cfg2"]
    world = synth.World(scene, gc)
    g = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for p in synth.trajectory(world, scans, step_x=0.25):
        data, mask = O.ingest_f32(world.scan(p[0], p[1], p[2], geo), MAX_RANGE, geo.angle_increment)
        g.push(synth.pose_matrix(*p), data, mask, geo.angle_increment, geo.angle_min, MAX_RANGE, MIN_RANGE, LOW_REFL, want_stats=False)
    g.sync()
    return g


def timed(fn, reps):
    fn()                                         # (untimed: first use allocates)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def workload(scans, reps, normals):
    """the profiled child: reps extractions (with OR without normals: the two instantiations of k_surface_emit are told apart by
    the run, the other kernels have one name) and reps occupancy maps"""
    g = setup(scans)
    for _ in range(reps):
        g.surface_extract(normals=normals)
    for _ in range(reps):
        g.occupancy()
    g.close()


def kernel_stats(trace_dir):
    """name -> (calls, total ns) of the surface and occupancy kernels in rocprofv3's kernel stats"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "k_surface" in name or "k_occ_" in name:
                    short = name.split("(")[0].split("::")[-1].split("<")[0]
                    c, t = out.get(short, (0, 0))
                    out[short] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]))
    return out


def profiled(a, normals):
    tmp = None
    d = a.trace_dir
    if d is None:
        tmp = tempfile.TemporaryDirectory(prefix="surface_trace_")
        d = tmp.name
    d = os.path.join(d, "normals" if normals else "plain")
    os.makedirs(d, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
                    os.path.abspath(__file__), "--workload", "--scans", str(a.scans), "--reps", str(a.reps), "--normals", str(int(normals))],
                   check=True, timeout=400)
    return kernel_stats(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface.txt"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory, removed afterwards)")
    ap.add_argument("--scans", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workload", action="store_true", help="the profiled child: extractions and occupancy maps only")
    ap.add_argument("--normals", type=int, default=1)
    a = ap.parse_args()
    if a.workload:
        workload(a.scans, a.reps, bool(a.normals))
        return
    # 1. kernel times: two profiled runs of their own (fresh child processes; the program goes behind `--`)
    ks_n, ks_p = profiled(a, True), profiled(a, False)
    # 2. the calls, unprofiled, host clock
    g = setup(a.scans)
    init, _ = g.download_tile_state()
    n = g.surface_extract()
    _, n_occ = g.occupancy()
    wall_n = timed(lambda: g.surface_extract(normals=True), a.reps)
    wall_p = timed(lambda: g.surface_extract(normals=False), a.reps)
    wall_f = timed(lambda: g.surface_points(), a.reps)
    wall_o = timed(lambda: g.occupancy(), a.reps)
    xy, nr, ok = g.surface_points()
    lines = [f"tsd_surface_extract: cfg-2 grid ({g.cells}^2 cells at {g.cell_size} m, {g.tiles} tiles, {int(init.sum())} initialised), {a.scans} scans pushed",
             f"n = {n} points ({n * 16} bytes of xy; the occupancy map is {g.cells * g.cells} bytes), tsd_occupancy's n_surface = {n_occ}, "
             f"normal_ok set for {int(ok.sum())}", "",
             f"kernel times (rocprofv3 --kernel-trace --stats, {a.reps} calls each; mean per dispatch):"]

    def rows(ks, tag):
        tot = 0.0
        for name in ("k_surface_count", "k_surface_scan", "k_surface_scan_top", "k_surface_emit"):
            if name in ks:
                c, t = ks[name]
                lines.append(f"  {tag:16s} {name:20s} {c:4d} dispatches   mean {t / c / 1e3:9.2f} us")
                tot += t / c / 1e3
        lines.append(f"  {tag:16s} {'sum':20s}                   {tot:14.2f} us")
    rows(ks_n, "with normals")
    rows(ks_p, "without normals")
    tot = 0.0
    for name in ("k_occ_cells", "k_occ_mark"):
        if name in ks_n:
            c, t = ks_n[name]
            lines.append(f"  {'yardstick':16s} {name:20s} {c:4d} dispatches   mean {t / c / 1e3:9.2f} us")
            tot += t / c / 1e3
    lines.append(f"  {'yardstick':16s} {'sum':20s}                   {tot:14.2f} us")

    def med(v):
        return f"median {np.median(v):9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}"
    lines += ["", f"the calls, unprofiled ({a.reps} calls, host clock):",
              f"  tsd_surface_extract with normals        {med(wall_n)}",
              f"  tsd_surface_extract without normals     {med(wall_p)}",
              f"  extract + fetch of everything (numpy)   {med(wall_f)}",
              f"  tsd_occupancy (kernels + 16 MiB copy)   {med(wall_o)}"]
    g.close()
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
