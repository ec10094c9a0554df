#!/usr/bin/env python3
"""What a map-to-map alignment costs (tsd_map_align: tsd_surface_extract, k_align_stage, k_align_score, k_reloc_peaks,
k_reloc_peaks_merge, k_align_refine): two cfg-2 grids (4096^2 cells at 0.025 m, pillars world) of the same scene built from the two
halves of one trajectory, the second one pushed at D * pose (D = 7.3 degrees about the start plus (0.43, -0.27) m), a 10 m x 10 m x 360
degree lattice at 0.1 m / 1 degree (3.6 M candidates), K = 16.  Kernel times come from `rocprofv3 --kernel-trace --stats` in a run of
its own (this script starts itself as the profiled child); the call's own search / refinement times from HIP events in an unprofiled
loop.  Writes profiles/align.txt.

    python tools/align_rate.py [--out profiles/align.txt] [--trace-dir DIR]
"""
import argparse
import csv
import glob
import math
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
STEP, NXY, NTHETA, K, ITERATIONS = 0.1, 100, 360, 16, 64
D_ANGLE, D_SHIFT = math.radians(7.3), (0.43, -0.27)
KERNELS = ("k_align", "k_reloc_peaks", "k_surface")


def rigid_about(angle, centre, shift):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, centre[0] - (c * centre[0] - s * centre[1]) + shift[0]],
                     [s, c, centre[1] - (s * centre[0] + c * centre[1]) + shift[1]], [0.0, 0.0, 1.0]])


def setup(scans):
    gc, geo, scene = synth.CONFIGS["cfg2"]
    world = synth.World(scene, gc)
    poses = synth.trajectory(world, scans, step_x=0.25)
    D = rigid_about(D_ANGLE, world.start, D_SHIFT)
    src = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    dst = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for i, p in enumerate(poses):
        data, mask = O.ingest_f32(world.scan(p[0], p[1], p[2], geo), MAX_RANGE, geo.angle_increment)
        g, pose = (src, synth.pose_matrix(*p)) if i < scans // 2 else (dst, D @ synth.pose_matrix(*p))
        g.push(pose, data, mask, geo.angle_increment, geo.angle_min, MAX_RANGE, MIN_RANGE, LOW_REFL, want_stats=False)
    side = gc.cells * gc.cell_size
    land = D @ np.array([0.5 * side, 0.5 * side, 1.0])               # where D carries the pivot (the centre of src's grid)
    lattice = dict(x0=land[0] - 49.4 * STEP, y0=land[1] - 49.7 * STEP, step_xy=STEP, nx=NXY, ny=NXY, ntheta=NTHETA,
                   theta0=D_ANGLE - 180.3 * math.radians(1.0), dtheta=math.radians(1.0), theta_wraps=True, K=K, iterations=ITERATIONS)

    def run(**over):
        return dst.align_to(src, **dict(lattice, **over))
    return dst, src, run, D, side


def workload(scans, reps):
    dst, src, run, _, _ = setup(scans)
    for _ in range(reps + 1):
        run()
    dst.close(); src.close()


def kernel_stats(trace_dir):
    """name -> (calls, total ns) of the alignment's rows of rocprofv3's kernel stats"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if any(k in name for k in KERNELS):
                    short = name.split("(")[0].split("::")[-1].split("<")[0]
                    c, t = out.get(short, (0, 0))
                    out[short] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align.txt"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory, removed afterwards)")
    ap.add_argument("--scans", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workload", action="store_true", help="the profiled child: the alignments only")
    a = ap.parse_args()
    if a.workload:
        workload(a.scans, a.reps)
        return
    # 1. kernel times: a profiled run of its own (a fresh child process; the program goes behind `--`)
    if a.trace_dir is None:
        tmp = tempfile.TemporaryDirectory(prefix="align_trace_")
        a.trace_dir = tmp.name
    os.makedirs(a.trace_dir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace_dir, "-o", "run", "--", sys.executable,
                    os.path.abspath(__file__), "--workload", "--scans", str(a.scans), "--reps", str(a.reps)], check=True, timeout=400)
    ks = kernel_stats(a.trace_dir)
    # 2. the call itself, unprofiled: HIP events around search and refinement
    dst, src, run, D, side = setup(a.scans)
    out = run()
    dst.profile(True, "all")
    search, refine, wall = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
        search.append(out["search_ms"]); refine.append(out["refine_ms"])
    dst.profile(False, "all")
    recs = dst.debug_align_peaks()
    worst = 0.0
    for px, py in ((0.5 * side, 0.5 * side), (0.0, 0.0), (side, 0.0), (0.0, side), (side, side)):
        p = np.array([px, py, 1.0])
        worst = max(worst, float(np.linalg.norm((out["T"] @ p - D @ p)[:2])))
    ang = abs(math.atan2(out["T"][1, 0], out["T"][0, 0]) - D_ANGLE)
    n, stride = out["n"], out["stride"]
    P = (n + stride - 1) // stride
    n_cand = NTHETA * NXY * NXY
    steps = sum(r["iterations"] + 1 for r in recs)                       # accumulations: one per step and the final one
    lines = [f"tsd_map_align: two cfg-2 grids ({dst.cells}^2 cells at {dst.cell_size} m), {a.scans // 2} + {a.scans - a.scans // 2} scans of one "
             f"trajectory, the second grid built at D * pose (7.3 degrees, (0.43, -0.27) m); src's surface list: {n} points, stride {stride} "
             f"({P} coarse points); lattice {NXY} x {NXY} x {NTHETA} at {STEP} m / 1 degree = {n_cand} candidates, K = {K}, {ITERATIONS} iterations at most",
             f"result: found {out['found']}, converged {out['converged']} after {out['iterations']} steps, {worst:.4f} m (worst over the grid's centre and corners) "
             f"and {ang:.2e} rad from D, rms {out['rms']:.4f} m, overlap {out['overlap']:.3f}, sum w {out['weight_sum']:.1f}, n_ok {out['n_ok']}",
             f"peaks: {out['n_peaks']} refined, status / steps / sum w: " + ", ".join(f"{r['status']}/{r['iterations']}/{r['sums'][9]:.0f}" for r in recs), "",
             f"kernel times (rocprofv3 --kernel-trace --stats, {a.reps + 1} calls):"]
    for name in sorted(ks):
        c, t = ks[name]
        lines.append(f"  {name:22s} {c:4d} dispatches   mean {t / c / 1e3:10.1f} us")
    if "k_align_score" in ks:
        c, t = ks["k_align_score"]
        sec = t / c * 1e-9
        lines.append(f"  k_align_score: {n_cand / sec / 1e6:.1f} M candidates/s, {n_cand * P / sec / 1e9:.2f} G look-ups/s "
                     f"({n_cand * P * 5 / sec / 1e9:.1f} G cell / flag reads/s)")
    if "k_align_refine" in ks:
        c, t = ks["k_align_refine"]
        sec = t / c * 1e-9
        longest = max(r["iterations"] + 1 for r in recs)
        lines.append(f"  k_align_refine: {steps} accumulations over {n} points in {len(recs)} workgroups, the longest workgroup {longest}: "
                     f"{sec / longest * 1e6:.1f} us per accumulation of the longest workgroup, {steps * n * 5 / sec / 1e9:.2f} G look-ups/s over the launch")
    lines += ["", f"the call, unprofiled ({a.reps} calls, HIP events on the context's stream / host clock):",
              f"  search (scores + peaks)                      median {np.median(search):8.3f} ms   min {min(search):.3f}   max {max(search):.3f}",
              f"  refinement, K = {K}, one launch               median {np.median(refine):8.3f} ms   min {min(refine):.3f}   max {max(refine):.3f}",
              f"  tsd_map_align wall clock (with the extraction of src's surface)   median {np.median(wall):8.3f} ms", ""]
    dst.close(); src.close()
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
