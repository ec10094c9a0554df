#!/usr/bin/env python3
"""What a relocalisation costs (tsd_relocalize: k_reloc_score, k_reloc_peaks, k_reloc_peaks_merge, then K registrations): a cfg-2 grid
(4096^2 cells at 0.025 m, pillars world) after --scans pushed scans, a 1081-beam scan taken off the trajectory, a 10 m x 10 m x 360
degree lattice at 0.1 m / 1 degree (3.6 M candidates), K = 16.  Kernel times come from `rocprofv3 --kernel-trace --stats` in a run of
its own (this script starts itself as the profiled child); the call's own search / refinement times from HIP events in an unprofiled
loop.  Also the gate's share of culled positions, the search over the same lattice moved to where no position passes the gate (what a
culled position costs) and, for context only, the numpy restatement's time for the tests' small lattice.
Writes profiles/reloc.txt.

    python tools/reloc_rate.py [--out profiles/reloc.txt] [--trace-dir DIR]
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
STEP, NXY, NTHETA, K = 0.1, 100, 360, 16


def setup(scans):
    gc, geo, scene = synth.CONFIGS["cfg2"]
    world = synth.World(scene, gc)
    g = capi.TsdGridDevice(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    for p in synth.trajectory(world, scans, step_x=0.25):
        data, mask = O.ingest_f32(world.scan(p[0], p[1], p[2], geo), MAX_RANGE, geo.angle_increment)
        g.push(synth.pose_matrix(*p), data, mask, geo.angle_increment, geo.angle_min, MAX_RANGE, MIN_RANGE, LOW_REFL, want_stats=False)
    truth = (world.start[0] + 0.93, world.start[1] + 0.38, 0.1 + math.radians(123.0))
    rays_local = O.rays_local(geo.beams, geo.angle_min, geo.angle_increment)
    data, mask = O.ingest_f32(world.scan(*truth, geo), MAX_RANGE, geo.angle_increment)
    sxy, ms, _ = O.scene_from_scan(rays_local, data, mask)
    pts = sxy.reshape(-1, 2)[ms.astype(bool)].copy()
    lattice = dict(x0=truth[0] - 49.4 * STEP, y0=truth[1] - 49.7 * STEP, step_xy=STEP, nx=NXY, ny=NXY, ntheta=NTHETA,
                   theta0=truth[2] - 180.3 * math.radians(1.0), dtheta=math.radians(1.0), theta_wraps=True, K=K, min_pairs=geo.beams // 4)
    prm = g.icp_params(30, 0.4, 0.02)

    def run(**over):
        return g.relocalize(pts, rays_local, data, mask, MIN_RANGE, MAX_RANGE, prm, **dict(lattice, **over))
    return g, run, truth, len(pts)


def workload(scans, reps):
    g, run, _, _ = setup(scans)
    for _ in range(reps + 1):
        run()
    g.close()


def kernel_stats(trace_dir):
    """name -> (calls, total ns) of the k_reloc_* rows of rocprofv3's kernel stats"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "k_reloc" in name:
                    short = name.split("(")[0].split("::")[-1]
                    c, t = out.get(short, (0, 0))
                    out[short] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc.txt"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory, removed afterwards)")
    ap.add_argument("--scans", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workload", action="store_true", help="the profiled child: the relocalisations only")
    a = ap.parse_args()
    if a.workload:
        workload(a.scans, a.reps)
        return
    # 1. kernel times: a profiled run of its own (a fresh child process; the program goes behind `--`)
    if a.trace_dir is None:
        tmp = tempfile.TemporaryDirectory(prefix="reloc_trace_")
        a.trace_dir = tmp.name
    os.makedirs(a.trace_dir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
                    "--workload", "--scans", str(a.scans), "--reps", str(a.reps)], check=True, timeout=400)
    ks = kernel_stats(a.trace_dir)
    # 2. the call itself, unprofiled: HIP events around search and refinement
    g, run, truth, P = setup(a.scans)
    out = run()
    g.profile(True, "all")
    search, refine, wall = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
        search.append(out["search_ms"]); refine.append(out["refine_ms"])
    # the same lattice in a corner of the grid that no scan reached (tiles never initialised): every position fails the gate, the
    # kernel does its gate look-up and its zero stores only
    culled = [run(x0=1.0, y0=1.0)["search_ms"] for _ in range(a.reps)]
    assert not g.debug_reloc_scores().any()
    run()                                                    # (the volume of the real search again, for the gate's share below)
    g.profile(False, "all")
    vol = g.debug_reloc_scores().reshape(NTHETA, NXY, NXY)
    passed = int(vol.any(axis=0).sum())                      # (a position that passes the gate scores > 0 for some rotation here)
    n_cand = NTHETA * NXY * NXY
    d = math.hypot(out["pose"][0, 2] - truth[0], out["pose"][1, 2] - truth[1])
    lines = [f"tsd_relocalize: cfg-2 grid ({g.cells}^2 cells at {g.cell_size} m), {a.scans} scans pushed, query scan of 1081 beams ({P} valid points), "
             f"lattice {NXY} x {NXY} x {NTHETA} at {STEP} m / 1 degree = {n_cand} candidates, K = {K}",
             f"result: found {out['found']}, {d:.4f} m from the true position, {out['icp'].pairs} pairs, {out['n_peaks']} peaks refined",
             f"gate: {NXY * NXY - passed} of {NXY * NXY} positions culled ({100.0 * (1 - passed / (NXY * NXY)):.1f} %): {passed * NTHETA} candidates scored, "
             f"{passed * NTHETA * P} look-ups", "",
             f"kernel times (rocprofv3 --kernel-trace --stats, {a.reps + 1} calls):"]
    for name in sorted(ks):
        c, t = ks[name]
        lines.append(f"  {name:22s} {c:4d} dispatches   mean {t / c / 1e3:10.1f} us")
    if "k_reloc_score" in ks:
        c, t = ks["k_reloc_score"]
        sec = t / c * 1e-9
        lines.append(f"  k_reloc_score: {n_cand / sec / 1e6:.1f} M candidates/s over the whole lattice, {passed * NTHETA / sec / 1e6:.1f} M scored candidates/s, "
                     f"{passed * NTHETA * P / sec / 1e9:.2f} G look-ups/s ({passed * NTHETA * P * 5 / sec / 1e9:.1f} G cell / flag reads/s)")
    lines += ["", f"the call, unprofiled ({a.reps} calls, HIP events on the context's stream / host clock):",
              f"  search (scores + peaks + copy of the keys)   median {np.median(search):8.3f} ms   min {min(search):.3f}   max {max(search):.3f}",
              f"  refinement, K = {K} ({out['n_refined']} registrations)     median {np.median(refine):8.3f} ms   min {min(refine):.3f}   max {max(refine):.3f}",
              f"  tsd_relocalize wall clock                    median {np.median(wall):8.3f} ms",
              f"  search, lattice moved to a corner no scan reached (every position culled: gate look-up + {NTHETA} zero stores each)   median {np.median(culled):8.3f} ms", ""]
    g.close()
    # 3. context: the numpy restatement on the tests' lattice (24 x 24 x 36, 1081 beams), CPU
    from tests import reloc_ref as R
    R.scene(1081)
    t0 = time.perf_counter()
    R.scene_scores(1081)
    lines.append(f"for context: the numpy restatement (tests/reloc_ref.py) takes {time.perf_counter() - t0:.2f} s for the tests' lattice of "
                 f"{R.NXY * R.NXY * R.NTHETA} candidates on the host CPU")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
