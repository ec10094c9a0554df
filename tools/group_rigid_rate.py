#!/usr/bin/env python3
"""What the merge under rigid transforms costs (k_group_merge_rigid, csrc/group.hip) beside the translation group's kernel
(k_group_merge) on the same member maps, in one process: two and eight random int8 maps of 4096^2 cells (cfg 2) resident on the device,
member 0 at the identity and member i >= 1 at
    identity   the whole-cell shift (17 i, 7 i),
    7.3deg     7.3 degrees about the grid's centre plus i * (0.43, -0.27) m,
    45deg      45 degrees about the grid's centre plus i * (0.43, -0.27) m.
Every figure is the merge kernel between two HIP events on the group's stream (tsd_group_profile / tsd_group_merge_times, one merge
per reading, so it includes the two records' own time), after warm-up merges, the cases taken in turn --rounds times so that a
drift of the machine shows in every case alike.  Writes profiles/group_merge_rigid.txt.

    python tools/group_rigid_rate.py [--out profiles/group_merge_rigid.txt] [--reps 10] [--rounds 3]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, multigpu  # noqa: E402

CS, LOG2 = 0.025, 12
SHIFT = (0.43, -0.27)
PEAK_TBS = 8.0


def about(angle, pivot, shift):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, pivot[0] - (c * pivot[0] - s * pivot[1]) + shift[0]],
                     [s, c, pivot[1] - (s * pivot[0] + c * pivot[1]) + shift[1]], [0.0, 0.0, 1.0]])


def transforms(case, n, cells):
    h = 0.5 * cells * CS
    if case == "identity":
        return [np.array([[1.0, 0.0, 17.0 * i * CS], [0.0, 1.0, 7.0 * i * CS], [0.0, 0.0, 1.0]]) for i in range(n)]
    angle = math.radians(7.3 if case == "7.3deg" else 45.0)
    return [np.eye(3)] + [about(angle, (h, h), (SHIFT[0] * i, SHIFT[1] * i)) for i in range(1, n)]


def timed_merges(grp, ptrs, reps):
    """`reps` readings of one merge each, in microseconds"""
    out = []
    _, before, _ = grp.merge_times()
    for _ in range(reps):
        grp.merge_maps_async(ptrs)
        grp.wait()
        _, total, _ = grp.merge_times()
        out.append((total - before) * 1e3)
        before = total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_merge_rigid.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2", type=int, default=LOG2)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    rows = []
    stream = None
    for n in (2, 8):
        grids = [capi.TsdGridDevice(a.log2, CS, 3 * CS) for _ in range(n)]
        cells = grids[0].cells
        maps = [rng.integers(-128, 128, size=(cells, cells), dtype=np.int16).astype(np.int8) for _ in grids]
        offs = [(17 * i, 7 * i) for i in range(n)]
        groups = {"translation": multigpu.LocalOccupancyGroup(grids, offs)}
        for case in ("identity", "7.3deg", "45deg"):
            groups[case] = multigpu.LocalOccupancyGroup(grids, transforms=transforms(case, n, cells))
        base = groups["translation"]
        base.merge_maps_async(maps)                          # the maps go to the device once, into this group's buffers
        want = base.merged()
        ptrs = [base.lib.tsd_group_member_map_dev(base.h, i) for i in range(n)]
        groups["identity"].merge_maps_async(ptrs)
        same = bool(np.array_equal(groups["identity"].merged(), want))
        times = {k: [] for k in groups}
        for g in groups.values():
            g.profile(True)
            timed_merges(g, ptrs, 3)                         # warm-up: code objects, the first touch of the merged map
        for _ in range(a.rounds):
            for k, g in groups.items():
                times[k] += timed_merges(g, ptrs, a.reps)
        if stream is None:
            stream = grids[0].measure_stream(1 << 25, 5)[0]  # 2 x 256 MiB: beyond the Infinity Cache
        t_base = float(np.median(times["translation"]))
        for k, g in groups.items():
            t = np.array(times[k])
            nbytes = n * cells * cells + g.width * g.height  # every member byte once (all lie inside the bounding box) + the window written
            med = float(np.median(t))
            rows.append(dict(n=n, case=k, window=(g.width, g.height), med=med, lo=float(t.min()), hi=float(t.max()), mb=nbytes / 1e6,
                             tbs=nbytes / (med * 1e-6) / 1e12, ratio=med / t_base, same=same, readings=len(t)))
        for g in groups.values():
            g.close()
        for g in grids:
            g.close()
    lines = [f"k_group_merge_rigid beside k_group_merge (csrc/group.hip) on the same random int8 maps of {cells}^2 cells of {CS} m, resident on the",
             "device: tools/group_rigid_rate.py, one process, the four groups of each N taken in turn.  us = the merge kernel between two HIP",
             "events on the group's stream (tsd_group_merge_times), one merge per reading: the records' own time is in every figure (about 6 us:",
             f"profiles/group_merge.txt has 12 / 27 us for k_group_merge under rocprofv3 and 18 / 33 us between events).  {rows[0]['readings']} readings per line",
             "after 3 warm-up merges.  MB = N x cells^2 (every member byte counted once; the bounding box holds every member) + W x H written.",
             f"stream = tsd_measure_stream of this process (k_calib_rmw over 2 x 256 MiB, best of 5): {stream / 1e3:.2f} TB/s.",
             "translation: tsd_group_create, member i at the whole-cell shift (17 i, 7 i).  identity: tsd_group_create_rigid with those shifts as",
             "transforms.  7.3deg / 45deg: member 0 at the identity, member i turned about the grid's centre and shifted by i x (0.43, -0.27) m.",
             f"The identity group's merged map equals the translation group's byte for byte: {all(r['same'] for r in rows)}.", "",
             " N case         window        median us  min us  max us      MB  TB/s of 8 TB/s  x translation"]
    for r in rows:
        lines.append(f"{r['n']:2d} {r['case']:<12} {r['window'][0]:5d} x {r['window'][1]:<5d} {r['med']:9.2f} {r['lo']:7.2f} {r['hi']:7.2f} {r['mb']:7.1f} "
                     f"{r['tbs']:5.2f} {r['tbs'] / PEAK_TBS:9.3f} {r['ratio']:13.2f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
