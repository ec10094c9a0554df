#!/usr/bin/env python3
"""The merge kernel of the same-device merge group (k_group_merge) at cfg 2's map size: N random 4096^2 int8 maps merged --reps times,
with x offsets that are multiples of 16 cells (one aligned 16-byte load per member and piece) or not (two loads, funnelled).  Meant to
run under `rocprofv3 --kernel-trace --stats`, one process per (N, offsets); prints one JSON line with the group's own HIP-event timing,
the result check against tests/group_merge_ref.py and the box's stream figure (tsd_measure_stream) of the same session.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/group_merge_profile.py --n 2 --offsets aligned
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, multigpu  # noqa: E402
from tests import group_merge_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--offsets", choices=("zero", "aligned", "unaligned"), default="aligned")
    ap.add_argument("--log2", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    step = {"zero": 0, "aligned": 16, "unaligned": 17}[a.offsets]
    offs = [(step * i + (1 if a.offsets == "unaligned" else 0), (7 * i) if step else 0) for i in range(a.n)]
    rng = np.random.default_rng(7)
    grids = [capi.TsdGridDevice(a.log2, 0.025, 0.075) for _ in range(a.n)]
    cells = grids[0].cells
    maps = [rng.integers(-128, 128, size=(cells, cells), dtype=np.int16).astype(np.int8) for _ in grids]
    grp = multigpu.LocalOccupancyGroup(grids, offs)
    grp.merge_maps_async(maps)
    ok = bool(np.array_equal(grp.merged(), R.merge(maps, offs)))
    ptrs = [grp.lib.tsd_group_member_map_dev(grp.h, i) for i in range(a.n)]
    grp.profile(True)
    for _ in range(a.reps):
        grp.merge_maps_async(ptrs)          # the maps are on the device: the kernel alone, back to back
        grp.wait()
    _, ms, timed = grp.merge_times()
    best, mean = grids[0].measure_stream(1 << 25, 5)        # 2 x 256 MiB: beyond the Infinity Cache
    nbytes = (a.n + 1) * cells * cells
    per = ms / max(timed, 1)
    print(json.dumps({"n": a.n, "offsets": a.offsets, "cells": cells, "window": [grp.width, grp.height], "equals_restatement": ok,
                      "merges_timed": timed, "event_ms_per_merge": round(per, 5), "bytes_n_plus_1_maps": nbytes,
                      "event_gbs": round(nbytes / (per * 1e-3) / 1e9, 1) if per > 0 else None,
                      "stream_gbs_best": round(best, 1), "stream_gbs_mean": round(mean, 1)}), flush=True)
    grp.close()
    for g in grids:
        g.close()


if __name__ == "__main__":
    main()
