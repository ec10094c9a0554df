#!/usr/bin/env python3
"""The fields call (tsd_route_fields_dev, csrc/route.hip with one layer per seed) on a SLAM-built map against the two ways to the same
keys without it: per L in --layers, with L seeds drawn from the map's free cells by a fixed generator,
  (a) one tsd_route_fields_dev with the L seeds: L layers relaxed side by side in the same rounds;
  (b) L tsd_route_dev calls with one seed each, one after the other: the same L fields, what a fleet had to do before;
  (c) one tsd_route_dev with all L seeds: one field for all, the floor -- one field's chain of rounds.
In one process, warmed, the three alternating within every repeat.  Per L one JSON line: the host's time per call of each (median,
min, max over the repeats), the rounds, the workgroups that found their tile active and the workgroups launched (tiles x layers x
rounds), the host's waits, and the stream time of the fields call's passes from the project's HIP-event profile.

    python tools/route_fields_rate.py [--cfg cfg2] [--scans 300] [--reps 10] [--layers 1,2,4,8,16] [--only a|b|c]

--only runs one of the three alone, for a run under rocprofv3 --kernel-trace --stats whose k_route_relax row is then that form's.
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

PASSES = ("route_fields_init", "route_fields_relax")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2")
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", default="1,2,4,8,16")
    ap.add_argument("--only", default="", choices=("", "a", "b", "c"))
    a = ap.parse_args()
    gc, geo, scene = synth.CONFIGS[a.cfg]
    world = synth.World(scene, gc)
    scans = np.ascontiguousarray(synth.scans_for(world, geo, synth.trajectory(world, a.scans)), dtype=np.float32)
    node = facade.SlamNode(facade.node_params(gc, geo, occ_grid_time_interval=0.0), synchronous=True)
    node.play([scans], 0, a.scans, geo.angle_min, geo.angle_increment)
    g = node.grid()
    occ, _, _ = g.map_frame()
    N = gc.cells
    cells, tiles = N * N, ((N + 31) // 32) ** 2
    free = np.argwhere(occ == 0)
    pick = np.random.default_rng(2025).choice(len(free), size=16, replace=False)
    all_seeds = [(int(free[i][1]), int(free[i][0])) for i in pick]
    print(json.dumps(dict(cfg=a.cfg, cells=N, tiles=tiles, scans=a.scans, free=int((occ == 0).sum()), unknown=int((occ < 0).sum()),
                          seeds=all_seeds)), flush=True)
    d_map = capi.DeviceBuffer(g, cells)
    d_map.upload(occ)
    lib, h, ptr = g.lib, g.h, C.c_void_p(d_map.ptr)
    for L in [int(v) for v in a.layers.split(",")]:
        seeds = all_seeds[:L]
        prm_all, keep_all = g._route_params(seeds, 0, None, 0, 0)
        prm_one = [g._route_params([s], 0, None, 0, 0) for s in seeds]
        fi, ri = capi.RouteFieldsInfo(), capi.RouteInfo()

        def run_a():
            assert lib.tsd_route_fields_dev(h, ptr, N, N, N, C.byref(prm_all), C.byref(fi)) == 0, lib.tsd_last_error(h)

        def run_b():
            for p, _ in prm_one:
                assert lib.tsd_route_dev(h, ptr, N, N, N, C.byref(p), C.byref(ri)) == 0, lib.tsd_last_error(h)

        def run_c():
            assert lib.tsd_route_dev(h, ptr, N, N, N, C.byref(prm_all), C.byref(ri)) == 0, lib.tsd_last_error(h)

        forms = [(k, f) for k, f in (("a", run_a), ("b", run_b), ("c", run_c)) if a.only in ("", k)]
        for _, f in forms:                                             # scratch (first use) and a warm call each
            f()
            f()
        if not a.only:                                                 # the same keys three ways, before anything is timed
            run_a()
            keys = g.route_fields_keys()
            run_c()
            assert np.array_equal(keys.min(axis=0), g.route_keys())
            for r, (p, _) in enumerate(prm_one):
                assert lib.tsd_route_dev(h, ptr, N, N, N, C.byref(p), C.byref(ri)) == 0
                one = g.route_keys()
                assert np.array_equal(one >> 4, keys[r] >> 4) or (one == capi.ROUTE_NONE).all()
        g.profile(True, ",".join(PASSES))
        g.profile_reset()
        times = {k: [] for k, _ in forms}
        counts = {}
        for _ in range(a.reps):
            for k, f in forms:
                t0 = time.perf_counter()
                f()
                times[k].append(1e3 * (time.perf_counter() - t0))
                if k == "a":
                    counts["a"] = dict(rounds=fi.rounds, converged=fi.converged, seeds_used=fi.seeds_used,
                                       tile_visits=g.route_fields_counts()[0], host_waits=g.route_fields_counts()[1],
                                       workgroups_launched=tiles * L * fi.rounds)
                elif k == "c":
                    counts["c"] = dict(rounds=ri.rounds, converged=ri.converged, tile_visits=g.route_counts()[0],
                                       host_waits=g.route_counts()[1], workgroups_launched=tiles * ri.rounds)
                else:
                    counts["b"] = dict(rounds_of_the_last_seed=ri.rounds, workgroups_launched_by_the_last_seed=tiles * ri.rounds)
        out = dict(cfg=a.cfg, layers=L, reps=a.reps)
        for k, _ in forms:
            t = np.array(times[k])
            out[k] = dict(host_ms_median=round(float(np.median(t)), 4), host_ms_min=round(float(t.min()), 4),
                          host_ms_max=round(float(t.max()), 4), **counts[k])
        if "a" in out and "b" in out:
            out["a_over_b"] = round(out["a"]["host_ms_median"] / out["b"]["host_ms_median"], 4)
        if "a" in out and "c" in out:
            out["a_over_c"] = round(out["a"]["host_ms_median"] / out["c"]["host_ms_median"], 4)
        if "a" in out:
            for name in PASSES:
                ms, launches = g.profile_get(name)
                mn, mx, _ = g.profile_spread(name)
                out[name] = dict(ms_per_call=round(ms / a.reps, 4), samples_per_call=launches / a.reps, min_ms=round(mn, 4), max_ms=round(mx, 4))
        g.profile(False)
        print(json.dumps(out), flush=True)
    d_map.free()
    node.close()


if __name__ == "__main__":
    main()
