"""What the ledger's epoch is for (csrc/grid_ledger.hpp, tsd_scan_submit in csrc/capi_scan.hip): the fused scan enqueues the NEXT scan's
ray cast right behind its push, and the next scan launches one of its own only if something changed the grid, the sensor's pose or the
context's ray-cast outputs in between.  Counted here as launches of the ray-cast kernel per scan (the per-kernel profile): 1 when the
ray cast enqueued ahead stands, 2 when the scan had to cast again.  A missing bump registers a scan against a grid that no longer
exists; a spurious one costs a ray cast (12 us) on every scan's latency chain.
"""
import numpy as np
import pytest

from ohm_tsd_slam_amd import synth
from tests.slam_driver import HipSlamFused, slam_kwargs

pytestmark = pytest.mark.gpu


def test_ray_casts_per_scan(oracle):
    gc = synth.GridConfig(9, 0.05)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    scans = synth.scans_for(world, geo, synth.trajectory(world, 12))
    kw = slam_kwargs(gc, geo)
    sh = HipSlamFused(oracle, **kw)
    g = sh.grid
    sh.process_scan(scans[0])                       # initialises: footprint, push, sensor
    g.profile(True, "raycast")
    g.profile_reset()

    def launches():
        g.sync()
        return g.profile_get("raycast")[1]

    def world_rays():
        return oracle.rays_rescale(oracle.rays_transform(sh.pose, sh.rays_local), g.cell_size, 1.0)

    def push_again():
        r = np.array(scans[0], dtype=np.float32)
        r[r < kw["laser_min_range"]] = 0.0
        data, mask = oracle.ingest_f32(r, kw["max_range"], kw["angle_increment"])
        g.push(sh.pose, data, mask, kw["angle_increment"], kw["angle_min"], kw["max_range"], kw["min_range"], kw["low_refl_range"],
               want_stats=False)

    # (what comes in between, the launches it makes itself, the launches of the scan behind it)
    steps = [
        ("the first fused scan", None, 0, 2),
        ("nothing", None, 0, 1),
        ("map_update, map_frame", lambda: (g.map_update(True, 2), g.map_frame(True, 2)), 0, 1),
        ("occupancy, color_image", lambda: (g.occupancy(True, 2), g.color_image()), 0, 1),
        ("digest, download_tiles, push_stats_total", lambda: (g.digest(), g.download_tiles(), g.push_stats_total()), 0, 1),
        ("raycast", lambda: g.raycast(sh.pose, world_rays(), kw["min_range"], kw["max_range"]), 1, 2),
        ("push", push_again, 0, 2),
        ("free_footprint", lambda: g.free_footprint([sh.pose[0, 2], sh.pose[1, 2]], 1.0, 1.0), 0, 2),
        ("set_max_truncation, same value", lambda: g.set_max_truncation(g.lib.tsd_max_truncation(g.h)), 0, 2),
        ("set_pose, the pose just reported", lambda: sh.sensor.set_pose(sh.pose, world_rays(), sh.rays_local), 0, 2),
        ("set_async_mapping(True)", lambda: sh.sensor.set_async_mapping(True), 0, 2),
    ]
    assert len(steps) == len(scans) - 1
    got = []
    n = launches()
    assert n == 0
    for (what, between, _, _), r in zip(steps, scans[1:]):
        if between is not None:
            between()
        n1 = launches()
        sh.process_scan(r)
        n2 = launches()
        got.append((n1 - n, n2 - n1))
        print(f"{what}: {n1 - n} ray-cast launches of its own, {n2 - n1} of the scan behind it")
        n = n2
    for (what, _, own, scan), (got_own, got_scan) in zip(steps, got):
        assert got_own == own, f"{what}: {got_own} ray-cast launches of its own, expected {own}"
        assert got_scan == scan, f"a scan after {what}: {got_scan} ray-cast launches, expected {scan}"
