#!/usr/bin/env python3
"""What a TSD-level fusion costs (k_tsd_fuse, tsd_fuse_*): N = 2 and 8 cfg-2 grids (4096^2 cells at 0.025 m) after --scans scans each,
fused at offsets 0 and (17, -5) per member.  Per case: the kernel's HIP-event time (median, min .. max of --reps launches), the bytes it
moves counted from the tile states, that rate as a fraction of the stream figure measured in the same run (tsd_measure_stream), the
same launch over EMPTY members (what 16 384 workgroups cost before they move a byte), and the only route to a fused grid without the
kernel: tsd_download_tiles x N, the numpy restatement (tests/tsd_fuse_ref.py), tsd_upload_tiles.  Writes profiles/tsd_fuse.txt.

    python tools/tsd_fuse_rate.py [--out profiles/tsd_fuse.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, facade, multigpu, synth  # noqa: E402
from tests import tsd_fuse_ref as F  # noqa: E402

MAX_RANGE, MIN_RANGE, LOW_REFL = 30.0, 0.001, 2.0
CELL_BYTES = 16          # tsd + weight, fp64 storage


def push_scans(host, grid, world, geo, robot, n, off):
    cs = grid.cell_size
    for k in range(n):
        x, y, yaw = world.cx + multigpu.robot_offset_x(robot) + 0.06 * k, world.cy - 0.21, 0.1 + 0.01 * k
        r = np.ascontiguousarray(world.scan(x, y, yaw, geo), dtype=np.float32)
        data, mask = np.zeros(geo.beams), np.zeros(geo.beams, dtype=np.uint8)
        host.tsd_host_sensor_ingest_f32(r.ctypes.data_as(C.POINTER(C.c_float)), geo.beams, geo.angle_increment, geo.angle_min, MAX_RANGE,
                                        data.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
        grid.push(synth.pose_matrix(x - off[0] * cs, y - off[1] * cs, yaw), data, mask, geo.angle_increment, geo.angle_min,
                  MAX_RANGE, MIN_RANGE, LOW_REFL, want_stats=False)


def timed_fusions(dst, grids, offs, reps):
    dst.fuse_from(grids, offs)                       # untimed: first touch
    dst.profile_reset()
    dst.profile(True, "fuse")
    for _ in range(reps):
        stats = dst.fuse_from(grids, offs)
    ms = np.sort(dst.profile_samples("fuse").astype(np.float64))
    dst.profile(False, "fuse")
    return stats, ms


def moved_bytes(grids, offs, dst, stats):
    """read: every cell of a member's initialised tile that lies inside the destination, once; written: the materialised tiles"""
    n = dst.cells
    read = 0
    for g, (ox, oy) in zip(grids, offs):
        init = g.download_tile_state()[0].reshape(g.cells // 32, g.cells // 32).astype(bool)
        ys, xs = np.nonzero(init)
        w = np.clip(np.minimum(xs * 32 + 32 + ox, n) - np.maximum(xs * 32 + ox, 0), 0, 32)
        h = np.clip(np.minimum(ys * 32 + 32 + oy, n) - np.maximum(ys * 32 + oy, 0), 0, 32)
        read += int((w * h).sum()) * CELL_BYTES
    return read, stats["tiles_materialised"] * F.CELLS * CELL_BYTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsd_fuse.txt"))
    ap.add_argument("--log2", type=int, default=12)
    ap.add_argument("--scans", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--members", type=int, nargs="*", default=[2, 8])
    a = ap.parse_args()
    gc = synth.GridConfig(a.log2, 0.025)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    host = facade.load_library()
    dst = capi.TsdGridDevice(a.log2, gc.cell_size, gc.max_trunc)
    best, mean = dst.measure_stream(1 << 25, 5)      # 2 x 256 MiB: beyond the Infinity Cache
    lines = [f"k_tsd_fuse: {dst.cells}^2 cells at {gc.cell_size} m ({dst.tiles} tiles, one workgroup each), {a.scans} scans per member, "
             f"{a.reps} timed launches per case", f"stream figure of this run (tsd_measure_stream, 2 x 256 MiB read + written): best {best:.0f} GB/s, mean {mean:.0f} GB/s", ""]
    for n in a.members:
        for name, step in (("0", (0, 0)), ("(17, -5) per member", (17, -5))):
            offs = [(step[0] * i, step[1] * i) for i in range(n)]
            grids = [capi.TsdGridDevice(a.log2, gc.cell_size, gc.max_trunc) for _ in range(n)]
            stats_e, ms_e = timed_fusions(dst, grids, offs, a.reps)          # empty members: the launch itself
            for r, g in enumerate(grids):
                push_scans(host, g, world, geo, r, a.scans, offs[r])
            stats, ms = timed_fusions(dst, grids, offs, a.reps)
            read, written = moved_bytes(grids, offs, dst, stats)
            med, med_e = float(np.median(ms)), float(np.median(ms_e))
            gbs = (read + written) / (med * 1e-3) / 1e9
            t0 = time.perf_counter()
            dumps = [g.download_tiles() for g in grids]
            t1 = time.perf_counter()
            want, _ = F.fuse_ref(dumps, offs, dst.cells)
            t2 = time.perf_counter()
            dst.upload_tiles(*want)
            t3 = time.perf_counter()
            del dumps
            # the uploaded restatement and the kernel's grid hold the same interiors (the upload leaves the halos to the next push)
            dst.fuse_from(grids, offs)
            got = dst.download_tiles()
            same = bool(np.array_equal(got[0], want[0]) and np.array_equal(np.nan_to_num(got[2][want[0] > 0], nan=9.0), np.nan_to_num(want[2][want[0] > 0], nan=9.0)))
            del got, want
            lines += [
                f"N = {n}, offsets {name}: {stats}",
                f"  kernel            median {med * 1e3:9.1f} us   min {ms[0] * 1e3:.1f}   max {ms[-1] * 1e3:.1f}   ({len(ms)} launches)",
                f"  empty members     median {med_e * 1e3:9.1f} us   min {ms_e[0] * 1e3:.1f}   max {ms_e[-1] * 1e3:.1f}   (the same launch with nothing to read or write)",
                f"  bytes             read {read / 1e6:.1f} MB (members' initialised tiles inside the destination) + written {written / 1e6:.1f} MB "
                f"(materialised tiles) -> {gbs:.0f} GB/s = {gbs / best:.2f} of the stream figure",
                f"  host route        download x {n} {t1 - t0:.2f} s + numpy restatement {t2 - t1:.2f} s + upload {t3 - t2:.2f} s = {t3 - t0:.2f} s"
                f"   -> kernel / host route = 1 / {(t3 - t0) / (med * 1e-3):.0f}   (same grid: {same})",
                ""]
            print("\n".join(lines[-6:]), flush=True)
            for g in grids:
                g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    dst.close()


if __name__ == "__main__":
    main()
