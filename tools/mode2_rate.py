#!/usr/bin/env python3
"""registration_mode 2 (PDFMatching pre-registration + ICP) through the C++ façade at cfg 2 with a fixed seed: scans per second of
the synchronous node, the pre-registration's phases in us per match (tsd_pdf_match's own timing, TSD_MODE2_TIMING: normals, host
lists, staging, and the device's model arrays / scoring / arg-max by HIP events) and, for comparison, the plain-C restatement of
PDFMatching::match (tests/pdfmatch_restate.c, one thread) in ms per match on the same inputs.  --mode 1: the same for
registration_mode 1 (RandomNormalMatching: tsd_rn_match, TSD_MODE1_TIMING, scoring / selection; tests/rnmatch_restate.c).

    python tools/mode2_rate.py [--mode {1,2}] [--scans N] [--warmup W] [--dump DIR]

--dump DIR: every scan's pose and lastPreregistration record as raw float64 rows in DIR/mode<m>.bin (two builds with the same seed are
compared bytewise) and nothing else: no timing lines, no restatement.
"""
import argparse
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ohm_tsd_slam_amd import capi, facade, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--mode", type=int, choices=(1, 2), default=2)
    ap.add_argument("--dump", metavar="DIR", default=None)
    a = ap.parse_args()
    if not a.dump:
        os.environ.setdefault(f"TSD_MODE{a.mode}_TIMING", "1")      # (read once, at the first tsd_pdf_match / tsd_rn_match)
    gc, geo, scene = synth.CONFIGS["cfg2"]
    world = synth.World(scene, gc)
    n = a.warmup + a.scans
    scans = synth.scans_for(world, geo, synth.trajectory(world, n))
    params = facade.node_params(gc, geo)
    params.update({"registration_mode": a.mode, "tsdpdf_seed": a.seed})
    node = facade.SlamNode(params, synchronous=True)
    if a.dump:
        rows = []
        for k in range(n):
            node.laser(scans[k], geo.angle_min, geo.angle_increment)
            pr = node.preregistration() or dict(T=np.zeros((3, 3)), prob=0.0, idx=0, i=0, candidates=0, valid_model=0, valid_scene=0, control=0)
            rows.append(np.concatenate([node.report()["pose"].ravel(), pr["T"].ravel(),
                                        [pr[key] for key in ("prob", "idx", "i", "candidates", "valid_model", "valid_scene", "control")]]))
        os.makedirs(a.dump, exist_ok=True)
        np.asarray(rows, dtype=np.float64).tofile(os.path.join(a.dump, f"mode{a.mode}.bin"))
        print(f"mode {a.mode}: {n} scans dumped to {a.dump}", flush=True)
        node.close()
        return
    for k in range(a.warmup):
        node.laser(scans[k], geo.angle_min, geo.angle_increment)
    sys.stderr.flush()
    t0 = time.perf_counter()
    for k in range(a.warmup, n):
        node.laser(scans[k], geo.angle_min, geo.angle_increment)
    dt = time.perf_counter() - t0
    sys.stderr.flush()
    pr = node.preregistration()
    rep = node.report()
    e = math.hypot(rep["pose"][0, 2] - synth.trajectory(world, n)[-1, 0], rep["pose"][1, 2] - synth.trajectory(world, n)[-1, 1])
    print(f"mode {a.mode}, cfg 2 ({geo.beams} beams), {a.scans} scans after {a.warmup}: {a.scans / dt:.0f} scans/s ({1e6 * dt / a.scans:.1f} us per scan), "
          f"last pre-registration: {pr['candidates']} candidates, {pr['control']} control points, {pr['valid_model']} model points; "
          f"tracking error {e:.4f} m", flush=True)
    # the restatement, single-threaded, on the last scan's inputs as the facade's ray cast gives them
    if a.mode == 1:
        from tests import rnmatch_ref as R
    else:
        from tests import pdfmatch_ref as R
    from tests import helpers as H
    from oracle import pyoracle as O
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        rs = R.Restatement(R.build(tmp))
        g = node.grid()
        pose = rep["pose"]
        rl, rw = H.world_rays(O, geo, pose, gc.cell_size)
        co, no, mo, cnt = g.raycast(pose, rw, H.MIN_RANGE, H.MAX_RANGE)
        data, mask = O.ingest_f32(scans[-1], H.MAX_RANGE, geo.angle_increment)
        sc, ms, _ = O.scene_from_scan(rl, data, mask)
        rng = np.random.default_rng(a.seed)
        ds, dc, dt_ = (rng.integers(0, 2 ** 31 - 1, k) for k in (geo.beams, 140, 100))
        phi = 30.0 * math.pi / 180.0
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            rr = rs.match(co, mo, sc, ms, phi, geo.angle_increment, ds, dc, dt_)
        tr = (time.perf_counter() - t0) / reps
        dg = capi.TsdGridDevice(9, 0.05, 0.15)
        match = dg.rn_match if a.mode == 1 else dg.pdf_match
        for _ in range(3):
            rh = match(co, mo, sc, ms, phi, geo.angle_increment, ds, dc, dt_)
        t0 = time.perf_counter()
        for _ in range(50):
            rh = match(co, mo, sc, ms, phi, geo.angle_increment, ds, dc, dt_)
        th = (time.perf_counter() - t0) / 50
        same = (rh["candidates"], rh["idx"], rh["i"]) == (rr["candidates"], rr["idx"], rr["i"])
        print(f"one match on the last scan's inputs ({rr['candidates']} candidates): restatement {1e3 * tr:.1f} ms (one CPU thread), "
              f"{'tsd_rn_match' if a.mode == 1 else 'tsd_pdf_match'} {1e6 * th:.1f} us end to end; same winner: {same}", flush=True)
        dg.close()
    node.close()


if __name__ == "__main__":
    main()
