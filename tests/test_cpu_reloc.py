"""The relocalisation rules, restated in numpy (tests/reloc_ref.py), on an oracle-built grid: shows that the inputs the GPU tests
use are fair -- the score's best peak is next to the true pose and the registration from it ends on the true pose -- and pins the
peak rule and the bilinear look-up independently of the kernels (tests/test_gpu_reloc.py compares the device with this restatement)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import reloc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_best_peak_is_next_to_the_truth_and_icp_ends_on_it(oracle):
    """Pillars world, 512^2 cells of 0.05 m, 12 scans pushed at their true poses; the query scan (360 beams) is taken 0.93 m / 0.38 m
    off the start, never pushed, 11.4 / 11.7 / 12.3 steps inside the 24 x 24 x 36 lattice (0.1 m, 10 degrees), turned by 123 degrees
    against the trajectory.  Bounds: one lattice step for the best peak, half a step after the oracle's ray cast + ICP.
    Observed: best peak off by (-0.04 m, +0.03 m, 3.0 degrees), score 109977944 against 47796630 for the runner-up; after ICP
    0.0063 m and 0.23 degrees with 234 pairs."""
    sc = R.scene(360)
    assert abs(sc.truth[2] - sc.poses[:, 2].max()) > math.pi / 2
    assert all(math.hypot(p[0] - sc.truth[0], p[1] - sc.truth[1]) > 0.3 for p in sc.poses)
    vol, gate = R.scene_scores(360)
    assert vol.shape == (R.NTHETA, R.NXY, R.NXY) and gate.any()
    idx, score = R.peaks(vol, vol.shape, True, 16)
    assert len(idx) >= 2 and score[0] > score[1]
    pose = R.candidate_pose(idx[0], sc.x0, sc.y0, R.STEP, R.NXY, R.NXY, sc.table)
    yaw = math.atan2(pose[1, 0], pose[0, 0])
    dth = math.atan2(math.sin(yaw - sc.truth[2]), math.cos(yaw - sc.truth[2]))
    print(f"best peak off by {pose[0, 2] - sc.truth[0]:+.4f} m {pose[1, 2] - sc.truth[1]:+.4f} m {math.degrees(dth):+.2f} deg, scores {score[:2]}")
    assert abs(pose[0, 2] - sc.truth[0]) <= R.STEP and abs(pose[1, 2] - sc.truth[1]) <= R.STEP and abs(dth) <= R.DTHETA
    r = R.oracle_refine(sc, pose)
    assert r is not None
    final = oracle.mat3_mul(pose, r["T"])
    d, a = R.pose_error(final, sc.truth)
    print(f"after ICP: {d:.4f} m {math.degrees(a):.3f} deg, {r['pairs']} pairs")
    assert d <= 0.5 * R.STEP and a <= 0.5 * R.DTHETA


def test_bilinear_restatement_equals_the_oracle(oracle):
    sc = R.scene(360)
    rng = np.random.default_rng(11)
    W = sc.gc.width
    # over the whole grid and beyond its border, and dense where the map is
    x = np.concatenate([rng.uniform(-0.5, W + 0.5, 3000), rng.uniform(sc.truth[0] - 6, sc.truth[0] + 6, 3000)])
    y = np.concatenate([rng.uniform(-0.5, W + 0.5, 3000), rng.uniform(sc.truth[1] - 6, sc.truth[1] + 6, 3000)])
    st, v = sc.view.bilinear(x, y)
    seen = set()
    for i in range(x.size):
        so, vo = sc.grid.bilinear(float(x[i]), float(y[i]))
        assert so == st[i], (i, x[i], y[i])
        if so == R.SUCCESS:
            assert vo == v[i]
        seen.add(so)
    assert seen == {R.SUCCESS, R.INVALIDINDEX, R.EMPTYPARTITION, R.ISNAN}


@pytest.mark.parametrize("name", sorted(R.handmade_volumes()))
def test_peak_rule_on_handmade_volumes(name):
    vol, wraps, expect = R.handmade_volumes()[name]
    for K in (1, 5, 64):
        idx, score = R.peaks(vol, vol.shape, wraps, K)
        flat = vol.reshape(-1)
        assert len(idx) <= K and np.array_equal(score, flat[idx])
        keys = [(-int(s), int(i)) for i, s in zip(idx, score)]
        assert keys == sorted(keys) and len(set(idx.tolist())) == len(idx)
        if expect is not None:
            assert idx.tolist() == expect[:K]
    if name == "many_peaks":
        idx, _ = R.peaks(vol, vol.shape, wraps, 64)
        assert len(idx) == 64                      # 200 peaks in the volume
        all_idx, _ = R.peaks(vol, vol.shape, wraps, 10 ** 6)
        assert len(all_idx) == 200
    if name == "long_line":
        all_idx, _ = R.peaks(vol, vol.shape, wraps, 10 ** 7)
        assert len(all_idx) == 500000


def test_winner_rule():
    assert R.winner([]) == -1
    assert R.winner([5]) == 0
    assert R.winner([5, 9, 9, 3]) == 1             # the earlier peak keeps a tie
    assert R.winner([7, 7, 7]) == 0
    assert R.winner([0, 0]) == 0


def test_gate_zeroes_whole_columns_of_the_volume():
    vol, gate = R.scene_scores(1081)
    assert (~gate).any() and gate.any()            # the 270-degree scene has positions inside pillars / unseen space
    assert not vol[:, ~gate].any()
    assert vol[:, gate].max() > 0


def test_abi_of_the_relocalisation_calls(hip_lib):
    from ohm_tsd_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "tsd_hip.h")).read()
    for name in ("tsd_relocalize", "tsd_debug_reloc_scores", "tsd_debug_reloc_peaks"):
        assert re.search(r"int %s\(tsd_ctx\* ctx," % name, hdr) and name in capi.ABI and hasattr(hip_lib, name)
    assert hip_lib.tsd_abi_sizeof(b"tsd_reloc_params") == C.sizeof(capi.RelocParams)
    assert hip_lib.tsd_abi_sizeof(b"tsd_reloc_result") == C.sizeof(capi.RelocResult)
    assert capi.RelocResult.icp.offset % 8 == 0 and C.sizeof(capi.RelocParams) == 3 * 8 + 4 * 4 + 8 + 2 * 8 + 2 * 4
    # without a context every call is an argument error, on a box without a GPU too
    assert hip_lib.tsd_relocalize(None, None, None, 0, None, None, None, 0, 0.0, 0.0, None, None) == -1
    assert hip_lib.tsd_debug_reloc_scores(None, None, 0) == -1
    assert hip_lib.tsd_debug_reloc_peaks(None, None, 1, 1, 1, 0, 1, None, None, None) == -1
