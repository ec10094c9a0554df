"""The map-alignment rules, restated in numpy (tests/align_ref.py), on oracle-built grids: shows that the scenes the GPU tests use are
solvable by the rules of include/tsd_hip.h (tsd_align_points / tsd_map_align), pins the half-cell offset between the surface list and the
field, and checks the gain rule, the winner rule and the whole-cell shift independently of the kernels (tests/test_gpu_align.py compares
the device with this restatement).

Errors are against D, the transform map B was built with: metres = the largest |T p - D p| over the centre and the corners of the grid,
radians = the angle between the rotations (align_ref.map_error).

Measured with this restatement (512^2 cells of 0.05 m, pillars, 360 beams, 1 873 surface points, K = 16, the winner of the 16 peaks):
    self    7.2e-8 m, 5.9e-11 rad, rms 9.1e-8 m, converged in 16 steps
    same    1.3e-3 m, 5.5e-5 rad, rms 0.0116 m, 18 steps
    diff    2.9e-3 m, 5.9e-5 rad, rms 0.0145 m, 18 steps
    cells   2.5e-3 m, 2.5e-5 rad, cell_off (16, -7), cell_error 0.051
    self with the raw list (no half-cell correction): translation (0.02499998, 0.02499986) m = cs/2 within 1.4e-7 m, -2.6e-9 rad
    gain rule off, self, both leading peaks: steps of 2.1e-3 .. 2.3e-3 m (lever metric 0.017 .. 0.018) after 60 iterations, not converged
    a start 1.2 m and 40 degrees off the truth (diff): sum w = 45.2 against 1 109.3 for the true basin
"""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import align_ref as A
from tests import reloc_ref as R


def _winner(name, points="staged"):
    sc = A.scene(name)
    idx, sco, recs = A.scene_records(name, points)
    w = A.winner(recs)
    assert w >= 0
    return sc, recs[w], A.transform(recs[w], sc.pivot), recs


def test_self_alignment_is_the_identity():
    sc, rec, T, _ = _winner("self")
    d, a = A.map_error(T, sc.D, sc.side)
    rms = math.sqrt(rec["sums"][10] / rec["sums"][9])
    print(f"self: {d:.3g} m, {a:.3g} rad, rms {rms:.3g} m, {rec['iterations']} steps")
    assert rec["status"] == A.CONVERGED
    assert d <= 1e-5 and a <= 1e-6
    assert rms <= 1e-5


@pytest.mark.parametrize("name", ["same", "diff"])
def test_alignment_finds_the_transform(name):
    sc, rec, T, _ = _winner(name)
    d, a = A.map_error(T, sc.D, sc.side)
    print(f"{name}: {d:.3g} m, {a:.3g} rad, {rec['iterations']} steps, sum w {rec['sums'][9]:.1f}")
    assert rec["status"] == A.CONVERGED
    assert d <= 0.5 * sc.cs and a <= 1e-3        # two maps rasterised differently do not encode D more finely than half a cell


def test_the_list_sits_half_a_cell_below_the_field():
    """calcCoords places a crossing between cells px-1 and px at (px - 1 + interp) * cs, interpolateBilinear a cell's value at
    (px + 0.5) * cs: the list as tsd_surface_* gives it is carried onto its own field by a shift of (+cs/2, +cs/2)"""
    sc, rec, T, _ = _winner("self", "raw")
    print(f"raw list: translation ({T[0, 2]:.8f}, {T[1, 2]:.8f}), angle {math.atan2(T[1, 0], T[0, 0]):.3g}")
    assert rec["status"] == A.CONVERGED
    side = sc.side
    for px, py in ((0.0, 0.0), (side, 0.0), (0.0, side), (side, side)):
        q = T @ np.array([px, py, 1.0])
        assert abs(q[0] - px - 0.5 * sc.cs) <= 1e-5 and abs(q[1] - py - 0.5 * sc.cs) <= 1e-5


def test_whole_cell_shift():
    sc, rec, T, _ = _winner("cells")
    off, err = A.cell_shift(T, sc.cs, sc.cells)
    print(f"cells: cell_off {off}, cell_error {err:.3g}")
    # tsd_fuse: member cell (x, y) is dst's cell (x + ox, y + oy); B's scans were pushed 16 cells right and 7 down of A's
    assert off == A.CELLS_SHIFT
    assert err < 0.5
    # a rotated transform is not a whole-cell shift
    sc2, _, T2, _ = _winner("diff")
    assert A.cell_shift(T2, sc2.cs, sc2.cells)[1] > 0.5


def test_winner_rule_picks_the_true_basin():
    sc, rec, T, recs = _winner("diff")
    th = sc.truth[2] + math.radians(40.0)
    wrong = A.refine(sc.view_b, sc.points, sc.pivot, (sc.truth[0] + 1.0, sc.truth[1] + 0.7), math.cos(th), math.sin(th), A.ITERATIONS,
                     sc.max_trunc, sc.lever)
    print(f"wrong basin: sum w {wrong['sums'][9]:.1f} against {rec['sums'][9]:.1f}")
    assert wrong["sums"][9] < 0.5 * rec["sums"][9]
    lineup = [wrong] + list(recs)
    assert A.winner(lineup) >= 1
    d, a = A.map_error(A.transform(lineup[A.winner(lineup)], sc.pivot), sc.D, sc.side)
    assert d <= 0.5 * sc.cs and a <= 1e-3
    # degenerate records never win, the earlier record keeps a tie
    assert A.winner([dict(status=A.DEGENERATE, sums=[0] * 9 + [9e9, 0])] + list(recs[:1])) == 1
    assert A.winner([recs[0], recs[0]]) == 0
    assert A.winner([]) == -1


def test_gain_rule():
    sc = A.scene("self")
    idx, _, recs = A.scene_records("self")
    m, c, s = A.start_of(sc, idx[0])
    off = A.refine(sc.view_b, sc.points, sc.pivot, m, c, s, 60, sc.max_trunc, sc.lever, gain_rule=False)
    print(f"gain rule off: last step {off['steps'][-1]}, on: {recs[0]['iterations']} steps, gain {recs[0]['gain']}")
    assert off["status"] == A.MAXITER and off["iterations"] == 60
    assert max(off["steps"][-1]) > 100.0 * A.EPS          # the two-cycle on the kinks of the bilinear field
    assert recs[0]["status"] == A.CONVERGED and recs[0]["gain"] < 1.0


def test_degenerate_and_zero_iterations():
    sc = A.scene("self")
    m, c, s = A.start_of(sc, A.scene_records("self")[0][0])
    r = A.refine(sc.view_b, sc.points[:2], sc.pivot, m, c, s, 10, sc.max_trunc, sc.lever)
    assert r["status"] == A.DEGENERATE and r["iterations"] == 0
    far = sc.points * 0.0 + 0.3                            # unseen space: every look-up fails
    assert A.refine(sc.view_b, far, (0.3, 0.3), (0.3, 0.3), 1.0, 0.0, 10, sc.max_trunc, sc.lever)["status"] == A.DEGENERATE
    r = A.refine(sc.view_b, sc.points, sc.pivot, m, c, s, 0, sc.max_trunc, sc.lever)
    assert r["status"] == A.MAXITER and r["iterations"] == 0 and r["m"] == m and (r["c"], r["s"]) == (c, s)
    assert A.solve([1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]) is None
    assert A.solve([2.0, 0.0, 0.0, 4.0, 0.0, 8.0, 2.0, 4.0, 8.0]) == (1.0, 1.0, 1.0)


def test_scores_have_no_gate_and_take_the_pivot():
    """the coarse score equals tsd_relocalize's sum (reloc_ref.scores) wherever that one's gate passes, for points given relative to the
    pivot -- and is not zeroed where it does not"""
    sc = A.scene("diff")
    vol = A.scene_scores("diff")
    rel, stride = A.coarse_points(sc.points, sc.pivot)
    assert stride == 1 and len(rel) == len(sc.points)
    ref, gate = R.scores(sc.view_b, rel, sc.x0, sc.y0, A.STEP, A.NXY, A.NXY, sc.table)
    assert gate.any() and not gate.all()
    assert np.array_equal(vol[:, gate], ref[:, gate])
    assert vol[:, ~gate].any()
    assert A.coarse_points(np.zeros((2049, 2)), (0.0, 0.0))[1] == 2 and len(A.coarse_points(np.zeros((4097, 2)), (0.0, 0.0))[0]) == 1366


def test_abi_of_the_alignment_calls(hip_lib):
    for name in ("tsd_align_points", "tsd_map_align", "tsd_debug_align_scores", "tsd_debug_align_peaks", "tsd_debug_align_sums"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.tsd_abi_sizeof(b"tsd_align_params") == C.sizeof(capi.AlignParams) == 128
    assert hip_lib.tsd_abi_sizeof(b"tsd_align_peak") == C.sizeof(capi.AlignPeak) == 152
    assert hip_lib.tsd_abi_sizeof(b"tsd_align_result") == C.sizeof(capi.AlignResult) == 248
    # null arguments are refused before anything else is looked at
    assert hip_lib.tsd_align_points(None, None, None, 0, 0, None) == -1
    assert hip_lib.tsd_map_align(None, None, None, None) == -1
    assert hip_lib.tsd_debug_align_scores(None, None, 0) == -1
    assert hip_lib.tsd_debug_align_peaks(None, None, 0) == -1
    assert hip_lib.tsd_debug_align_sums(None, None, 0, None, None, 1.0, 0.0, 0.75, None, None) == -1
