"""The merge group under rigid transforms without a device: the properties of its numpy restatement (tests/group_rigid_ref.py) -- at
whole-cell identity transforms it is the translation group's restatement, exact quarter turns are np.rot90, no occupied cell is lost
under any rotation, the footprint is one or two cells per axis, the bounding-box rule -- the fairness of the agreement measure on two
oracle-built maps, and the refusals tsd_group_create_rigid makes before it looks at a context."""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, multigpu
from tests import group_merge_ref as GR
from tests import group_rigid_ref as R

# the member sets of tests/test_gpu_group_merge.py's CASES up to 512^2 (restated): map_size_log2 per member, offsets, window
XS, YS = (0, 16, 32, 1, 17, -5), (0, 7, -40)


def _offsets(n, k0=0):
    return [(XS[(k0 + i) % len(XS)], YS[(k0 + i) % len(YS)]) for i in range(n)]


CASES = {
    "n1": ([9], [(0, 0)], (0, 0)),
    "n1_shifted_window": ([9], [(17, 7)], (512, 512)),
    "n2_aligned": ([9, 9], [(0, 0), (16, -40)], (0, 0)),
    "n2_unaligned": ([9, 9], [(1, 7), (-5, 0)], (0, 0)),
    "n3": ([9, 9, 9], _offsets(3, 1), (0, 0)),
    "n3_zero": ([9, 9, 9], [(0, 0)] * 3, (0, 0)),
    "n8": ([9] * 8, _offsets(8), (0, 0)),
    "mixed_sizes": ([8, 9, 8], [(0, 0), (17, -40), (32, 7)], (0, 0)),
    "mixed_sizes_far": ([8, 9], [(-5, 0), (300, 7)], (0, 0)),
    "window_smaller_than_box": ([9, 9, 9], [(-5, -40), (16, 7), (33, 0)], (400, 300)),
    "window_width_not_16": ([9, 9], [(1, 0), (17, 7)], (500, 410)),
}
CELL_SIZES = (0.01, 0.025, 0.037, 0.05)
ANGLES = [0.0, 1e-6, math.radians(7.3), math.radians(30.0), math.radians(45.0), math.radians(90.0), math.radians(123.4),
          math.radians(180.0), math.radians(-17.0)]


def _maps(logs, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-128, 128, size=(1 << l, 1 << l), dtype=np.int16).astype(np.int8) for l in logs]


@pytest.mark.parametrize("case", list(CASES))
def test_whole_cell_identity_transforms_are_the_translation_group(case):
    logs, offs, (W, H) = CASES[case]
    maps = _maps(logs, sum(map(ord, case)))
    want = GR.merge(maps, offs, W, H)
    box = GR.window([m.shape for m in maps], offs, W, H)
    for cs in CELL_SIZES:
        Ts = [R.shift(ox, oy, cs) for ox, oy in offs]
        assert R.window([m.shape for m in maps], Ts, cs, W, H) == box, cs
        got = R.merge(maps, Ts, cs, W, H)
        assert np.array_equal(got, want), f"cs = {cs}: {int((got != want).sum())} cells differ"


@pytest.mark.parametrize("cs", CELL_SIZES)
def test_exact_quarter_turns_are_rot90(cs):
    (m,) = _maps([7], 5)
    n = m.shape[0]
    for k, turns in ((0, 0), (1, -1), (2, 2), (3, 1)):       # a turn by +90 degrees of the map's content is np.rot90(m, -1) of the rows
        T = R.quarter_turn(k, n * cs)
        assert set(np.abs(T[:2, :2]).ravel()) == {0.0, 1.0}
        assert np.array_equal(R.merge([m], [T], cs, n, n), np.rot90(m, turns)), k
        assert R.window([m.shape], [T], cs) == (0, 0, n, n)


def _source():
    """256^2: axis-aligned walls one cell thick, an 8-connected diagonal wall, a lone cell; free elsewhere, unknown beyond a margin"""
    m = np.zeros((256, 256), dtype=np.int8)
    m[:8] = m[-8:] = -1
    m[40, 30:200] = 100
    m[60:220, 50] = 100
    m[200, 60:180] = 100
    d = np.arange(70, 160)
    m[d, d + 20] = 100
    m[120, 220] = 100
    return m


TRANSLATIONS = [(0.0, 0.0), (3.25, -2.5), (0.5, 0.25), (8.6240, -5.4360)]       # in cells: whole, cs/4 and cs/2 fractions, generic


@pytest.mark.parametrize("angle", ANGLES)
def test_no_occupied_cell_is_lost(angle):
    cs = 0.05
    m = _source()
    ky, kx = np.nonzero(m == 100)
    assert len(kx) > 400
    for fx, fy in TRANSLATIONS:
        T = R.rigid(angle, fx * cs, fy * cs)
        x0, y0, W, H = R.window([m.shape], [T], cs)
        out = R.merge([m], [T], cs)
        # where the centre of every occupied source cell lands
        px, py = (kx + 0.5) * cs, (ky + 0.5) * cs
        X = np.floor((T[0, 0] * px + T[0, 1] * py + T[0, 2]) / cs).astype(np.int64) - x0
        Y = np.floor((T[1, 0] * px + T[1, 1] * py + T[1, 2]) / cs).astype(np.int64) - y0
        assert (X >= 0).all() and (X < W).all() and (Y >= 0).all() and (Y < H).all()
        assert (out[Y, X] == 100).all(), f"{int((out[Y, X] != 100).sum())} occupied cells lost at {angle} rad, shift ({fx}, {fy}) cells"
        assert len(kx) <= R.n_occupied(out) <= 4 * len(kx)
        # the footprint: one or two cells per axis, everywhere
        xa, xb, ya, yb = R.footprint(T, cs, x0, y0, W, H)
        assert set(np.unique(xb - xa)) <= {0, 1} and set(np.unique(yb - ya)) <= {0, 1}
    if angle == 0.0:                                          # whole cells: one source cell each; a quarter cell off: the tie is a rule
        assert np.array_equal(R.merge([m], [R.rigid(0.0)], cs), m)


def test_bounding_box_rule():
    cs = 0.05
    sizes = [(256, 256), (512, 512)]
    for c in CELL_SIZES:
        for ox, oy in [(0, 0), (17, -40), (-5, 300), (399, -399)]:
            Ts = [R.shift(0, 0, c), R.shift(ox, oy, c)]
            assert R.window(sizes, Ts, c) == GR.window(sizes, [(0, 0), (ox, oy)])
    # rotated: the box holds every member's corners and is tight to a cell
    for angle in ANGLES:
        Ts = [R.rigid(0.0), R.rigid(angle, 1.234, -0.777)]
        x0, y0, W, H = R.window(sizes, Ts, cs)
        pts = []
        for (_, w), T in zip(sizes, Ts):
            for x in (0.0, w * cs):
                for y in (0.0, w * cs):
                    pts.append((T @ np.array([x, y, 1.0]))[:2] / cs)
        pts = np.array(pts)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        assert x0 <= lo[0] + 1e-6 and lo[0] < x0 + 1 + 1e-6 and y0 <= lo[1] + 1e-6 and lo[1] < y0 + 1 + 1e-6
        assert x0 + W >= hi[0] - 1e-6 and hi[0] > x0 + W - 1 - 1e-6 and y0 + H >= hi[1] - 1e-6 and hi[1] > y0 + H - 1 - 1e-6
    # an explicit window has its corner at frame cell (0, 0)
    assert R.window(sizes, [R.rigid(0.3), R.rigid(1.0, 5.0, 5.0)], cs, 500, 410) == (0, 0, 500, 410)


def test_uncovered_cells_are_unknown_and_the_maximum_is_signed():
    cs = 0.05
    a, b = np.full((16, 16), -128, np.int8), np.full((16, 16), 7, np.int8)
    m = R.merge([a, b], [R.rigid(0.0), R.rigid(0.0, 32 * cs, 0.0)], cs)
    assert m.shape == (16, 48)
    assert (m[:, :16] == -128).all() and (m[:, 16:32] == -1).all() and (m[:, 32:] == 7).all()
    # a member turned by 45 degrees leaves the box's corners uncovered
    t = R.merge([b], [R.rigid(math.radians(45.0))], cs)
    assert t[0, 0] == -1 and t[t.shape[0] // 2, t.shape[1] // 2] == 7 and set(np.unique(t)) == {-1, 7}


def _oracle_occupancy(sc, dump):
    from oracle import pyoracle as O
    g = O.Grid(sc.gc.map_size_log2, sc.gc.cell_size, sc.gc.max_trunc)
    g.load(*dump)
    occ, _ = g.occupancy(np.full(g.cells * g.cells, -1, dtype=np.int8))
    g.close()
    return occ.reshape(sc.cells, sc.cells)


def test_agreement_measure_discriminates(oracle):
    """Two oracle-built maps of one world (tests/align_ref.scene("diff"): 512^2 cells of 0.05 m, map A from poses 0-11, map B from poses
    6-17 pushed at D = 7.3 degrees + (0.43, -0.27) m): A's occupancy warped into B's frame by the restatement agrees with B's under D
    and not under a wrong transform.  Measured with the oracle's maps (the reference, not the code under test):
    1350 / 1358 = 0.994 under D, 1337 / 1347 = 0.993 under D perturbed by the alignment's own bound (half a cell, 1e-3 rad), 86 / 596 =
    0.144 under the identity.  The bound of 0.97 leaves 2.4 points for rasterisation differences."""
    from tests import align_ref as A
    sc = A.scene("diff")
    occ_a, occ_b = _oracle_occupancy(sc, sc.dump_a), _oracle_occupancy(sc, sc.dump_b)
    assert (occ_a == 100).sum() > 1000 and (occ_b == 100).sum() > 1000
    n = sc.cells

    def share(T):
        return R.agreement(occ_b, R.merge([occ_a], [T], sc.cs, n, n))

    good, wrong = share(sc.D), share(np.eye(3))
    th = math.atan2(sc.D[1, 0], sc.D[0, 0]) + 1e-3
    near = share(R.rigid(th, sc.D[0, 2] + 0.5 * sc.cs / math.sqrt(2.0), sc.D[1, 2] - 0.5 * sc.cs / math.sqrt(2.0)))
    print(f"agreement: {good[1]} / {good[2]} = {good[0]:.3f} under D, {near[1]} / {near[2]} = {near[0]:.3f} perturbed, "
          f"{wrong[1]} / {wrong[2]} = {wrong[0]:.3f} under the identity")
    assert good[2] > 1000 and wrong[2] > 300
    assert good[0] >= 0.97
    assert wrong[0] <= 0.5


def test_create_rigid_refuses_bad_arguments_without_a_device(hip_lib, capfd):
    lib = hip_lib
    dummy = (C.c_void_p * 65)(*([1] * 65))             # never dereferenced: the count is checked first
    assert lib.tsd_group_create_rigid(0, dummy, None, 0, 0) is None
    assert lib.tsd_group_create_rigid(65, dummy, None, 0, 0) is None
    assert lib.tsd_group_create_rigid(2, None, None, 0, 0) is None
    null2 = (C.c_void_p * 2)(None, None)
    assert lib.tsd_group_create_rigid(2, null2, None, 0, 0) is None
    assert "tsd_group_create_rigid" in capfd.readouterr().err
    T = (C.c_double * 9)()
    assert lib.tsd_group_member_transform(None, 0, T) == -1
    with pytest.raises(capi.TsdError):
        multigpu.LocalOccupancyGroup([], transforms=[])
    with pytest.raises(capi.TsdError, match="exclusive"):
        multigpu.LocalOccupancyGroup([], cell_offsets=[], transforms=[])
