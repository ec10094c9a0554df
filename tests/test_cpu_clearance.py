"""The clearance field's restatement (tests/clearance_ref.py) against an independent brute force, its Euclidean cut-off, the window
rule the windowed cost map relies on, the cost rule on unknown cells, and tsd_costmap_table through the library (host code: it runs
without a GPU)."""
import ctypes as C

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi
from tests import clearance_ref as R_

_i8p = C.POINTER(C.c_int8)


def brute_dist2(src, R):
    """min over ALL obstacle cells, written without the separable form"""
    H, W = src.shape
    oy, ox = np.nonzero(src == 100)
    out = np.full((H, W), 0xFFFF, dtype=np.uint16)
    if oy.size == 0:
        return out
    ys, xs = np.mgrid[0:H, 0:W]
    d = (xs[..., None] - ox[None, None, :]) ** 2 + (ys[..., None] - oy[None, None, :]) ** 2
    m = d.min(axis=2)
    out[m <= R * R] = m[m <= R * R].astype(np.uint16)
    return out


def random_map(rng, H, W, density):
    src = rng.choice(np.array([-1, 0], dtype=np.int8), size=(H, W))
    if density == "one":
        src[rng.integers(H), rng.integers(W)] = 100
    elif density == "all":
        src[:] = 100
    elif density > 0:
        src[rng.random((H, W)) < density] = 100
    return src


@pytest.mark.parametrize("R", [1, 2, 5, 13])
@pytest.mark.parametrize("density", [0, "one", 1e-2, 0.3, "all"])
def test_restatement_equals_brute_force(R, density):
    rng = np.random.default_rng(1000 + R)
    for H, W in ((37, 48), (1, 30), (19, 1), (32, 33)):
        src = random_map(rng, H, W, density)
        assert np.array_equal(R_.dist2(src, R), brute_dist2(src, R)), (H, W, R, density)


def test_restatement_equals_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    src = np.zeros((256, 256), dtype=np.int8)
    src[rng.random(src.shape) < 2e-4] = 100
    src[200, 17] = 100
    edt = ndi.distance_transform_edt(src != 100)
    want = np.rint(edt * edt).astype(np.int64)
    got = R_.dist2(src, 255).astype(np.int64)
    near = want <= 255 * 255
    assert np.array_equal(got[near], want[near]) and np.all(got[~near] == 0xFFFF)


def test_cutoff_is_euclidean():
    for R in (5, 13):
        src = np.zeros((64, 64), dtype=np.int8)
        src[30, 30] = 100
        d = R_.dist2(src, R)
        assert d[30 + R, 30] == R * R and d[30, 30 - R] == R * R          # (0, R) counts
        assert d[30 + R, 31] == 0xFFFF                                     # R^2 + 1 does not
    d = R_.dist2(src, 5)
    assert d[34, 33] == 25            # (3, 4)
    assert d[31, 35] == 0xFFFF        # (5, 1): inside the square, outside the circle
    assert d[30, 30] == 0


def test_costmap_table_through_the_library(hip_lib):
    total = same = 0
    for cs, R, ins, k in ((0.025, 22, 0.25, 10.0), (0.05, 11, 0.25, 10.0), (0.1, 255, 0.3, 0.5), (0.025, 64, 0.0, 3.0), (0.025, 1, 1.0, 10.0)):
        t = np.zeros(R * R + 1, dtype=np.int8)
        assert hip_lib.tsd_costmap_table(cs, R, ins, k, t.ctypes.data_as(_i8p)) == 0
        want = R_.table(cs, R, ins, k)
        d = np.sqrt(np.arange(R * R + 1)) * cs
        assert t[0] == 100
        assert np.all(t[1:][d[1:] <= ins] == 99) and np.all(t[1:][d[1:] > ins] <= 98)
        assert np.all(np.diff(t.astype(int)) <= 0) and t.min() >= 1
        assert np.all(np.abs(t.astype(int) - want.astype(int)) <= 1)
        total += t.size
        same += int(np.count_nonzero(t == want))
        assert np.array_equal(capi.costmap_table(cs, R, ins, k), t)
    print(f"tsd_costmap_table: {same} of {total} entries equal the numpy formula")
    assert same >= 0.99 * total
    t = np.zeros(4, dtype=np.int8)
    assert hip_lib.tsd_costmap_table(0.025, 0, 0.25, 10.0, t.ctypes.data_as(_i8p)) == -1
    assert hip_lib.tsd_costmap_table(0.025, 256, 0.25, 10.0, t.ctypes.data_as(_i8p)) == -1
    assert hip_lib.tsd_costmap_table(0.025, 1, 0.25, 10.0, None) == -1
    with pytest.raises(capi.TsdError):
        capi.costmap_table(0.025, 256)


@pytest.mark.parametrize("R", [1, 7, 40])
def test_window_grown_by_radius_gives_the_full_recomputation(R):
    rng = np.random.default_rng(50 + R)
    tab = R_.table(0.05, R, 0.25, 4.0)
    for _ in range(6):
        old = random_map(rng, 96, 96, 0.02)
        x, y = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        w, h = int(rng.integers(1, 96 - x + 1)), int(rng.integers(1, 96 - y + 1))
        new = old.copy()
        new[y:y + h, x:x + w] = random_map(rng, h, w, 0.05)
        d_old, c_old = R_.both(old, R, tab)
        d_new, c_new = R_.both(new, R, tab)
        g = R_.grown((x, y, w, h), R, 96, 96)
        assert np.array_equal(R_.patch(d_old, d_new, g), d_new)
        assert np.array_equal(R_.patch(c_old, c_new, g), c_new)
    assert R_.grown((3, 90, 10, 6), 7, 96, 96) == (0, 83, 20, 13)
    assert R_.grown((5, 5, 0, 0), 7, 96, 96) == (0, 0, 0, 0)


def test_cost_rule_on_unknown_cells():
    R = 6
    tab = np.zeros(R * R + 1, dtype=np.int8)
    tab[:] = 40
    tab[0], tab[1:5] = 100, 99                   # d2 1, 2, 4: the inscribed band
    src = np.full((20, 20), -1, dtype=np.int8)
    src[10, 10] = 100
    src[10, 14] = 0
    src[3, 3] = 77
    d2 = R_.dist2(src, R)
    c = R_.cost_from(src, d2, tab, R)
    assert c[10, 10] == 100
    assert c[10, 11] == 99 and c[11, 11] == 99 and c[10, 12] == 99      # unknown inside the band becomes 99
    assert c[10, 13] == -1 and d2[10, 13] == 9                           # unknown beyond it stays unknown
    assert c[10, 14] == 40                                               # free takes the table's cost
    assert c[3, 3] == 77 and d2[3, 3] == 0xFFFF                          # beyond R: the source
    assert c[0, 19] == -1
    src[10, 13] = 50
    assert R_.cost_from(src, d2, tab, R)[10, 13] == 50                   # max(s, c)


def test_abi_struct_sizes(hip_lib):
    assert hip_lib.tsd_abi_sizeof(b"tsd_costmap_params") == C.sizeof(capi.CostmapParams) == 24
    assert hip_lib.tsd_abi_sizeof(b"tsd_map_window") == C.sizeof(capi.MapWindow) == 16
