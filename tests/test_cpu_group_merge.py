"""The same-device merge group without a device: the properties of its numpy restatement (tests/group_merge_ref.py), the refusals
tsd_group_create makes before its first HIP call, libtsd_hip.so's independence of RCCL, and the origin-to-offset rule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, multigpu
from tests import group_merge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps(n, shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-128, 128, size=shape, dtype=np.int16).astype(np.int8) for _ in range(n)]


def test_one_member_at_zero_offset_is_the_identity():
    (m,) = _maps(1, (64, 64), 1)
    assert np.array_equal(R.merge([m]), m)
    assert np.array_equal(R.merge([m], [(0, 0)], 64, 64), m)


def test_equal_members_at_zero_offsets_are_the_elementwise_maximum():
    """the semantics tests/test_cpu_multigpu.py pins for the RCCL merge"""
    maps = _maps(5, (48, 48), 2)
    assert np.array_equal(R.merge(maps), np.maximum.reduce(maps))
    occ = [np.random.default_rng(s).choice(np.array([-1, 0, 100], dtype=np.int8), size=(32, 32)) for s in range(3)]
    m = R.merge(occ)
    assert np.array_equal(m, np.maximum.reduce(occ)) and R.n_occupied(m) == int((np.maximum.reduce(occ) == 100).sum())


def test_merge_is_commutative_in_member_order():
    maps = _maps(4, (32, 48), 3)
    offs = [(0, 0), (5, -3), (-17, 9), (16, 16)]
    a = R.merge(maps, offs)
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        assert np.array_equal(R.merge([maps[i] for i in perm], [offs[i] for i in perm]), a)


def test_uncovered_cells_are_unknown():
    a, b = np.full((16, 16), -128, np.int8), np.full((16, 16), 7, np.int8)
    m = R.merge([a, b], [(0, 0), (32, 0)])
    assert m.shape == (16, 48)
    assert (m[:, :16] == -128).all() and (m[:, 16:32] == -1).all() and (m[:, 32:] == 7).all()   # covered -128 stays -128


def test_window_clips_the_members():
    maps = _maps(2, (32, 32), 4)
    offs = [(-4, -6), (10, 20)]
    full = R.merge(maps, offs)                         # bounding box: corner (-4, -6)
    x0, y0, W, H = R.window([m.shape for m in maps], offs)
    assert (x0, y0, W, H) == (-4, -6, 46, 58)
    clip = R.merge(maps, offs, 24, 30)                 # explicit window: corner (0, 0)
    assert clip.shape == (30, 24)
    assert np.array_equal(clip, full[6:36, 4:28])


def test_group_create_refuses_bad_arguments_without_a_device(hip_lib, capfd):
    lib = hip_lib
    dummy = (C.c_void_p * 65)(*([1] * 65))             # never dereferenced: the count is checked first
    assert lib.tsd_group_create(0, dummy, None, 0, 0) is None
    assert lib.tsd_group_create(65, dummy, None, 0, 0) is None
    assert lib.tsd_group_create(-1, dummy, None, 0, 0) is None
    assert lib.tsd_group_create(2, None, None, 0, 0) is None
    null2 = (C.c_void_p * 2)(None, None)
    assert lib.tsd_group_create(2, null2, None, 0, 0) is None
    assert "tsd_group_create" in capfd.readouterr().err
    prm = capi.MapParams(0, 2)
    assert lib.tsd_group_merge_begin(None, C.byref(prm), None) == -1
    assert lib.tsd_group_merge_maps_begin(None, None, None) == -1
    assert lib.tsd_group_merge_wait(None, None) == -1
    assert lib.tsd_group_size(None) == 0 and lib.tsd_group_map_dev(None) is None
    with pytest.raises(capi.TsdError):
        multigpu.LocalOccupancyGroup([])


def test_cell_offsets_refuses_null_arguments_without_a_device(hip_lib):
    buf = (C.c_int32 * 4)()
    assert hip_lib.tsd_group_cell_offsets(None, buf) == -1            # TSD_E_ARG
    assert hip_lib.tsd_group_cell_offsets(None, None) == -1


def test_libtsd_hip_needs_no_rccl():
    """the group lives in libtsd_hip.so, and a single-GPU host still never maps RCCL: checked in a fresh interpreter that loads and
    binds the library (this process may have loaded libtsd_comm.so for other tests)"""
    code = ("from ohm_tsd_slam_amd import capi\n"
            "lib = capi.load_library()\n"
            "assert hasattr(lib, 'tsd_group_create')\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libtsd_hip.so' in maps\n"
            "assert 'librccl' not in maps, 'librccl is mapped'\n"
            "print('no rccl')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "no rccl" in out.stdout, out.stderr[-1500:]


@pytest.mark.parametrize("cells,cs,xa,xb,want", [(1024, 0.025, 0.0, 0.6, -24), (1024, 0.025, 0.6, 0.0, 24), (4096, 0.015, 0.0, -0.7 * 3, 140),
                                                 (512, 0.05, 0.37, 0.37, 0), (1024, 0.025, 0.0, 1e-9, 0)])
def test_origin_to_offset_rule(cells, cs, xa, xb, want):
    """x_offset moves a grid's origin to -(W / 2 + x_offset): a grid with the larger offset lies at the smaller origin"""
    oa, ob = R.map_origin(cells, cs, xa), R.map_origin(cells, cs, xb)
    assert R.cell_offset(ob, oa, cs) == want
    assert multigpu.cell_offset_from_origins(ob, oa, cs) == want


def test_origin_to_offset_rule_refuses_a_fraction_of_a_cell():
    oa, ob = R.map_origin(1024, 0.025, 0.0), R.map_origin(1024, 0.025, 0.61)      # 24.4 cells
    with pytest.raises(ValueError):
        R.cell_offset(ob, oa, 0.025)
    with pytest.raises(ValueError):
        multigpu.cell_offset_from_origins(ob, oa, 0.025)
