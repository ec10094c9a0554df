"""The published map at its edges, CPU half: the oracle's occupancy / color_image against the restatement of tests/map_edges_ref.py.

The same case table and reuse sequence as tests/test_gpu_map_edges.py, so that a disagreement between the oracle and the restatement
shows without a GPU; where the two disagree the reference's text decides.  Every comparison is exact, and every case asserts from the
restatement alone that it reaches the edge it is named after (`reach`).
"""
import numpy as np
import pytest

from ohm_tsd_slam_amd import synth
from tests import helpers as H
from tests import map_edges_ref as R

CASES = R.table()


def _oracle_grid(oracle, log2, cs, arrays):
    og = oracle.Grid(log2, cs, 3 * cs)
    og.load(*arrays)
    return og


def _compare(og, ref, content, inflate, factor, what):
    """one extraction on both sides; the persistent maps must agree afterwards as well"""
    r_occ, r_n, info = ref.occupancy(*og.dump()[:3], inflate, factor)
    o_occ, o_n = og.occupancy(content, inflate, factor)
    N = ref.N
    print(f"{what}: n_surface restatement {r_n} oracle {o_n}, marked cells {(r_occ == 100).sum()} / {(o_occ == 100).sum()}")
    assert o_n == r_n, f"{what}: n_surface {o_n} != {r_n}"
    assert np.array_equal(o_occ.reshape(N, N), r_occ), f"{what}: {np.count_nonzero(o_occ.reshape(N, N) != r_occ)} cells differ"
    assert np.array_equal(content, ref.content), f"{what}: the persistent maps differ"
    return r_occ, r_n, info


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_oracle_equals_restatement(oracle, case):
    og = _oracle_grid(oracle, case.map_size_log2, case.cell_size, case.grid.arrays())
    ref = R.MapRef(case.map_size_log2, case.cell_size)
    content = np.full(ref.N * ref.N, -1, dtype=np.int8)
    results = [_compare(og, ref, content, inflate, factor, f"{case.name} inflate={inflate} factor={factor}")
               for inflate, factor in case.params]
    case.reach(case, results)
    assert np.array_equal(og.color_image(ref.N, ref.N), ref.color_image(*og.dump()[:3], ref.N, ref.N))


def test_first_row_column_corner_take_the_last_writer(oracle):
    """every combination of the four writers of a tile's first row / column / corner cell, on one persistent map"""
    ref = R.MapRef(7, 0.05)
    content = np.full(ref.N * ref.N, -1, dtype=np.int8)
    og = oracle.Grid(7, 0.05, 0.15)
    decided_by = set()
    for k, (g, present, signs) in enumerate(R.gather_steps()):
        before = int(ref.content[64 * ref.N + 64])
        og.load(*g.arrays())
        occ, n, info = _compare(og, ref, content, False, 2, f"gather step {k} {present} {signs}")
        assert n == 0
        assert occ[64, 64] == R.gather_expected_corner(present, signs, before), (k, present, signs)
        own, left, down, diag, own_empty = present
        if not own and not own_empty and left and down and signs[1] != signs[2]:
            assert occ[64, 64] == (0 if signs[1] > 0 else -1)          # left over down
            assert (occ[64, 65:96] == (0 if signs[2] > 0 else -1)).all() and (occ[65:96, 64] == (0 if signs[1] > 0 else -1)).all()
            decided_by.add("left>down")
        if not own and not own_empty and not left and down and diag and signs[2] != signs[3]:
            decided_by.add("down>diag")
        if not own and not own_empty and not left and not down and diag:
            decided_by.add("diag")
        if own and left and signs[0] != signs[1]:
            decided_by.add("own>left")
        if own_empty and (left or down or diag):
            assert (occ[64:96, 64:96] == 0).all()
            decided_by.add("empty>neighbours")
    assert decided_by == {"left>down", "down>diag", "diag", "own>left", "empty>neighbours"}


@pytest.mark.parametrize("width,height", R.IMAGE_SIZES)
def test_color_image_sizes(oracle, width, height):
    g = R.mixed_grid()
    og = _oracle_grid(oracle, 7, 0.05, g.arrays())
    ref = R.MapRef(7, 0.05)
    img = ref.color_image(*og.dump()[:3], width, height)
    assert img.shape == (height, width, 3)
    assert np.array_equal(og.color_image(width, height), img), f"{np.argwhere(og.color_image(width, height) != img)[:5]}"
    if width >= 100 and height >= 77:        # what the grid had to hold: green, red, white and black pixels
        s = img.reshape(-1, 3).astype(int)
        assert (s[:, 1] == 255).any() and ((s[:, 1] == 0) & (s[:, 0] > 0)).any() and (s.sum(axis=1) == 765).any() and (s.sum(axis=1) == 0).any()


def test_reuse_sequence(oracle, tmp_path):
    gc = synth.GridConfig(R.SEQ_LOG2, R.SEQ_CS)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    ref = R.MapRef(R.SEQ_LOG2, R.SEQ_CS)
    content = np.full(ref.N * ref.N, -1, dtype=np.int8)
    og = oracle.Grid(gc.map_size_log2, gc.cell_size, gc.max_trunc)
    text = tmp_path / "sparse.txt"
    reach = R.SequenceReach(ref)
    pushes = 0
    for k, (action, inflate, factor) in enumerate(R.SEQUENCE):
        if action in ("dense", "sparse"):
            og.load(*(R.dense_grid() if action == "dense" else R.sparse_grid()).arrays())
        elif action == "reset":                 # TsdGrid::reset: every partition as constructed (the oracle has no call for it)
            og.load(*R.TileGrid(R.SEQ_LOG2).arrays())
        elif action == "load_text":
            og = oracle.Grid.load_text(text, gc.cell_size)
            assert og is not None
        elif action == "push":
            pose, (x, y, yaw) = H.sensor_pose(world, 5 * pushes)
            data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), H.MAX_RANGE, geo.angle_increment)
            og.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL)
            pushes += 1
        before = ref.content.copy()
        occ, n, info = _compare(og, ref, content, inflate, factor, f"step {k} {action}")
        reach.record(k, action, inflate, factor, og.dump()[0], before, occ, n)
        if k == 1:
            assert og.store_text(text)
    reach.assert_reached()
