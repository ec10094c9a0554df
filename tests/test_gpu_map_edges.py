"""The published map at its edges, on the device: borders, seams, inflation factors, reuse of the context between calls.

Every map a consumer can get -- tsd_occupancy, the caller's device buffer filled by tsd_occupancy_dev, the frame of tsd_map_frame_begin / _wait -- and
the colour image are compared byte for byte with the restatement of tests/map_edges_ref.py (the reference's loops in plain Python) and
with the oracle, on hand-built grids whose sign changes sit exactly where the index arithmetic of occupancy_kernels.hip,
occupancy_device.hpp and map_publish.hip has its edges.  The case table and the sequence are those of tests/test_cpu_map_edges.py; each
case asserts from the restatement alone that it reaches what it is named after (`reach`).

Where the reference writes past the end of its map (inflation above the top row) the restatement drops the write; that the device and
the oracle do the same is asserted here, not assumed.  The persistent map is the reference's _occGridContent: -1 when the context is
created and cleared by nothing afterwards, tsd_reset included.
"""
import ctypes as C
import os

import numpy as np
import pytest

from ohm_tsd_slam_amd import capi, synth
from tests import helpers as H
from tests import map_edges_ref as R

pytestmark = pytest.mark.gpu

CASES = R.table()
KINDS = ("occupancy", "occupancy_into", "map_frame")


def _hip_runtime():
    """the HIP runtime the device library is linked against, as this process has it mapped.  (A torch tensor's data_ptr() would do as
    the caller's buffer in a process of its own; inside this one the torch wheel's bundled runtime and the library's do not mix.)"""
    capi.load_library()
    paths = []
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64.so" in os.path.basename(path) and path not in paths:
                paths.append(path)
    own = [q for q in paths if "torch" not in q]
    assert own, f"no HIP runtime mapped beside torch's: {paths}"
    hip = C.CDLL(own[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipSetDevice.argtypes = [C.c_int]
    for fn in (hip.hipMalloc, hip.hipFree, hip.hipMemset, hip.hipMemcpy, hip.hipSetDevice, hip.hipDeviceSynchronize):
        fn.restype = C.c_int
    return hip


class DeviceBuffer:
    """`nbytes` of device memory that belong to the test, not to the context (what tsd_occupancy_dev is for)"""

    def __init__(self, nbytes):
        self.hip, self.nbytes = _hip_runtime(), nbytes
        p = C.c_void_p()
        assert self.hip.hipSetDevice(0) == 0 and self.hip.hipMalloc(C.byref(p), nbytes) == 0 and p.value
        self.ptr = p.value

    def fill(self, byte):
        assert self.hip.hipMemset(self.ptr, byte, self.nbytes) == 0 and self.hip.hipDeviceSynchronize() == 0

    def to_host(self):
        out = np.zeros(self.nbytes, dtype=np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0          # hipMemcpyDeviceToHost
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            self.hip.hipFree(self.ptr)
            self.ptr = None


class Trio:
    """one device context, an oracle grid that is given the device grid's content, and the restatement, each with its own persistent map"""

    def __init__(self, oracle, log2, cs):
        self.dg = capi.TsdGridDevice(log2, cs, 3 * cs)
        self.og = oracle.Grid(log2, cs, 3 * cs)
        self.ref = R.MapRef(log2, cs)
        self.N = self.ref.N
        self.content = np.full(self.N * self.N, -1, dtype=np.int8)
        self._buf = None

    def tiles(self):
        t = self.dg.download_tiles()
        self.og.load(*t)
        return t

    def _into(self, inflate, factor):
        """tsd_occupancy_dev into a device buffer of the caller's, pre-filled with 7 so that every byte has to be written"""
        n = self.N * self.N
        if self._buf is None:
            self._buf = DeviceBuffer(n)
        self._buf.fill(7)
        self.dg.occupancy_into(self._buf.ptr, inflate, factor)
        return self._buf.to_host().view(np.int8).reshape(self.N, self.N)

    def call(self, kind, inflate, factor, what, tiles=None):
        """one extraction on the device (by `kind`), the oracle and the restatement; -> the restatement's (map, n, info)"""
        N = self.N
        tiles = self.tiles() if tiles is None else tiles
        r_occ, r_n, info = self.ref.occupancy(*tiles[:3], inflate, factor)
        o_occ, o_n = self.og.occupancy(self.content, inflate, factor)
        rgb, d_n = None, None
        if kind == "occupancy":
            d_occ, d_n = self.dg.occupancy(inflate, factor)
        elif kind == "occupancy_into":
            d_occ = self._into(inflate, factor)
        else:
            d_occ, rgb, d_n = self.dg.map_frame(inflate=inflate, factor=factor, image=True)
        print(f"{what} [{kind}]: n_surface restatement {r_n} oracle {o_n} device {d_n}; cells differing from the restatement: "
              f"device {np.count_nonzero(d_occ != r_occ)} oracle {np.count_nonzero(o_occ.reshape(N, N) != r_occ)}")
        assert o_n == r_n, f"{what}: oracle n_surface {o_n} != {r_n}"
        assert d_n is None or d_n == r_n, f"{what} [{kind}]: device n_surface {d_n} != {r_n}"
        assert d_occ.shape == (N, N) and d_occ.dtype == np.int8
        assert np.array_equal(d_occ, r_occ), f"{what} [{kind}]: {np.count_nonzero(d_occ != r_occ)} cells differ at {np.argwhere(d_occ != r_occ)[:5]}"
        assert np.array_equal(o_occ.reshape(N, N), r_occ), f"{what}: oracle differs at {np.argwhere(o_occ.reshape(N, N) != r_occ)[:5]}"
        assert np.array_equal(self.content, self.ref.content), f"{what}: the oracle's persistent map differs"
        if rgb is not None:
            r_img = self.ref.color_image(*tiles[:3], N, N)
            assert np.array_equal(rgb, r_img), f"{what}: the frame's image differs at {np.argwhere(rgb != r_img)[:5]}"
            assert np.array_equal(self.og.color_image(N, N), r_img), f"{what}: the oracle's image differs"
        return r_occ, r_n, info


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_every_path_equals_restatement_and_oracle(oracle, case):
    t = Trio(oracle, case.map_size_log2, case.cell_size)
    t.dg.upload_tiles(*case.grid.arrays())
    tiles = t.tiles()
    assert np.array_equal(tiles[0], case.grid.init) and np.array_equal(tiles[2][tiles[0] != 0], case.grid.tsd[case.grid.init != 0], equal_nan=True)
    results = []
    for inflate, factor in case.params:
        per_kind = [t.call(kind, inflate, factor, f"{case.name} inflate={inflate} factor={factor}", tiles) for kind in KINDS]
        results.append(per_kind[0])
    case.reach(case, results)
    assert np.array_equal(t.dg.color_image(t.N, t.N), t.ref.color_image(*tiles[:3], t.N, t.N))


def test_first_row_column_corner_take_the_last_writer(oracle):
    """every combination of the four writers of a tile's first row / column / corner cell (own > left > down > diagonal: the last
    writer of the reference's serial tile order), on one context whose map persists from step to step; the path rotates"""
    t = Trio(oracle, 7, 0.05)
    decided_by = set()
    for k, (g, present, signs) in enumerate(R.gather_steps()):
        before = int(t.ref.content[64 * t.N + 64])
        t.dg.upload_tiles(*g.arrays())
        occ, n, info = t.call(KINDS[k % 3], False, 2, f"gather step {k} {present} {signs}")
        assert n == 0
        assert occ[64, 64] == R.gather_expected_corner(present, signs, before), (k, present, signs)
        own, left, down, diag, own_empty = present
        if not own and not own_empty and left and down and signs[1] != signs[2]:
            decided_by.add("left>down")
        if not own and not own_empty and not left and down and diag and signs[2] != signs[3]:
            decided_by.add("down>diag")
        if not own and not own_empty and not left and not down and diag:
            decided_by.add("diag")
        if own and left and signs[0] != signs[1]:
            decided_by.add("own>left")
        if own_empty and (left or down or diag):
            decided_by.add("empty>neighbours")
    assert decided_by == {"left>down", "down>diag", "diag", "own>left", "empty>neighbours"}


def test_color_image_sizes(oracle):
    """width / height 1, several pixels per cell, widths that are and are not multiples of the 256-thread block"""
    g = R.mixed_grid()
    t = Trio(oracle, 7, 0.05)
    t.dg.upload_tiles(*g.arrays())
    tiles = t.tiles()
    assert any(w % 256 == 0 for w, _ in R.IMAGE_SIZES) and any(w % 256 not in (0, 1) and w > 256 for w, _ in R.IMAGE_SIZES)
    assert any(w == 1 for w, _ in R.IMAGE_SIZES) and any(h == 1 for _, h in R.IMAGE_SIZES) and any(w > t.N and h > t.N for w, h in R.IMAGE_SIZES)
    for width, height in R.IMAGE_SIZES + R.IMAGE_SIZES[:3]:          # (again: small images in the staging a larger one left)
        r_img = t.ref.color_image(*tiles[:3], width, height)
        d_img = t.dg.color_image(width, height)
        assert d_img.shape == (height, width, 3)
        assert np.array_equal(d_img, r_img), f"{width} x {height}: device differs at {np.argwhere(d_img != r_img)[:5]}"
        assert np.array_equal(t.og.color_image(width, height), r_img), f"{width} x {height}: oracle differs"
    s = t.ref.color_image(*tiles[:3], 259, 259).reshape(-1, 3).astype(int)
    assert (s[:, 1] == 255).any() and ((s[:, 1] == 0) & (s[:, 0] > 0)).any() and (s.sum(axis=1) == 765).any() and (s.sum(axis=1) == 0).any()


def test_reuse_sequence(oracle, tmp_path):
    """dense grid, sparse grid, reset, pushes and a loaded file on ONE context, the three paths in rotation (so both sets of list heads
    and every hand-over between the paths are used): a stale work-list entry or head would show as marks of a surface that is gone"""
    gc = synth.GridConfig(R.SEQ_LOG2, R.SEQ_CS)
    geo = synth.ScanGeometry.full_circle_360()
    world = synth.World("room", gc)
    t = Trio(oracle, R.SEQ_LOG2, R.SEQ_CS)
    text = tmp_path / "sparse.txt"
    reach = R.SequenceReach(t.ref)
    pushes = 0
    for k, (action, inflate, factor) in enumerate(R.SEQUENCE):
        if action in ("dense", "sparse"):
            t.dg.upload_tiles(*(R.dense_grid() if action == "dense" else R.sparse_grid()).arrays())
        elif action == "reset":
            t.dg.reset()
        elif action == "load_text":
            t.dg.load_text(text)
        elif action == "push":
            pose, (x, y, yaw) = H.sensor_pose(world, 5 * pushes)
            data, mask = oracle.ingest_f32(world.scan(x, y, yaw, geo), H.MAX_RANGE, geo.angle_increment)
            t.dg.push(pose, data, mask, geo.angle_increment, geo.angle_min, H.MAX_RANGE, H.MIN_RANGE, H.LOW_REFL, want_stats=False)
            pushes += 1
        tiles = t.tiles()
        before = t.ref.content.copy()
        occ, n, info = t.call(KINDS[k % 3], inflate, factor, f"step {k} {action}", tiles)
        reach.record(k, action, inflate, factor, tiles[0], before, occ, n)
        if k == 1:
            t.dg.store_text(text)
    reach.assert_reached()
    assert {KINDS[x["k"] % 3] for x in reach.steps if x["action"] == "reset"} >= {"occupancy_into", "map_frame"}
