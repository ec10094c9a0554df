"""One robot + one TSD grid per GPU, and the ONE exchange step the multi-robot case has: merging the
ranks' occupancy maps.

The reference's multi-robot mode (SlamNode.cpp:101-122, config/double-laser.yaml, launch/multi_slam)
runs N ``ThreadLocalize`` workers against one shared ``TsdGrid`` in one process; nothing is exchanged
between robots except through that grid, and the only consumer of the combined map is
``ThreadGrid``'s ``nav_msgs/OccupancyGrid`` (-1 unknown / 0 free / 100 occupied, ThreadGrid.cpp:72-118).
Here every rank (one process per GPU, ``torch.distributed``; backend "nccl" is RCCL over xGMI on
ROCm, "gloo" in the CPU tests) owns its robot's grid; localise and push never communicate.  The
shared occupancy map is the element-wise maximum of the per-rank int8 maps (all robots use the same
grid geometry, their start poses differ by ``local_offset_*``): occupied (100) wins over free (0) wins
over unknown (-1), which is what writing all robots' scans into one grid converges to.

The collective itself lives behind the C ABI (``include/tsd_comm.h``, ``lib/libtsd_comm.so``): extraction kernels and
``ncclAllReduce(int8, max)`` enqueued on the grid context's own stream, so a C++ host can merge without Python or
torch.  :class:`NativeOccupancyMerger` is the thin ctypes caller ``bench.py`` uses; ``torch.distributed`` is only the
launcher's process group (rank / world size, the 128-byte unique id travels through it, barrier and max-over-ranks of
the bench contract).  The merge semantics are also checked with two ranks on CPU (gloo, ``tests/test_cpu_multigpu.py``,
through the test-only ``tests/gloo_merger.py``) where RCCL cannot run; with two or more GPUs visible
``tests/test_gpu_multigpu_nranks.py`` and ``bench.py --gpus N`` compare the native merge with the element-wise maximum
of the ranks' own maps.
"""
from __future__ import annotations

import os

import ctypes as C

import numpy as np

from . import capi

UNKNOWN, FREE, OCCUPIED = -1, 0, 100
COMM_LIB_PATH = os.path.join(capi.LIB_DIR, "libtsd_comm.so")
COMM_ID_BYTES = 128

COMM_ABI = {
    "tsd_comm_unique_id": (C.c_int, [C.c_char_p]),
    "tsd_comm_create": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "tsd_comm_destroy": (None, [C.c_void_p]),
    "tsd_comm_world_size": (C.c_int, [C.c_void_p]),
    "tsd_comm_rank": (C.c_int, [C.c_void_p]),
    "tsd_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "tsd_comm_occupancy_allreduce": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "tsd_comm_allreduce_map": (C.c_int, [C.c_void_p]),
    "tsd_comm_occupancy_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_int8)]),
    "tsd_comm_map_dev": (C.c_void_p, [C.c_void_p]),
    "tsd_comm_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "tsd_comm_merge_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}
_comm_lib = None


def load_comm_library():
    """``lib/libtsd_comm.so`` (links librccl + libtsd_hip); every symbol of include/tsd_comm.h is bound."""
    global _comm_lib
    if _comm_lib is None:
        capi.load_library()
        if not os.path.exists(COMM_LIB_PATH):
            raise capi.TsdError(f"{COMM_LIB_PATH} not found: run __graft_entry__.build()")
        lib = C.CDLL(COMM_LIB_PATH)
        for name, (res, args) in COMM_ABI.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _comm_lib = lib
    return _comm_lib


class NativeOccupancyMerger:
    """The RCCL merge through the C ABI: one communicator per grid context, ``merge_async`` enqueues the extraction
    kernels and ``ncclAllReduce(int8, max)`` on the context's stream (nothing waits), ``wait`` synchronises.
    ``unique_id`` comes from rank 0 (``NativeOccupancyMerger.new_id()``) and is handed to every rank by the launcher."""

    @staticmethod
    def new_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        if load_comm_library().tsd_comm_unique_id(buf) != 0:
            raise capi.TsdError("tsd_comm_unique_id failed")
        return buf.raw

    def __init__(self, grid, world_size: int, rank: int, unique_id: bytes):
        self.lib = load_comm_library()
        self.grid = grid
        self.cells = grid.cells
        assert len(unique_id) == COMM_ID_BYTES
        self.h = self.lib.tsd_comm_create(grid.h, world_size, rank, unique_id)
        if not self.h:
            raise capi.TsdError("tsd_comm_create failed (RCCL communicator)")

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise capi.TsdError(f"{what} failed ({rc}): {self.lib.tsd_comm_last_error(self.h).decode()}")

    def merge_async(self, inflate: bool = False, inflate_factor: int = 2):
        self._check(self.lib.tsd_comm_occupancy_allreduce(self.h, int(inflate), inflate_factor), "tsd_comm_occupancy_allreduce")

    def wait(self):
        self._check(self.lib.tsd_comm_occupancy_wait(self.h, None), "tsd_comm_occupancy_wait")

    def world_size(self) -> int:
        """what the RCCL communicator itself says (``tsd_comm_world_size``), not what the launcher's environment claims"""
        return int(self.lib.tsd_comm_world_size(self.h))

    def profile(self, on: bool = True):
        self._check(self.lib.tsd_comm_profile(self.h, int(on)), "tsd_comm_profile")

    def merge_times(self):
        """(extraction ms, all-reduce ms, merges timed): totals over the merges issued while ``profile`` was on"""
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        self._check(self.lib.tsd_comm_merge_times(self.h, C.byref(a), C.byref(b), C.byref(n)), "tsd_comm_merge_times")
        return a.value, b.value, n.value

    def merged(self) -> np.ndarray:
        out = np.empty(self.cells * self.cells, dtype=np.int8)
        self._check(self.lib.tsd_comm_occupancy_wait(self.h, out.ctypes.data_as(C.POINTER(C.c_int8))), "tsd_comm_occupancy_wait")
        return out.reshape(self.cells, self.cells)


def cell_offset_from_origins(origin: float, origin_ref: float, cell_size: float, what: str = "origins") -> int:
    """Whole-cell offset of a grid whose map origin (``-(W / 2 + offset)``, ThreadGrid.cpp:28-29) is ``origin`` relative to one at
    ``origin_ref``.  A difference that is not within 1e-6 cells of an integer is refused: the merge shifts by whole cells."""
    d = (float(origin) - float(origin_ref)) / float(cell_size)
    r = round(d)
    if abs(d - r) > 1e-6:
        raise ValueError(f"{what}: the map origins differ by {d!r} cells, which is no whole number of cells")
    return int(r)


class LocalOccupancyGroup:
    """The same-device merge group (``tsd_group_*``, in ``lib/libtsd_hip.so``: no RCCL): N grids of this process on ONE GPU, grid i
    shifted by ``cell_offsets[i] = (ox, oy)`` whole cells, merged by a local kernel into one int8 map -- the signed maximum
    :class:`NativeOccupancyMerger` gets from ``ncclAllReduce`` across GPUs.  ``width = height = 0``: the window is the members'
    bounding box (``corner`` is its corner in the offsets' frame).  ``merge_async`` / ``merge_maps_async`` only enqueue; ``wait``
    synchronises.  This is co-residency on one chip, never a scaling curve.

    ``transforms`` (exclusive with ``cell_offsets``): one 3x3 rigid transform per grid that carries the grid's coordinates (metres,
    what ``align_to`` speaks) into the group's frame -- rotations and fractions of a cell included (``tsd_group_create_rigid``: every
    merged cell is the maximum over a footprint of one or two source cells per axis, so no occupied cell is lost).  ``corner`` is then
    the window's corner in frame cells, ``transforms`` what the group holds (for a translation group: the shifts as transforms)."""

    def __init__(self, grids, cell_offsets=None, width: int = 0, height: int = 0, transforms=None):
        self.lib = capi.load_library()
        self.grids = list(grids)
        n = len(self.grids)
        if cell_offsets is not None and transforms is not None:
            raise capi.TsdError("cell_offsets and transforms are exclusive")
        hs = (C.c_void_p * max(n, 1))(*[g.h for g in self.grids])
        if transforms is not None:
            flat = np.ascontiguousarray([np.asarray(T, dtype=np.float64).reshape(9) for T in transforms], dtype=np.float64).reshape(-1)
            if flat.size != 9 * n:
                raise capi.TsdError("transforms: one 3x3 matrix per grid")
            self.h = self.lib.tsd_group_create_rigid(n, hs, flat.ctypes.data_as(C.POINTER(C.c_double)), int(width), int(height))
            if not self.h:
                raise capi.TsdError("tsd_group_create_rigid refused the group (see stderr)")
        else:
            offs = None
            if cell_offsets is not None:
                flat = [int(v) for xy in cell_offsets for v in xy]
                if len(flat) != 2 * n:
                    raise capi.TsdError("cell_offsets: one (ox, oy) per grid")
                offs = (C.c_int32 * max(2 * n, 1))(*flat)
            self.h = self.lib.tsd_group_create(n, hs, offs, int(width), int(height))
            if not self.h:
                raise capi.TsdError("tsd_group_create refused the group (see stderr)")
        self.transforms = []
        for i in range(n):
            T = np.zeros(9)
            self.lib.tsd_group_member_transform(self.h, i, T.ctypes.data_as(C.POINTER(C.c_double)))
            self.transforms.append(T.reshape(3, 3))
        self.width, self.height = self.lib.tsd_group_width(self.h), self.lib.tsd_group_height(self.h)
        x0, y0 = C.c_int32(0), C.c_int32(0)
        self.lib.tsd_group_corner(self.h, C.byref(x0), C.byref(y0))
        self.corner = (x0.value, y0.value)
        self._host = self.lib.tsd_host_alloc(self.width * self.height)
        if not self._host:
            self.close()
            raise capi.TsdError("tsd_host_alloc failed")
        self._n_occupied = 0
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.tsd_group_destroy(self.h)
            self.h = None
        if getattr(self, "_host", None):
            self.lib.tsd_host_free(self._host)
            self._host = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise capi.TsdError(f"{what} failed ({rc}): {self.lib.tsd_group_last_error(self.h).decode()}")

    def cell_offsets(self):
        """the members' whole-cell offsets ``[(ox, oy), ...]`` as the group holds them, or ``None`` unless every member is a
        whole-cell shift (``tsd_group_cell_offsets``)"""
        n = len(self.grids)
        off = (C.c_int32 * (2 * n))()
        if self.lib.tsd_group_cell_offsets(self.h, off) != 0:
            return None
        return [(off[2 * i], off[2 * i + 1]) for i in range(n)]

    def merge_async(self, inflate: bool = False, inflate_factor: int = 2):
        """every member's extraction on its own stream, the merge and the copy to the host behind them; nothing waits"""
        prm = capi.MapParams(int(bool(inflate)), int(inflate_factor))
        self._check(self.lib.tsd_group_merge_begin(self.h, C.byref(prm), self._host), "tsd_group_merge_begin")

    def merge_maps_async(self, maps):
        """the merge of given maps: per member a (cells, cells) int8 array (copied into the group's buffer) or a device address"""
        assert len(maps) == len(self.grids)
        ptrs, keep = [], []
        for i, (m, g) in enumerate(zip(maps, self.grids)):
            if isinstance(m, int):
                ptrs.append(m)
                continue
            a = np.ascontiguousarray(m, dtype=np.int8)
            assert a.size == g.cells * g.cells, f"member {i}: {a.size} bytes for a {g.cells}^2 grid"
            keep.append(a)
            self._check(self.lib.tsd_group_member_map_upload(self.h, i, a.ctypes.data), "tsd_group_member_map_upload")
            ptrs.append(self.lib.tsd_group_member_map_dev(self.h, i))
        self._keep = keep               # (the copies are asynchronous: the arrays live until wait())
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._check(self.lib.tsd_group_merge_maps_begin(self.h, arr, self._host), "tsd_group_merge_maps_begin")

    def wait(self) -> int:
        n = C.c_int(0)
        self._check(self.lib.tsd_group_merge_wait(self.h, C.byref(n)), "tsd_group_merge_wait")
        self._keep = None
        self._n_occupied = n.value
        return n.value

    @property
    def n_occupied(self) -> int:
        """cells equal to 100 in the merged map of the last ``wait`` (counted by the merge kernel)"""
        return self._n_occupied

    def merged(self) -> np.ndarray:
        """waits; the merged map as (height, width) int8, row = y"""
        self.wait()
        buf = np.ctypeslib.as_array(C.cast(self._host, C.POINTER(C.c_int8)), shape=(self.height * self.width,))
        return buf.reshape(self.height, self.width).copy()

    def profile(self, on: bool = True):
        self._check(self.lib.tsd_group_profile(self.h, int(on)), "tsd_group_profile")

    def merge_times(self):
        """(extraction ms summed over members, merge kernel ms, merges timed): totals while ``profile`` was on"""
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        self._check(self.lib.tsd_group_merge_times(self.h, C.byref(a), C.byref(b), C.byref(n)), "tsd_group_merge_times")
        return a.value, b.value, n.value


def env_rank():
    """(rank, local_rank, world_size) as ``torch.distributed.run`` exports them."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def robot_offset_x(rank: int, base: float = 0.37, spacing: float = 0.7) -> float:
    """``local_offset_x`` of robot ``rank``: robots start ``spacing`` metres apart along -x
    (launch/multi_slam.launch:40 uses -0.7 for the second robot)."""
    return base - spacing * rank


def merge_bytes_per_rank(cells: int, world_size: int) -> float:
    """Bytes each rank sends in a ring all-reduce of the int8 map: 2 (W-1)/W of the map (DESIGN.md
    "Multi-GPU")."""
    if world_size <= 1:
        return 0.0
    return 2.0 * (world_size - 1) / world_size * cells * cells
