// occupancy_device.hpp -- the per-tile rules of ThreadGrid's two outputs, shared by the extraction kernels of occupancy_kernels.hip
// (k_occ_cells, k_color_image) and the one-pass publication of map_publish.hip (k_map_frame, k_map_frame_window); calcCoords' scan
// positions, sign changes and surface points, shared by k_occ_mark and the surface list of surface.hip.
#pragma once
#include "tsd_ctx.hpp"

namespace tsd {

// work list of k_occ_mark: the tiles that hold cells (processed and initialised), in OCC_SHARDS segments of the list with a counter
// each on its own 128-byte line (tile p goes to shard p % OCC_SHARDS, which has room for exactly tiles / OCC_SHARDS entries) -- one
// counter for all tiles would hand out ~88 slots per microsecond (MI355X_MICROARCH.md "dequeue"), 45 us for a cfg 2 map
constexpr int OCC_SHARDS = 32, OCC_HEAD_STRIDE = 32;

__device__ __forceinline__ bool tile_processed(int X, int Y, int PX)
{
  return X >= 1 && X <= PX - 2 && Y >= 1 && Y <= PX - 2;   // loops 1 .. partitions-2 (:25-27)
}

// value an initialised tile writes for its local cell (ly,lx), lx/ly in 0..32 (:41-47)
__device__ __forceinline__ int8_t occ_from_tsd(const GridDev& g, int p, int ly, int lx)
{
  const double t = ld_tsd(g.tsd + (size_t)p * TILE_STRIDE + cell_off(lx, ly));
  return (t > 0.0) ? 0 : -1;
}

// four consecutive cells of an initialised tile as four map bytes
__device__ __forceinline__ uint32_t occ_bits4(double t0, double t1, double t2, double t3)
{
  return (t0 > 0.0 ? 0u : 0xFFu) | (t1 > 0.0 ? 0u : 0xFF00u) | (t2 > 0.0 ? 0u : 0xFF0000u) | (t3 > 0.0 ? 0u : 0xFF000000u);
}

// calcCoords' scan positions of one tile, numbered in its serial order: c in [0, 1056) are the row scans (py = c / 32 in 0..32,
// px = c % 32 + 1, :38-60), c in [1056, 2112) the column scans (px = (c - 1056) / 32 in 0..32, py = (c - 1056) % 32 + 1, :62-80)
constexpr int SCAN_POSITIONS = 2 * TILE_PITCH * TILE_DIM;
struct ScanPos { int px, py; bool col; };
__device__ __forceinline__ ScanPos scan_pos(int c)
{
  ScanPos s;
  s.col = c >= TILE_PITCH * TILE_DIM;
  const int cc = s.col ? c - TILE_PITCH * TILE_DIM : c;
  const int a = cc / TILE_DIM;          // fixed index 0..32
  const int b = cc % TILE_DIM + 1;      // running index 1..32
  s.py = s.col ? b : a; s.px = s.col ? a : b;
  return s;
}
// the two cells of scan position s in T, the tile in the 33 x 33 form; true where they change sign (:51, :73): NaN and 0 make no event
__device__ __forceinline__ bool scan_event(const double* T, const ScanPos& s, double& prev, double& cur)
{
  prev = s.col ? T[(s.py - 1) * TILE_PITCH + s.px] : T[s.py * TILE_PITCH + s.px - 1];
  cur = T[s.py * TILE_PITCH + s.px];
  return (prev > 0 && cur < 0) || (prev < 0 && cur > 0);
}
// the sub-cell surface point of a sign change at scan position s of tile (X, Y) (:53-55, :76-77), in the reference's operation order
__device__ __forceinline__ void surface_point(const ScanPos& s, double prev, double cur, int X, int Y, double cs, double& x, double& y)
{
  const double interp = prev / (prev - cur);
  if (!s.col) {
    x = s.px * cs + cs * (interp - 1.0) + (X * TILE_DIM) * cs;
    y = s.py * cs + (Y * TILE_DIM) * cs;
  } else {
    x = s.px * cs + (X * TILE_DIM) * cs;
    y = s.py * cs + cs * (interp - 1.0) + (Y * TILE_DIM) * cs;
  }
}

// This extraction's mark counter and the NEXT extraction's list heads are cleared by the launch's first workgroup -- the heads come in
// two sets used in turn -- instead of by two memset launches ahead of every extraction.
__device__ __forceinline__ void occ_launch_clear(unsigned int* __restrict__ heads_next, int* __restrict__ count)
{
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) *count = 0;
    if (threadIdx.x < OCC_SHARDS) heads_next[threadIdx.x * OCC_HEAD_STRIDE] = 0u;
  }
}

// puts tile p (processed and initialised) on k_occ_mark's work list; one lane of the tile's workgroup calls it
__device__ __forceinline__ void occ_list_tile(const GridDev& g, int p, unsigned int* __restrict__ heads, uint32_t* __restrict__ list)
{
  const unsigned sh = (unsigned)p % OCC_SHARDS, cap = ((unsigned)g.tiles + OCC_SHARDS - 1) / OCC_SHARDS;
  list[sh * cap + atomicAdd(&heads[sh * OCC_HEAD_STRIDE], 1u)] = (uint32_t)p;
}

// k_occ_cells for one workgroup and tile p (the full-map kernels: p = blockIdx.x; the windowed frame: a tile of its box), one lane per
// 4 consecutive cells of a row (256 lanes): the map is read and written 4 bytes per lane (16-byte aligned rows).  A tile nobody writes
// (most of the grid) only forwards the persistent map to the output.
// own_bits(t) gives the lane's 4 map bytes of a processed, initialised tile (t: its 4 interior cells); it is called only for such a tile.
template <class OwnBits>
__device__ __forceinline__ void occ_cells_tile(const GridDev& g, int p, int8_t* __restrict__ content, int8_t* __restrict__ out,
                                               unsigned int* __restrict__ heads, uint32_t* __restrict__ list,
                                               unsigned int* __restrict__ heads_next, int* __restrict__ count, OwnBits own_bits)
{
  occ_launch_clear(heads_next, count);
  const int PX = g.PX;
  const int X = p % PX, Y = p / PX;
  const bool own_proc = tile_processed(X, Y, PX);
  const bool own_init = g.flags[p] != 0;
  const bool own_empty = !own_init && g.init_weight[p] > 0.0;   // isEmpty(), TsdGridPartition.h:72
  const bool left_w = X >= 1 && tile_processed(X - 1, Y, PX) && g.flags[p - 1];
  const bool down_w = Y >= 1 && tile_processed(X, Y - 1, PX) && g.flags[p - PX];
  const bool diag_w = X >= 1 && Y >= 1 && tile_processed(X - 1, Y - 1, PX) && g.flags[p - PX - 1];
  const int lx0 = (threadIdx.x & 7) * 4, ly = threadIdx.x >> 3;
  const size_t gi = (size_t)(Y * TILE_DIM + ly) * g.N + (size_t)(X * TILE_DIM + lx0);
  uint32_t* c4 = reinterpret_cast<uint32_t*>(content + gi);
  uint32_t* o4 = reinterpret_cast<uint32_t*>(out + gi);
  if (own_proc && own_init) {
    if (threadIdx.x == 0) occ_list_tile(g, p, heads, list);
    const uint32_t v = own_bits(g.tsd + (size_t)p * TILE_STRIDE + ly * TILE_DIM + lx0);     // interior row, 4 cells
    *c4 = v; *o4 = v;
    return;
  }
  if (own_proc && own_empty) { *c4 = 0u; *o4 = 0u; return; }
  uint32_t v = *c4;
  // a neighbour's halo lands in this tile's first column / row / corner cell (the last writer of the reference's
  // serial order wins: left > down > diagonal)
  bool changed = false;
  if (lx0 == 0 && left_w) { v = (v & ~0xFFu) | (uint8_t)occ_from_tsd(g, p - 1, ly, TILE_DIM); changed = true; }
  else if (lx0 == 0 && ly == 0 && down_w) { }       // (handled with the rest of row 0 below)
  if (ly == 0 && down_w) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (lx0 + k == 0 && left_w) continue;                                        // left neighbour wins the corner cell
      v = (v & ~(0xFFu << (8 * k))) | ((uint32_t)(uint8_t)occ_from_tsd(g, p - PX, TILE_DIM, lx0 + k) << (8 * k));
    }
    changed = true;
  }
  if (lx0 == 0 && ly == 0 && !left_w && !down_w && diag_w) { v = (v & ~0xFFu) | (uint8_t)occ_from_tsd(g, p - PX - 1, TILE_DIM, TILE_DIM); changed = true; }
  if (changed) *c4 = v;
  *o4 = v;
}

// grid2ColorImage's colour of one cell (TsdGrid.cpp:429-488), r | g << 8 | b << 16: t is the cell's tsd (NaN where the tile is not
// initialised or the coordinate is outside the grid), is_empty the tile's isEmpty()
__device__ __forceinline__ uint32_t cell_rgb(double t, bool is_empty)
{
  uint8_t r, gch, b;
  if (t > 0.0) { r = (uint8_t)(t * 255.0); gch = 255; b = (uint8_t)(t * 255.0); }
  else if (t < 0.0) { r = (uint8_t)((1.0 + t) * 255.0); gch = 0; b = 0; }
  else if (is_empty) { r = 255; gch = 255; b = 255; }
  else { r = 0; gch = 0; b = 0; }
  return (uint32_t)r | ((uint32_t)gch << 8) | ((uint32_t)b << 16);
}

// the colour of cell (lx, ly) of tile p read from the grid
__device__ __forceinline__ uint32_t cell_rgb_at(const GridDev& g, int p, int lx, int ly)
{
  double t = __builtin_nan("");
  const bool init = g.flags[p] != 0;
  if (init) t = ld_tsd(g.tsd + (size_t)p * TILE_STRIDE + cell_off(lx, ly));
  return cell_rgb(t, !init && g.init_weight[p] > 0.0);          // isEmpty(), TsdGridPartition.h:72
}

// the colour of the pixel at (x, y): coord2Cell, then the cell (black where coord2Cell fails)
__device__ __forceinline__ uint32_t pixel_rgb(const GridDev& g, double x, double y)
{
  int p, lx, ly; double dx, dy;
  if (coord2cell(g, x, y, p, lx, ly, dx, dy)) return cell_rgb_at(g, p, lx, ly);
  return cell_rgb(__builtin_nan(""), false);
}

}  // namespace tsd
