// occupancy_kernels.hip -- the occupancy map of ThreadGrid::eventLoop (ThreadGrid.cpp:72-118):
// RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105) writes -1 / 0 per cell of every
// non-border tile into a PERSISTENT char map (_occGridContent, initialised to -1, ThreadGrid.cpp:27)
// and collects the sign changes along rows and columns; ThreadGrid then copies the map and marks the
// rounded sign-change cells with 100 (+ optional inflation).
//
// The reference walks tiles serially (y outer, x inner) and each initialised tile also writes its
// 1-cell halo, i.e. into the first row/column of its up/right neighbours, so for a cell at a tile's
// first row/column the LAST writer in that serial order wins: own tile > left > down > diagonal.
// k_occ_cells resolves that priority per cell (a gather, no write races); k_occ_mark does the
// idempotent "100" marks.  Streams the whole grid once: HBM-bound (cells*8 B read, cells*2 B written).
#include "occupancy_device.hpp"

namespace tsd {

// One workgroup per tile, one thread per 4 consecutive cells of a row (occ_cells_tile, occupancy_device.hpp); the tile's cells are read
// 32 bytes per lane.
__global__ void __launch_bounds__(256)
k_occ_cells(GridDev g, int8_t* __restrict__ content, int8_t* __restrict__ out, unsigned int* __restrict__ heads, uint32_t* __restrict__ list,
            unsigned int* __restrict__ heads_next, int* __restrict__ count)
{
  occ_cells_tile(g, (int)blockIdx.x, content, out, heads, list, heads_next, count, [](const tsd_cell_t* t) {
    return occ_bits4(ld_tsd(t), ld_tsd(t + 1), ld_tsd(t + 2), ld_tsd(t + 3));
  });
}

__device__ __forceinline__ void occ_mark(const GridDev& g, int8_t* out, double x, double y, int inflate,
                                         int factor)
{
  // ThreadGrid.cpp:96-117
  const double ru = round(x / g.cs), rv = round(y / g.cs);
  if (!(ru > 0.0 && ru < (double)g.N && rv > 0.0 && rv < (double)g.N)) return;
  const unsigned u = (unsigned)ru, v = (unsigned)rv, N = (unsigned)g.N;
  out[(size_t)v * N + u] = 100;
  if (inflate) {
    for (unsigned i = v - (unsigned)factor; i < v + (unsigned)factor; i++)
      for (unsigned j = u - (unsigned)factor; j < u + (unsigned)factor; j++)
        if ((size_t)i * N + j < (size_t)N * N) out[(size_t)i * N + j] = 100;
  }
}

// One 256-thread workgroup per LISTED tile (k_occ_cells' work list), a fixed grid looping over the list's shards.  (Round 2: one
// workgroup per tile of the grid -- 16 384 launches at cfg 2, of which three quarters found their tile uninitialised and left.)
__global__ void __launch_bounds__(256)
k_occ_mark(GridDev g, int8_t* __restrict__ out, int* __restrict__ count, int inflate, int factor,
           const unsigned int* __restrict__ heads, const uint32_t* __restrict__ list)
{
  const int PX = g.PX;
  const unsigned sh = blockIdx.x % OCC_SHARDS, cap = ((unsigned)g.tiles + OCC_SHARDS - 1) / OCC_SHARDS;
  const unsigned n_sh = heads[sh * OCC_HEAD_STRIDE];
  // the tile (33 x 33 doubles) through LDS: every cell is looked at by up to four scan positions
  __shared__ double T[TILE_CELLS];
  // The scan positions that hold a sign change (a few dozen of a surface tile's 2 112) are LISTED, and the interpolation, the two
  // divisions and the rounding of a mark run over the list, one lane per change: inside the scan loop the ~250 instructions of a mark
  // were executed by the whole wave for every loop round in which ANY lane had a change -- 12 of this kernel's 21 us at cfg 2
  // (seven variants of the stores themselves had changed nothing).
  __shared__ unsigned short s_ev[2 * TILE_PITCH * TILE_DIM];
  __shared__ int s_nev;
  if (threadIdx.x == 0) s_nev = 0;
  const double cs = g.cs;
  int n = 0;
  // A tile's 1 089 cells are five reads per thread, requested TOGETHER (as a plain loop the compiler had read -> wait -> LDS write five
  // times in a row), and the NEXT tile's five are requested before this tile's scans, whose time covers their round trip.
  constexpr int OCC_RD = (TILE_CELLS + 255) / 256;
  const unsigned k_first = blockIdx.x / OCC_SHARDS, k_step = gridDim.x / OCC_SHARDS;
  auto request = [&](int p, double (&v)[OCC_RD]) {
    const tsd_cell_t* Tg = g.tsd + (size_t)p * TILE_STRIDE;
#pragma unroll
    for (int j = 0; j < OCC_RD; j++) { const int i = (int)threadIdx.x + 256 * j; v[j] = ld_tsd_pinned(Tg + (i < TILE_CELLS ? i : 0)); }
  };
  double cur[OCC_RD];
  int p = 0;
  if (k_first < n_sh) { p = (int)list[sh * cap + k_first]; request(p, cur); }
  for (unsigned k = k_first; k < n_sh; k += k_step) {
    const int X = p % PX, Y = p / PX;
#pragma unroll
    for (int j = 0; j < OCC_RD; j++) { const int i = (int)threadIdx.x + 256 * j; if (i < TILE_CELLS) T[canonical_of_off(i)] = cur[j]; }   // LDS copy in the 33 x 33 form
    __syncthreads();
    const bool has_next = k + k_step < n_sh;
    int p_next = p;
    if (has_next) { p_next = (int)list[sh * cap + k + k_step]; request(p_next, cur); }
    // row scans: py in 0..32, px in 1..32 (:38-60); column scans: px in 0..32, py in 1..32 (:62-80)
    for (int c = threadIdx.x; c < SCAN_POSITIONS; c += 256) {
      double prev, cur;
      if (scan_event(T, scan_pos(c), prev, cur)) s_ev[atomicAdd(&s_nev, 1)] = (unsigned short)c;
    }
    __syncthreads();
    const int nev = s_nev;
    for (int e = threadIdx.x; e < nev; e += 256) {
      const ScanPos s = scan_pos((int)s_ev[e]);
      double prev, cur, x, y;
      scan_event(T, s, prev, cur);
      surface_point(s, prev, cur, X, Y, cs, x, y);      // (the same point tsd_surface_extract hands out: surface.hip)
      occ_mark(g, out, x, y, inflate, factor);
      n++;
    }
    __syncthreads();            // (the LDS copy and the list are rewritten by the next tile)
    if (threadIdx.x == 0) s_nev = 0;
    p = p_next;
  }
  n = wave_sum_i(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}

// TsdGrid::grid2ColorImage (TsdGrid.cpp:429-488), what ThreadGrid publishes next to the occupancy map
// (ThreadGrid.cpp:125).  The reference walks the image with px += stepW / py += stepH (repeated fp64 addition):
// the two coordinate tables are built that way on the host and a pixel is then one coord2Cell + one cell read.
// One thread per pixel, 3 bytes out; streams the touched cells once.
__global__ void __launch_bounds__(256)
k_color_image(GridDev g, const double* __restrict__ pxs, const double* __restrict__ pys, unsigned width,
              unsigned height, uint8_t* __restrict__ image)
{
  const unsigned w = blockIdx.x * 256u + threadIdx.x, h = blockIdx.y;
  if (w >= width || h >= height) return;
  const uint32_t c = pixel_rgb(g, pxs[w], pys[h]);
  uint8_t* o = image + 3 * ((size_t)h * width + w);
  o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
}

int launch_color_image(tsd_ctx* ctx, const double* d_px, const double* d_py, unsigned width, unsigned height, uint8_t* d_image)
{
  hipLaunchKernelGGL(k_color_image, dim3((width + 255) / 256, height), dim3(256), 0, ctx->stream, ctx->grid, d_px, d_py,
                     width, height, d_image);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

size_t occ_heads_bytes() { return 2 * OCC_SHARDS * OCC_HEAD_STRIDE * sizeof(unsigned int); }      // two sets, used in turn (zeroed at creation)

OccHeads next_occ_heads(tsd_ctx* ctx)
{
  OccHeads h;
  h.cur = ctx->d_occ_heads + (size_t)ctx->occ_parity * OCC_SHARDS * OCC_HEAD_STRIDE;
  h.next = ctx->d_occ_heads + (size_t)(ctx->occ_parity ^ 1) * OCC_SHARDS * OCC_HEAD_STRIDE;
  ctx->occ_parity ^= 1;
  return h;
}

// max_tiles: an upper bound of the list's length where the caller has one (the windowed frame: the tiles of its box), < 0: the grid's
int launch_occ_mark(tsd_ctx* ctx, int8_t* d_out, int* d_count, int inflate, int inflate_factor, const unsigned int* heads, int max_tiles)
{
  // (measured at cfg 2, maps of 40 / 200 scans: 2 048 workgroups 9.3 / 12.3 us, 1 024: 10.5 / 12.6, 512: 14.1 / 17.7, 256: 21.9 / 28.2 --
  //  a tile is a ~5 us chain of dependent round trips, so as many of them side by side as there are)
  constexpr int OCC_MARK_GROUPS = 2048;
  const int n_tiles = max_tiles >= 0 && max_tiles < ctx->grid.tiles ? (max_tiles < 1 ? 1 : max_tiles) : ctx->grid.tiles;
  const int mark_groups = n_tiles < OCC_MARK_GROUPS ? ((n_tiles + OCC_SHARDS - 1) / OCC_SHARDS) * OCC_SHARDS : OCC_MARK_GROUPS;   // a multiple of the shards
  hipLaunchKernelGGL(k_occ_mark, dim3(mark_groups), dim3(256), 0, ctx->stream, ctx->grid, d_out,
                     d_count, inflate, inflate_factor, heads, ctx->d_occ_list);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

int launch_occupancy(tsd_ctx* ctx, int8_t* d_out, int inflate, int inflate_factor)
{
  ScopedKernelTimer t(ctx, "occupancy", true);
  const OccHeads h = next_occ_heads(ctx);
  hipLaunchKernelGGL(k_occ_cells, dim3(ctx->grid.tiles), dim3(256), 0, ctx->stream, ctx->grid,
                     ctx->d_occ, d_out, h.cur, ctx->d_occ_list, h.next, ctx->d_occ_count);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return launch_occ_mark(ctx, d_out, ctx->d_occ_count, inflate, inflate_factor, h.cur);
}

}  // namespace tsd
