// surface.hip -- the map's surface as an ordered point list (tsd_surface_extract / _fetch / _dev in include/tsd_hip.h): the `coords`
// array of RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105), point for point in its serial order, and
// TsdGrid::interpolateNormal (TsdGrid.cpp:517-546) at every point.  k_occ_mark (occupancy_kernels.hip) finds the same sign changes
// and computes the same points (occupancy_device.hpp: scan_event, surface_point), rounds them into marks and drops them.
//
// The list's length is not known before it is counted and its order is a serial one, so three steps:
//   k_surface_count   one workgroup per window tile: the tile's events, counts[tile]
//   k_surface_scan    exclusive sums of the counts in the window's row-major tile order, 1 024 tiles per workgroup, and each
//   (+ _scan_top)     workgroup's total; above 1 024 tiles one more workgroup turns those totals into bases.  No workgroup waits for
//                     another inside a launch: the order between the levels is the stream's.
//   k_surface_emit    one workgroup per window tile: the rank of every event inside the tile from wave ballots, the points and
//                     normals over the tile's events as a dense loop, stored at base[tile / 1024] + offset[tile] + rank
// The host waits once, between scan and emit, for the total (the list's buffers are sized by it).
#include "capi_internal.hpp"
#include "occupancy_device.hpp"

#include <climits>

using namespace tsd;

namespace tsd {

constexpr int SURF_ROUNDS = (SCAN_POSITIONS + 255) / 256;      // 9: 8 full rounds of scan positions and 64 more
constexpr int SURF_SCAN_PER_LANE = 4;
constexpr int SURF_SCAN_BLOCK = 256 * SURF_SCAN_PER_LANE;      // tiles per workgroup of the scan
constexpr int SURF_SCAN_SHIFT = 10;
constexpr int SURF_TOTAL_SLOT = SURF_SCAN_BLOCK;               // d_bsum[0 .. 1024): the workgroups' bases; d_bsum[1024]: the list's length
static_assert((1 << SURF_SCAN_SHIFT) == SURF_SCAN_BLOCK, "emit finds a tile's scan workgroup by a shift");

// the window's tiles, row-major: tile w of the launch is (tx0 + w % wx, ty0 + w / wx)
struct SurfWindow { int tx0, ty0, wx, wy; };

// Tile p into LDS in the 33 x 33 form, its 1 089 cells as five reads per lane requested together (k_occ_mark's staging).  The caller
// synchronises.
__device__ __forceinline__ void surf_stage_tile(const GridDev& g, int p, double* T)
{
  constexpr int RD = (TILE_CELLS + 255) / 256;
  const tsd_cell_t* Tg = g.tsd + (size_t)p * TILE_STRIDE;
  double v[RD];
#pragma unroll
  for (int j = 0; j < RD; j++) { const int i = (int)threadIdx.x + 256 * j; v[j] = ld_tsd_pinned(Tg + (i < TILE_CELLS ? i : 0)); }
#pragma unroll
  for (int j = 0; j < RD; j++) { const int i = (int)threadIdx.x + 256 * j; if (i < TILE_CELLS) T[canonical_of_off(i)] = v[j]; }
}

// the sum of v over the workgroup's 256 lanes, in every lane (s_part: 4 words of LDS)
__device__ __forceinline__ unsigned surf_block_sum(unsigned v, unsigned* s_part)
{
  const int s = wave_sum_i((int)v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = (unsigned)s;
  __syncthreads();
  return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// An uninitialised tile (three quarters of a cfg 2 grid) costs its flag read.
__global__ void __launch_bounds__(256)
k_surface_count(GridDev g, SurfWindow win, uint32_t* __restrict__ counts)
{
  const int w = (int)blockIdx.x;
  const int p = (win.ty0 + w / win.wx) * g.PX + win.tx0 + w % win.wx;
  if (!g.flags[p]) { if (threadIdx.x == 0) counts[w] = 0u; return; }
  __shared__ double T[TILE_CELLS];
  __shared__ unsigned s_part[4];
  surf_stage_tile(g, p, T);
  __syncthreads();
  unsigned n = 0;
#pragma unroll
  for (int r = 0; r < SURF_ROUNDS; r++) {
    const int c = r * 256 + (int)threadIdx.x;
    double prev, cur;
    if (c < SCAN_POSITIONS && scan_event(T, scan_pos(c), prev, cur)) n++;
  }
  n = surf_block_sum(n, s_part);
  if (threadIdx.x == 0) counts[w] = n;
}

// Exclusive sums of 1 024 consecutive entries per workgroup (4 per lane): in[i] -> out[i] relative to the workgroup's first entry,
// the workgroup's total to totals[blockIdx.x].  A launch of ONE workgroup is the whole scan: its base is 0 and its total the list's
// length (totals[0] = 0, totals[SURF_TOTAL_SLOT] = the total).
__device__ __forceinline__ void surf_scan_block(const uint32_t* in, uint32_t* out /* may be `in` */, int n, unsigned& total)
{
  __shared__ unsigned s_wave[4];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * SURF_SCAN_PER_LANE;
  unsigned v[SURF_SCAN_PER_LANE], mine = 0;
#pragma unroll
  for (int k = 0; k < SURF_SCAN_PER_LANE; k++) { v[k] = i0 + k < n ? in[i0 + k] : 0u; mine += v[k]; }
  unsigned incl = mine;                       // inclusive sums over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned t = (unsigned)__shfl_up((int)incl, off, 64); if (lane >= off) incl += t; }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned before = 0; total = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { const unsigned t = s_wave[k]; total += t; if (k < wave) before += t; }
  unsigned run = before + incl - mine;
#pragma unroll
  for (int k = 0; k < SURF_SCAN_PER_LANE; k++) { if (i0 + k < n) out[i0 + k] = run; run += v[k]; }
}

__global__ void __launch_bounds__(256)
k_surface_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int n, uint32_t* __restrict__ bsum)
{
  unsigned total;
  surf_scan_block(counts, offsets, n, total);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) { bsum[0] = 0u; bsum[SURF_TOTAL_SLOT] = total; }
    else bsum[blockIdx.x] = total;
  }
}

// the workgroups' totals (at most 1 024 of them) into their bases, in place, and the list's length
__global__ void __launch_bounds__(256)
k_surface_scan_top(uint32_t* __restrict__ bsum, int n_blocks)
{
  unsigned total;
  surf_scan_block(bsum, bsum, n_blocks, total);
  if (threadIdx.x == 0) bsum[SURF_TOTAL_SLOT] = total;
}

// The rounds advance the scan position c in ascending order, lanes and waves inside a round likewise, so the rank -- events of the
// earlier rounds + of the round's earlier waves + of the wave's lower lanes -- is c's order, the reference's.  A round only LISTS its
// events (s_ev[rank] = c); the point's division and the normal's twenty reads run over the list, one lane per event: under the
// rounds' sparse predicate a whole wave would execute them for every round in which any of its lanes holds an event (k_occ_mark).
// counts[w] bounds what is written: a grid written between the two launches (which the caller must not do) cannot push the stores
// past the tile's share of the list.
template <bool NORMALS>
__global__ void __launch_bounds__(256)
k_surface_emit(GridDev g, SurfWindow win, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
               const uint32_t* __restrict__ bsum, double* __restrict__ xy, double* __restrict__ normals, uint8_t* __restrict__ ok)
{
  const int w = (int)blockIdx.x;
  const unsigned n_tile = counts[w];
  if (n_tile == 0u) return;                       // (also: every uninitialised tile)
  const int X = win.tx0 + w % win.wx, Y = win.ty0 + w / win.wx, p = Y * g.PX + X;
  const size_t base = (size_t)bsum[w >> SURF_SCAN_SHIFT] + (size_t)offsets[w];
  __shared__ double T[TILE_CELLS];
  __shared__ unsigned short s_ev[SCAN_POSITIONS];
  __shared__ unsigned s_wc[2][4];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  surf_stage_tile(g, p, T);
  __syncthreads();
  unsigned run = 0;
#pragma unroll 1
  for (int r = 0; r < SURF_ROUNDS; r++) {
    const int c = r * 256 + (int)threadIdx.x;
    double prev, cur;
    const bool ev = c < SCAN_POSITIONS && scan_event(T, scan_pos(c), prev, cur);
    const unsigned long long b = __ballot(ev);
    if (lane == 0) s_wc[r & 1][wave] = (unsigned)__popcll(b);
    __syncthreads();                              // (the two sets in turn: one barrier per round)
    unsigned before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const unsigned t = s_wc[r & 1][k]; all += t; if (k < wave) before += t; }
    if (ev) s_ev[run + before + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)c;
    run += all;
  }
  __syncthreads();
  const unsigned n_ev = run < n_tile ? run : n_tile;
  const double cs = g.cs;
  for (unsigned e = threadIdx.x; e < n_ev; e += 256u) {
    const ScanPos s = scan_pos((int)s_ev[e]);
    double prev, cur, x, y;
    scan_event(T, s, prev, cur);
    surface_point(s, prev, cur, X, Y, cs, x, y);
    reinterpret_cast<double2*>(xy)[base + e] = make_double2(x, y);
    if constexpr (NORMALS) {
      double nx, ny;
      const bool okn = interpolate_normal(g, x, y, nx, ny);
      reinterpret_cast<double2*>(normals)[base + e] = make_double2(nx, ny);
      ok[base + e] = okn ? 1 : 0;
    }
  }
}

void surface_free(tsd_ctx* ctx)
{
  tsd_ctx::Surface& s = ctx->surface;
  hipFree(s.d_counts); hipFree(s.d_offsets); hipFree(s.d_bsum); hipFree(s.d_xy); hipFree(s.d_normals); hipFree(s.d_ok);
  if (s.h_total) hipHostFree(s.h_total);
  s = tsd_ctx::Surface{};
}

// the scan's arrays, once per context: one entry per tile of the processed ring (the largest window), whole scan workgroups
static int surface_ensure_scan(tsd_ctx* ctx)
{
  tsd_ctx::Surface& s = ctx->surface;
  if (s.d_counts) return TSD_OK;
  const size_t ring = (size_t)(ctx->grid.PX - 2) * (size_t)(ctx->grid.PX - 2);
  const size_t entries = (ring + SURF_SCAN_BLOCK - 1) / SURF_SCAN_BLOCK * SURF_SCAN_BLOCK;
  hipError_t e = hipMalloc(&s.d_counts, entries * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&s.d_offsets, entries * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&s.d_bsum, (SURF_SCAN_BLOCK + 1) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&s.h_total), sizeof(unsigned int), hipHostMallocDefault);
  if (e != hipSuccess) { surface_free(ctx); return set_error(ctx, TSD_E_HIP, "tsd_surface_extract: scan buffers", e); }
  return TSD_OK;
}

// room for a list of `total` points (with normals where wanted); geometric growth, the old list is not kept
static int surface_ensure_list(tsd_ctx* ctx, size_t total, bool normals)
{
  tsd_ctx::Surface& s = ctx->surface;
  if (s.cap < total) {
    const size_t cap = std::max<size_t>({total, 2 * s.cap, 1024});
    hipFree(s.d_xy); s.d_xy = nullptr; s.cap = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&s.d_xy, cap * 2 * sizeof(double)));
    s.cap = cap;
  }
  if (normals && s.ncap < total) {
    const size_t cap = std::max<size_t>({total, 2 * s.ncap, 1024});
    hipFree(s.d_normals); hipFree(s.d_ok); s.d_normals = nullptr; s.d_ok = nullptr; s.ncap = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&s.d_normals, cap * 2 * sizeof(double)));
    TSD_HIP_CHECK(ctx, hipMalloc(&s.d_ok, cap));
    s.ncap = cap;
  }
  return TSD_OK;
}

}  // namespace tsd

extern "C" {

int tsd_surface_extract(tsd_ctx* ctx, const tsd_surface_params* params, int* n)
{
  if (!ctx || !n) return TSD_E_ARG;
  if (int rc = enter(ctx)) return rc;
  tsd_ctx::Surface& s = ctx->surface;
  const int PX = ctx->grid.PX;
  const bool normals = params ? params->want_normals != 0 : true;
  // the window, clipped to the processed ring 1 .. PX-2 (RayCastAxisAligned2D.cpp:25-27)
  const int tx0 = std::max(params ? params->tx0 : 1, 1), ty0 = std::max(params ? params->ty0 : 1, 1);
  const int tx1 = std::min(params ? params->tx1 : PX - 1, PX - 1), ty1 = std::min(params ? params->ty1 : PX - 1, PX - 1);
  s.n = 0; s.has_normals = normals; *n = 0;
  if (tx1 <= tx0 || ty1 <= ty0) return TSD_OK;
  if (int rc = surface_ensure_scan(ctx)) return rc;
  const SurfWindow win{tx0, ty0, tx1 - tx0, ty1 - ty0};
  const int tiles = win.wx * win.wy;                              // <= 1022^2
  const int scan_blocks = (tiles + SURF_SCAN_BLOCK - 1) / SURF_SCAN_BLOCK;
  if (scan_blocks > SURF_SCAN_BLOCK) return set_error(ctx, TSD_E_CAPACITY, "tsd_surface_extract: more than 2^20 tiles", hipSuccess);
  hipLaunchKernelGGL(k_surface_count, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->grid, win, s.d_counts);
  hipLaunchKernelGGL(k_surface_scan, dim3((unsigned)scan_blocks), dim3(256), 0, ctx->stream, (const uint32_t*)s.d_counts, s.d_offsets, tiles, s.d_bsum);
  if (scan_blocks > 1) hipLaunchKernelGGL(k_surface_scan_top, dim3(1), dim3(256), 0, ctx->stream, s.d_bsum, scan_blocks);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  // the one wait of the call: the list's buffers are sized by the total
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(s.h_total, s.d_bsum + SURF_TOTAL_SLOT, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const unsigned int total = *s.h_total;
  if (total > (unsigned int)INT_MAX) return set_error(ctx, TSD_E_CAPACITY, "tsd_surface_extract: more than INT_MAX points", hipSuccess);
  if (total == 0u) return TSD_OK;
  if (int rc = surface_ensure_list(ctx, (size_t)total, normals)) return rc;
  if (normals)
    hipLaunchKernelGGL(k_surface_emit<true>, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->grid, win, (const uint32_t*)s.d_counts,
                       (const uint32_t*)s.d_offsets, (const uint32_t*)s.d_bsum, s.d_xy, s.d_normals, s.d_ok);
  else
    hipLaunchKernelGGL(k_surface_emit<false>, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->grid, win, (const uint32_t*)s.d_counts,
                       (const uint32_t*)s.d_offsets, (const uint32_t*)s.d_bsum, s.d_xy, (double*)nullptr, (uint8_t*)nullptr);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  s.n = (int)total; *n = (int)total;
  return TSD_OK;
}

int tsd_surface_fetch(tsd_ctx* ctx, int first, int count, double* xy, double* normals, uint8_t* normal_ok)
{
  if (!ctx || !xy) return TSD_E_ARG;
  const tsd_ctx::Surface& s = ctx->surface;
  if (first < 0 || count < 0 || (long long)first + count > (long long)s.n)
    return set_error(ctx, TSD_E_ARG, "tsd_surface_fetch: the range is not inside the last list", hipSuccess);
  if ((normals || normal_ok) && !s.has_normals)
    return set_error(ctx, TSD_E_ARG, "tsd_surface_fetch: the last extraction was made without normals", hipSuccess);
  if (count == 0) return TSD_OK;
  if (int rc = enter(ctx)) return rc;
  const size_t f = (size_t)first, c = (size_t)count;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(xy, s.d_xy + 2 * f, 2 * c * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (normals) TSD_HIP_CHECK(ctx, hipMemcpyAsync(normals, s.d_normals + 2 * f, 2 * c * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (normal_ok) TSD_HIP_CHECK(ctx, hipMemcpyAsync(normal_ok, s.d_ok + f, c, hipMemcpyDeviceToHost, ctx->stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}

int tsd_surface_dev(tsd_ctx* ctx, const double** xy_dev, const double** normals_dev, const uint8_t** ok_dev, int* n)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Surface& s = ctx->surface;
  if (xy_dev) *xy_dev = s.d_xy;
  if (normals_dev) *normals_dev = s.has_normals ? s.d_normals : nullptr;
  if (ok_dev) *ok_dev = s.has_normals ? s.d_ok : nullptr;
  if (n) *n = s.n;
  return TSD_OK;
}

}  // extern "C"
