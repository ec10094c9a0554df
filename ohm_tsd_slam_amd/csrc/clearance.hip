// clearance.hip -- the exact Euclidean distance field to the occupied cells of an int8 map, up to a radius R, and the cost map nav2's
// inflation layer computes from it (tsd_clearance_dev, tsd_costmap_begin / _wait, tsd_costmap_table of include/tsd_hip.h, where the
// rule is written out).  The separable exact transform, in integers, over a window of the map:
//
// k_clear_mask   one bit per cell, "equals 100", as a byte map (byte k of a row = cells 8k .. 8k + 7, bit i = cell 8k + i: the row read
//                as little-endian 64-bit words has cell x at bit x % 64 of word x / 64), and per 32 x 32 tile "holds an obstacle", built
//                from a ballot over the wave's 64 bytes.  One workgroup = 32 rows x 512 cells; it writes every byte and every tile
//                flag of its area, so nothing has to be cleared first.
// k_clear_field  one workgroup = 64 columns (one mask word) x 32 rows.  If no tile within R of its area holds an obstacle it writes
//                0xFFFF / passes the source through and reads nothing else.  Otherwise it builds g -- the distance along the row to the
//                nearest obstacle, capped at R + 1 -- for its columns and its rows grown by R in LDS: one wave per row, the words to
//                the left and right are the same for all 64 lanes, a lane's own word is cut at its bit (clz / ctz).  Then every cell
//                walks outward from dy = 0 over g(x, y +- dy)^2 + dy^2 and stops when dy^2 reaches the best so far.  The cost table
//                lies in LDS behind g.
//
// The mask pass covers the column pass's workgroup-aligned area grown by R, so every word and tile flag the column pass reads was
// written by the same call.
#include "map_product.hpp"

namespace tsd {

constexpr int CLR_BW = 64, CLR_BH = 32;      // cells of one workgroup of the column pass
constexpr int CLR_CHUNK = 512;               // cells of a row that one wave of the mask pass turns into 64 mask bytes
constexpr int CLR_TABLE_BYTES = TSD_CLEARANCE_MAX_RADIUS * TSD_CLEARANCE_MAX_RADIUS + 4;   // the table, padded to dwords
constexpr int CLR_MAX_SIDE = 65536;          // the sides this file takes: above TSD_FRONTIER_MAX_SIDE, the other products' limit

struct ClrScratch { uint8_t* mask; size_t row_bytes; uint8_t* tiles; int tiles_w; };
struct ClrWindow { int x0, y0, x1, y1; };    // cells, half open

// bit i = byte i of v equals 100
__device__ __forceinline__ unsigned bytes_equal_100(uint64_t v)
{
  const uint64_t t = v ^ 0x6464646464646464ull, m = 0x7F7F7F7F7F7F7F7Full;
  const uint64_t z = ~(((t & m) + m) | t | m);           // 0x80 in every byte of t that is zero, exactly
  return (unsigned)(((z >> 7) * 0x0102040810204080ull) >> 56);
}

__global__ void __launch_bounds__(256)
k_clear_mask(MapView m, ClrScratch s, int c0, int t0, int aligned)
{
  __shared__ unsigned int s_any;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = c0 + (int)blockIdx.x, trow = t0 + (int)blockIdx.y;
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  const int x = chunk * CLR_CHUNK + lane * 8;
  unsigned any = 0u;
  for (int r = wave; r < 32; r += 4) {
    const int y = trow * 32 + r;
    unsigned b = 0u;
    if (y < m.H && x < m.W) {
      const int8_t* p = m.map + (size_t)y * m.stride + x;
      if (aligned && x + 8 <= m.W) {
        b = bytes_equal_100(*reinterpret_cast<const uint64_t*>(p));
      } else {
        const int n = m.W - x < 8 ? m.W - x : 8;
        for (int i = 0; i < n; i++) b |= (p[i] == 100 ? 1u : 0u) << i;
      }
    }
    s.mask[(size_t)y * s.row_bytes + (size_t)chunk * 64 + lane] = (uint8_t)b;      // (the mask's rows are padded to 32)
    any |= b;
  }
  // a tile is 4 of the wave's bytes wide: 16 tiles per wave, 4 waves over the tile's 32 rows
  const unsigned long long bal = __ballot(any != 0u);
  if (lane == 0) {
    unsigned bits = 0u;
    for (int t = 0; t < 16; t++) if ((bal >> (4 * t)) & 0xFull) bits |= 1u << t;
    if (bits) atomicOr(&s_any, bits);
  }
  __syncthreads();
  if (threadIdx.x < 16) s.tiles[(size_t)trow * s.tiles_w + chunk * 16 + (int)threadIdx.x] = (uint8_t)((s_any >> threadIdx.x) & 1u);
}

__device__ __forceinline__ int8_t cost_of(int8_t src, int8_t c)
{
  if (src == -1 && c < 99) return -1;       // unknown stays unknown outside the inscribed band
  return src > c ? src : c;
}

// kx0 / ty0: the mask word and the tile row of workgroup (0, 0).  d2 / cost: W x H, may be nullptr (cost only with kCost).
template <bool kCost>
__global__ void __launch_bounds__(256)
k_clear_field(MapView m, ClrScratch s, ClrWindow w, int kx0, int ty0, int R, const int8_t* __restrict__ table,
              uint16_t* __restrict__ d2, int8_t* __restrict__ cost, int skip, int aligned)
{
  extern __shared__ __attribute__((aligned(16))) uint16_t s_g[];      // [32 + 2R][64], then the table
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = kx0 + (int)blockIdx.x;
  const int bx = k * CLR_BW, by = (ty0 + (int)blockIdx.y) * CLR_BH;

  bool walk = true;
  if (skip) {
    // the tiles that hold a cell within R (Chebyshev) of the workgroup's area
    const int tx_lo = (bx - R > 0 ? bx - R : 0) >> 5, tx_hi = (bx + CLR_BW - 1 + R < m.W - 1 ? bx + CLR_BW - 1 + R : m.W - 1) >> 5;
    const int ty_lo = (by - R > 0 ? by - R : 0) >> 5, ty_hi = (by + CLR_BH - 1 + R < m.H - 1 ? by + CLR_BH - 1 + R : m.H - 1) >> 5;
    const int ntx = tx_hi - tx_lo + 1, nt = ntx * (ty_hi - ty_lo + 1);
    int any = 0;
    for (int i = (int)threadIdx.x; i < nt; i += 256) any |= s.tiles[(size_t)(ty_lo + i / ntx) * s.tiles_w + tx_lo + i % ntx];
    walk = __syncthreads_or(any) != 0;
  }
  if (!walk) {
    // open space: 8 cells per thread, whole vectors where the window and the alignment allow
    const int gx = bx + (int)(threadIdx.x & 7) * 8, gy = by + (int)(threadIdx.x >> 3);
    if (gy < w.y0 || gy >= w.y1) return;
    const size_t o = (size_t)gy * m.W + gx;
    if (aligned && gx >= w.x0 && gx + 8 <= w.x1) {
      if (d2) *reinterpret_cast<uint4*>(d2 + o) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      if (kCost && cost) *reinterpret_cast<uint64_t*>(cost + o) = *reinterpret_cast<const uint64_t*>(m.map + (size_t)gy * m.stride + gx);
      return;
    }
    for (int i = 0; i < 8; i++) {
      const int x = gx + i;
      if (x < w.x0 || x >= w.x1) continue;
      if (d2) d2[o + i] = 0xFFFFu;
      if (kCost && cost) cost[o + i] = m.map[(size_t)gy * m.stride + x];
    }
    return;
  }

  // ---- g for rows by - R .. by + 31 + R (those inside the map), one wave per row
  const int nrows = CLR_BH + 2 * R, ya = by - R;
  const int nw = (R + 63) >> 6;                  // words to either side that hold a cell within R of the word's nearer end
  const int roww = (int)(s.row_bytes >> 3);
  const uint64_t* mw = reinterpret_cast<const uint64_t*>(s.mask);
  for (int r = wave; r < nrows; r += 4) {
    const int y = ya + r;
    if (y < 0 || y >= m.H) continue;
    const uint64_t* row = mw + (size_t)y * roww;
    const uint64_t wk = row[k];
    // from bit 0 of the word down to the nearest obstacle of the words below, from bit 63 up to that of the words above
    int dl = R + 1, dr = R + 1;
    for (int j = 1; j <= nw && k - j >= 0; j++) {
      const uint64_t v = row[k - j];
      if (v) { dl = 64 * (j - 1) + 1 + __clzll((long long)v); break; }
    }
    for (int j = 1; j <= nw && k + j < roww; j++) {
      const uint64_t v = row[k + j];
      if (v) { dr = 64 * (j - 1) + __ffsll((unsigned long long)v); break; }
    }
    const uint64_t lo = wk & (~0ull >> (63 - lane));      // the word's cells at or below the lane's
    const uint64_t hi = wk & (~0ull << lane);             // ... at or above
    const int gl = lo ? lane - (63 - __clzll((long long)lo)) : lane + dl;
    const int gr = hi ? __ffsll((unsigned long long)hi) - 1 - lane : (63 - lane) + dr;
    int g = gl < gr ? gl : gr;
    if (g > R + 1) g = R + 1;
    s_g[r * CLR_BW + lane] = (uint16_t)g;
  }
  int8_t* s_tab = reinterpret_cast<int8_t*>(s_g + (size_t)nrows * CLR_BW);
  if (kCost) {
    const int nd = (R * R + 1 + 3) >> 2;          // (the device table is padded to whole dwords)
    const uint32_t* t4 = reinterpret_cast<const uint32_t*>(table);
    uint32_t* s4 = reinterpret_cast<uint32_t*>(s_tab);
    for (int i = (int)threadIdx.x; i < nd; i += 256) s4[i] = t4[i];
  }
  __syncthreads();

  // ---- d2 = min over |dy| <= R of g(x, y + dy)^2 + dy^2, outward from dy = 0
  const unsigned R2 = (unsigned)(R * R);
  const int x = bx + lane;
  if (x < w.x0 || x >= w.x1) return;
  for (int i = 0; i < 8; i++) {
    const int ly = wave * 8 + i, y = by + ly;
    if (y < w.y0 || y >= w.y1) continue;
    const uint16_t* col = s_g + (size_t)(ly + R) * CLR_BW + lane;
    const unsigned g0 = col[0];
    unsigned best = g0 * g0;
    for (int dy = 1; dy <= R; dy++) {
      const unsigned d = (unsigned)(dy * dy);
      if (d >= best) break;
      if (y - dy >= 0) { const unsigned g = col[-dy * CLR_BW]; const unsigned c = g * g + d; best = c < best ? c : best; }
      if (y + dy < m.H) { const unsigned g = col[dy * CLR_BW]; const unsigned c = g * g + d; best = c < best ? c : best; }
    }
    const size_t o = (size_t)y * m.W + x;
    if (d2) d2[o] = best <= R2 ? (uint16_t)best : (uint16_t)0xFFFFu;
    if (kCost && cost) {
      const int8_t src = m.map[(size_t)y * m.stride + x];
      cost[o] = best <= R2 ? cost_of(src, s_tab[best]) : src;
    }
  }
}

static size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// the scratch for a W x H map; replaced (behind everything that may still read it) where it is too small.  Not map_product.hpp's scratch_grow,
// here and in tsd_costmap_begin: this file waits for both streams before a buffer goes, and a failed allocation is TSD_E_HIP, out of memory too.
static int clearance_scratch(tsd_ctx* ctx, int W, int H, ClrScratch* out)
{
  tsd_ctx::Clearance& c = ctx->clearance;
  const size_t wpad = round_up((size_t)W, CLR_CHUNK), hpad = round_up((size_t)H, 32);
  const size_t mask_bytes = wpad / 8 * hpad, tiles_bytes = wpad / 32 * (hpad / 32);
  if (c.mask_bytes < mask_bytes || c.tiles_bytes < tiles_bytes) {
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->stream_io) TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream_io));
    if (c.mask_bytes < mask_bytes) {
      if (c.d_mask) hipFree(c.d_mask);
      c.d_mask = nullptr; c.mask_bytes = 0;
      TSD_HIP_CHECK(ctx, hipMalloc(&c.d_mask, mask_bytes));
      c.mask_bytes = mask_bytes;
    }
    if (c.tiles_bytes < tiles_bytes) {
      if (c.d_tiles) hipFree(c.d_tiles);
      c.d_tiles = nullptr; c.tiles_bytes = 0;
      TSD_HIP_CHECK(ctx, hipMalloc(&c.d_tiles, tiles_bytes));
      c.tiles_bytes = tiles_bytes;
    }
  }
  if (!c.d_table) TSD_HIP_CHECK(ctx, hipMalloc(&c.d_table, CLR_TABLE_BYTES));
  if (!c.h_table) {
    TSD_HIP_CHECK(ctx, hipHostMalloc(&c.h_table, CLR_TABLE_BYTES, hipHostMallocDefault));
    std::memset(c.h_table, 0, CLR_TABLE_BYTES);
  }
  out->mask = c.d_mask; out->row_bytes = wpad / 8; out->tiles = c.d_tiles; out->tiles_w = (int)(wpad / 32);
  return TSD_OK;
}

// Both kernels on `stream` for the window `win` of the map; table: R * R + 1 host bytes or nullptr (then cost is nullptr too).
// The caller has checked the arguments and that nothing else of the context uses the scratch.
static int launch_clearance(tsd_ctx* ctx, hipStream_t stream, const MapView& m, const tsd_map_window& win, int R, const int8_t* table,
                            uint16_t* d2, int8_t* cost, bool timed)
{
  ClrScratch s;
  if (int rc = clearance_scratch(ctx, m.W, m.H, &s)) return rc;
  tsd_ctx::Clearance& c = ctx->clearance;
  if (table) {
    std::memcpy(c.h_table, table, (size_t)R * R + 1);
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(c.d_table, c.h_table, round_up((size_t)R * R + 1, 4), hipMemcpyHostToDevice, stream));
  }
  const ClrWindow w{win.x, win.y, win.x + win.width, win.y + win.height};
  // the column pass's workgroups, and the area they read: theirs grown by R, clipped
  const int kx0 = w.x0 / CLR_BW, kx1 = (w.x1 - 1) / CLR_BW, ty0 = w.y0 / CLR_BH, ty1 = (w.y1 - 1) / CLR_BH;
  const int rx0 = std::max(0, kx0 * CLR_BW - R), rx1 = std::min(m.W, (kx1 + 1) * CLR_BW + R);
  const int ry0 = std::max(0, ty0 * CLR_BH - R), ry1 = std::min(m.H, (ty1 + 1) * CLR_BH + R);
  const int c0 = rx0 / CLR_CHUNK, c1 = (rx1 - 1) / CLR_CHUNK, t0 = ry0 / 32, t1 = (ry1 - 1) / 32;
  const uintptr_t mp = reinterpret_cast<uintptr_t>(m.map);
  const int aligned_in = (mp % 8 == 0 && m.stride % 8 == 0) ? 1 : 0;
  const int aligned_out = (aligned_in && m.W % 8 == 0 && reinterpret_cast<uintptr_t>(d2) % 16 == 0 && reinterpret_cast<uintptr_t>(cost) % 8 == 0) ? 1 : 0;
  const size_t lds = (size_t)(CLR_BH + 2 * R) * CLR_BW * sizeof(uint16_t) + (table ? round_up((size_t)R * R + 1, 4) : 0);
  const void* fn = table ? reinterpret_cast<const void*>(&k_clear_field<true>) : reinterpret_cast<const void*>(&k_clear_field<false>);
  if (int rc = ensure_dynamic_lds(ctx, fn, lds)) return rc;
  {
    ScopedKernelTimer t(ctx, timed ? "clearance" : "", true);
    hipLaunchKernelGGL(k_clear_mask, dim3(c1 - c0 + 1, t1 - t0 + 1), dim3(256), 0, stream, m, s, c0, t0, aligned_in);
    if (table)
      hipLaunchKernelGGL(k_clear_field<true>, dim3(kx1 - kx0 + 1, ty1 - ty0 + 1), dim3(256), lds, stream, m, s, w, kx0, ty0, R,
                         c.d_table, d2, cost, c.skip, aligned_out);
    else
      hipLaunchKernelGGL(k_clear_field<false>, dim3(kx1 - kx0 + 1, ty1 - ty0 + 1), dim3(256), lds, stream, m, s, w, kx0, ty0, R,
                         nullptr, d2, nullptr, c.skip, aligned_out);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

static bool window_inside(const tsd_map_window& w, int W, int H)
{
  return w.x >= 0 && w.y >= 0 && w.width >= 0 && w.height >= 0 && w.x <= W - w.width && w.y <= H - w.height;
}

void clearance_free(tsd_ctx* ctx)
{
  tsd_ctx::Clearance& c = ctx->clearance;
  if (c.ev_done) { hipEventSynchronize(c.ev_done); hipEventDestroy(c.ev_done); }
  hipFree(c.d_mask); hipFree(c.d_tiles); hipFree(c.d_table); hipFree(c.d_cost); hipFree(c.d_dist2);
  if (c.h_table) hipHostFree(c.h_table);
  c = tsd_ctx::Clearance{};
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_costmap_table(double cell_size, int radius_cells, double inscribed_radius_m, double cost_scaling, int8_t* table)
{
  if (!table || radius_cells < 1 || radius_cells > TSD_CLEARANCE_MAX_RADIUS || !(cell_size > 0.0)) return TSD_E_ARG;
  table[0] = 100;
  for (int d2 = 1; d2 <= radius_cells * radius_cells; d2++) {
    const double d = std::sqrt((double)d2) * cell_size;
    if (d <= inscribed_radius_m) { table[d2] = 99; continue; }
    const double e = 98.0 * std::exp(-cost_scaling * (d - inscribed_radius_m));
    table[d2] = (int8_t)(e >= 98.0 ? 98 : (e >= 1.0 ? (int)e : 1));      // clamp((int)e, 1, 98); a NaN gives 1
  }
  return TSD_OK;
}

int tsd_clearance_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_map_window* win, int radius_cells,
                      const int8_t* table, void* dist2_dev, void* cost_dev)
{
  if (!ctx) return TSD_E_ARG;
  if (caller_map_wrong(map_dev, width, height, stride, CLR_MAX_SIDE) || (!dist2_dev && !cost_dev) || (cost_dev && !table))
    return set_error(ctx, TSD_E_ARG, "tsd_clearance_dev: a null map, a size outside 1 .. 65536, no output, or a cost map without a table", hipSuccess);
  if (radius_cells < 1 || radius_cells > TSD_CLEARANCE_MAX_RADIUS)
    return set_error(ctx, TSD_E_ARG, "tsd_clearance_dev: the radius is outside 1 .. TSD_CLEARANCE_MAX_RADIUS", hipSuccess);
  const tsd_map_window whole{0, 0, width, height};
  const tsd_map_window w = win ? *win : whole;
  if (!window_inside(w, width, height) || w.width < 1 || w.height < 1)
    return set_error(ctx, TSD_E_ARG, "tsd_clearance_dev: the window is empty or not inside the map", hipSuccess);
  if (ctx->clearance.inflight) return set_error(ctx, TSD_E_ARG, "tsd_clearance_dev: a cost map is in flight (tsd_costmap_wait first)", hipSuccess);
  if (int rc = enter(ctx)) return rc;
  const MapView m{static_cast<const int8_t*>(map_dev), width, height, (size_t)stride};
  if (int rc = launch_clearance(ctx, ctx->stream, m, w, radius_cells, cost_dev ? table : nullptr, static_cast<uint16_t*>(dist2_dev),
                                static_cast<int8_t*>(cost_dev), true))
    return rc;
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}

int tsd_costmap_begin(tsd_ctx* ctx, const tsd_costmap_params* prm, int8_t* cost_host, uint16_t* dist2_host, const tsd_map_window* map_win,
                      tsd_map_window* out_win)
{
  if (!ctx) return TSD_E_ARG;
  if (!prm || !cost_host || !out_win || (prm->want_dist2 && !dist2_host))
    return set_error(ctx, TSD_E_ARG, "tsd_costmap_begin: a null argument", hipSuccess);
  tsd_ctx::Clearance& c = ctx->clearance;
  const int N = ctx->grid.N, R = prm->radius_cells;
  if (R < 1 || R > TSD_CLEARANCE_MAX_RADIUS) return set_error(ctx, TSD_E_ARG, "tsd_costmap_begin: the radius is outside 1 .. TSD_CLEARANCE_MAX_RADIUS", hipSuccess);
  MapSource src{};                               // (every grid's side is below CLR_MAX_SIDE)
  if (int rc = map_source_frame(ctx, "tsd_costmap_begin", false, &src, CLR_MAX_SIDE)) return rc;
  const tsd_map_window whole{0, 0, N, N};
  const tsd_map_window mw = map_win ? *map_win : whole;
  if (!window_inside(mw, N, N)) return set_error(ctx, TSD_E_ARG, "tsd_costmap_begin: the window is not inside the map", hipSuccess);
  if (mw.width == 0 || mw.height == 0) {         // an update that changed nothing: nothing to recompute
    out_win->x = out_win->y = out_win->width = out_win->height = 0;
    c.inflight = true; c.empty = true;
    return TSD_OK;
  }
  if (int rc = map_source_enter(ctx, src)) return rc;
  const size_t cells = (size_t)N * N;
  const bool dist2 = prm->want_dist2 != 0;
  if (!c.ev_done) TSD_HIP_CHECK(ctx, hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming));
  if (c.out_cells < cells) {
    if (c.d_cost) hipFree(c.d_cost);
    c.d_cost = nullptr; c.out_cells = 0; c.cost_cells = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&c.d_cost, cells));
    c.out_cells = cells;
  }
  if (dist2 && c.dist2_cells < cells) {
    if (c.d_dist2) hipFree(c.d_dist2);
    c.d_dist2 = nullptr; c.dist2_cells = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&c.d_dist2, cells * sizeof(uint16_t)));
    c.dist2_cells = cells;
  }
  std::vector<int8_t> table((size_t)R * R + 1);
  if (tsd_costmap_table(ctx->grid.cs, R, prm->inscribed_radius_m, prm->cost_scaling, table.data()) != TSD_OK)
    return set_error(ctx, TSD_E_ARG, "tsd_costmap_begin: tsd_costmap_table refused the parameters", hipSuccess);
  // what can differ from the previous cost map: map_win grown by R, clipped
  tsd_map_window ow;
  ow.x = std::max(0, mw.x - R); ow.y = std::max(0, mw.y - R);
  ow.width = std::min(N, mw.x + mw.width + R) - ow.x; ow.height = std::min(N, mw.y + mw.height + R) - ow.y;
  if (int rc = launch_clearance(ctx, src.stream, src.m, ow, R, table.data(), dist2 ? c.d_dist2 : nullptr, c.d_cost, src.timed)) return rc;
  const size_t o = (size_t)ow.y * N + ow.x;
  if (ow.width == N && ow.height == N) {
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(cost_host, c.d_cost, cells, hipMemcpyDeviceToHost, ctx->stream_io));
    if (dist2) TSD_HIP_CHECK(ctx, hipMemcpyAsync(dist2_host, c.d_dist2, cells * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream_io));
  } else {
    TSD_HIP_CHECK(ctx, hipMemcpy2DAsync(cost_host + o, (size_t)N, c.d_cost + o, (size_t)N, (size_t)ow.width, (size_t)ow.height,
                                        hipMemcpyDeviceToHost, ctx->stream_io));
    if (dist2)
      TSD_HIP_CHECK(ctx, hipMemcpy2DAsync(dist2_host + o, (size_t)N * 2, c.d_dist2 + o, (size_t)N * 2, (size_t)ow.width * 2, (size_t)ow.height,
                                          hipMemcpyDeviceToHost, ctx->stream_io));
  }
  TSD_HIP_CHECK(ctx, hipEventRecord(c.ev_done, ctx->stream_io));
  *out_win = ow;
  c.inflight = true; c.empty = false;
  c.cost_cells = cells;
  return TSD_OK;
}

int tsd_costmap_wait(tsd_ctx* ctx)
{
  if (!ctx) return TSD_E_ARG;
  tsd_ctx::Clearance& c = ctx->clearance;
  if (!c.inflight) return set_error(ctx, TSD_E_ARG, "tsd_costmap_wait: no cost map in flight", hipSuccess);
  c.inflight = false;
  const bool empty = c.empty;
  c.empty = false;
  if (!empty) TSD_HIP_CHECK(ctx, hipEventSynchronize(c.ev_done));
  return TSD_OK;
}

void* tsd_dev_alloc(tsd_ctx* ctx, uint64_t bytes)
{
  void* p = nullptr;
  if (!ctx || bytes == 0 || hipSetDevice(ctx->device) != hipSuccess) return nullptr;
  if (hipMalloc(&p, (size_t)bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}

void tsd_dev_free(tsd_ctx* ctx, void* p)
{
  if (!ctx || !p) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  hipFree(p);
}

int tsd_dev_copy(tsd_ctx* ctx, void* dst, const void* src, uint64_t bytes, int to_device)
{
  if (!ctx || !dst || !src) return TSD_E_ARG;
  if (int rc = enter(ctx)) return rc;
  if (bytes == 0) return TSD_OK;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}

int tsd_debug_set_clearance_skip(tsd_ctx* ctx, int on)
{
  if (!ctx) return TSD_E_ARG;
  ctx->clearance.skip = on ? 1 : 0;
  return TSD_OK;
}

}  // extern "C"
