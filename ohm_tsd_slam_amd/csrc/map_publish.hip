// map_publish.hip -- ThreadGrid's publication (ThreadGrid.cpp:72-131) as one frame: the int8 occupancy map and the
// cellsX x cellsY RGB8 image of grid2ColorImage (TsdGrid.cpp:429-488), from one read of each tile, copied to the host beside the
// scans (tsd_map_frame_begin / tsd_map_frame_wait of include/tsd_hip.h).
//
// k_map_frame runs k_occ_cells' rules (occ_cells_tile, occupancy_device.hpp) and, in the same workgroup, writes the image pixels that
// sample its tile.  The reference accumulates the pixel coordinates (px += stepW, py += stepH); the tables are built that way on the
// host, as tsd_color_image does.  They are monotone, so the pixels whose coord2Cell lands in tile (X, Y) are a contiguous range of
// rows times a contiguous range of columns: col0[X] .. col0[X+1] and row0[Y] .. row0[Y+1], also built on the host.  Each workgroup
// stores whole dwords of its rows: the dwords whose first byte belongs to one of its pixels.  A dword that reaches into the next tile's
// first pixel reads that pixel from the grid; every other pixel comes from the tile's colours in LDS.  The ranges only decide which
// workgroup stores a dword -- each pixel is still placed by its own coord2Cell -- so the image equals k_color_image's whatever the
// ranges are (pixels whose coord2Cell fails are black there and here).  k_occ_mark then marks the surfaces unchanged.
#include "capi_internal.hpp"
#include "occupancy_device.hpp"

namespace tsd {

struct FrameTables {
  const double* pxs;     // [width] pixel x coordinates, accumulated like the reference
  const double* pys;     // [height]
  const int* col0;       // [PX + 1] first pixel column of every tile column (col0[0] = 0, col0[PX] = width)
  const int* row0;       // [PX + 1] first pixel row of every tile row
  unsigned width, height;
};

// one workgroup's part of a frame: tile p's cells and, with kImage, the image dwords it owns
template <bool kImage>
__device__ __forceinline__ void map_frame_tile(const GridDev& g, int p, int8_t* __restrict__ content, int8_t* __restrict__ out,
                                               unsigned int* __restrict__ heads, uint32_t* __restrict__ list,
                                               unsigned int* __restrict__ heads_next, int* __restrict__ count, const FrameTables& tab,
                                               uint8_t* __restrict__ image)
{
  const int PX = g.PX;
  const int X = p % PX, Y = p / PX;
  const bool own_init = g.flags[p] != 0;
  const int lx0 = (threadIdx.x & 7) * 4, ly = threadIdx.x >> 3;
  // the lane's 4 interior cells: read once, for the image and for the map
  double t0 = __builtin_nan(""), t1 = t0, t2 = t0, t3 = t0;
  if (own_init && (kImage || tile_processed(X, Y, PX))) {
    const tsd_cell_t* tc = g.tsd + (size_t)p * TILE_STRIDE + ly * TILE_DIM + lx0;
    t0 = ld_tsd(tc); t1 = ld_tsd(tc + 1); t2 = ld_tsd(tc + 2); t3 = ld_tsd(tc + 3);
  }
  if (kImage) {
    __shared__ uint32_t s_rgb[TILE_INTERIOR];
    const bool own_empty = !own_init && g.init_weight[p] > 0.0;      // isEmpty(), TsdGridPartition.h:72
    uint32_t* sr = s_rgb + ly * TILE_DIM + lx0;
    sr[0] = cell_rgb(t0, own_empty); sr[1] = cell_rgb(t1, own_empty); sr[2] = cell_rgb(t2, own_empty); sr[3] = cell_rgb(t3, own_empty);
    __syncthreads();
    const int r0 = tab.row0[Y], r1 = tab.row0[Y + 1];
    const unsigned d0 = (3u * (unsigned)tab.col0[X] + 3u) / 4u, d1 = (3u * (unsigned)tab.col0[X + 1] + 3u) / 4u;   // ceil(3 c / 4)
    const unsigned nd = d1 > d0 ? d1 - d0 : 0u;
    const unsigned n = r1 > r0 ? nd * (unsigned)(r1 - r0) : 0u;
    const size_t row_dw = (size_t)tab.width * 3u / 4u;      // (width % 4 == 0: every row starts on a dword)
    uint32_t* img4 = reinterpret_cast<uint32_t*>(image);
    for (unsigned i = threadIdx.x; i < n; i += 256u) {
      const unsigned h = (unsigned)r0 + i / nd, d = d0 + i % nd;
      const double y = tab.pys[h];
      const unsigned b0 = 4u * d, wa = b0 / 3u, wb = (b0 + 3u) / 3u;     // the (at most) two pixels of bytes b0 .. b0 + 3
      uint32_t c[2];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        int q, lx, lyc; double dx, dy;
        if (!coord2cell(g, tab.pxs[k ? wb : wa], y, q, lx, lyc, dx, dy)) c[k] = cell_rgb(__builtin_nan(""), false);
        else if (q == p) c[k] = s_rgb[lyc * TILE_DIM + lx];
        else c[k] = cell_rgb_at(g, q, lx, lyc);
      }
      uint32_t word = 0u;
#pragma unroll
      for (unsigned j = 0; j < 4u; j++) {
        const unsigned b = b0 + j, w = b / 3u;
        word |= ((c[w == wa ? 0 : 1] >> (8u * (b - 3u * w))) & 0xFFu) << (8u * j);
      }
      img4[(size_t)h * row_dw + d] = word;
    }
  }
  occ_cells_tile(g, p, content, out, heads, list, heads_next, count, [&](const tsd_cell_t*) { return occ_bits4(t0, t1, t2, t3); });
}

template <bool kImage>
__global__ void __launch_bounds__(256)
k_map_frame(GridDev g, int8_t* __restrict__ content, int8_t* __restrict__ out, unsigned int* __restrict__ heads, uint32_t* __restrict__ list,
            unsigned int* __restrict__ heads_next, int* __restrict__ count, FrameTables tab, uint8_t* __restrict__ image)
{
  map_frame_tile<kImage>(g, (int)blockIdx.x, content, out, heads, list, heads_next, count, tab, image);
}

// The windowed frame (tsd_map_update_begin).  u: the tiles that may differ from the previous frame, grown by the reach of a mark
// (window_growth); m: u grown by that reach again.  One workgroup per tile of m.  A tile of u is redone as k_map_frame does it: the
// persistent map and the staged map of its cells are rewritten -- which also erases every mark a changed tile can have left there --
// and so are its image dwords.  Every processed, initialised tile of m goes on k_occ_mark's list: the marks of u's own tiles, and
// those that the tiles around u drop into it, are made again; what such a tile marks outside u is there already (marks are
// idempotent).  The staged map then equals a full frame's byte for byte.
struct FrameWindow { int ux0, uy0, ux1, uy1, mx0, my0, mnx; };

template <bool kImage>
__global__ void __launch_bounds__(256)
k_map_frame_window(GridDev g, int8_t* __restrict__ content, int8_t* __restrict__ out, unsigned int* __restrict__ heads,
                   uint32_t* __restrict__ list, unsigned int* __restrict__ heads_next, int* __restrict__ count, FrameTables tab,
                   uint8_t* __restrict__ image, FrameWindow w)
{
  const int X = w.mx0 + (int)blockIdx.x % w.mnx, Y = w.my0 + (int)blockIdx.x / w.mnx;
  const int p = Y * g.PX + X;
  if (X >= w.ux0 && X <= w.ux1 && Y >= w.uy0 && Y <= w.uy1) {
    map_frame_tile<kImage>(g, p, content, out, heads, list, heads_next, count, tab, image);
    return;
  }
  occ_launch_clear(heads_next, count);
  if (threadIdx.x == 0 && tile_processed(X, Y, g.PX) && g.flags[p] != 0) occ_list_tile(g, p, heads, list);
}

// tiles a mark can land away from the tile that makes it: factor + 1 cells with inflation (the mark's cell is at most one past the
// tile's 32, the square reaches `factor` further), one cell without
static int window_growth(int inflate, int factor) { return inflate ? (factor + 1 + TILE_DIM - 1) / TILE_DIM : 1; }

static TileBox grow_box(const TileBox& b, int by, int PX)
{
  TileBox r;
  r.x0 = std::max(0, b.x0 - by); r.y0 = std::max(0, b.y0 - by);
  r.x1 = std::min(PX - 1, b.x1 + by); r.y1 = std::min(PX - 1, b.y1 + by);
  return r;
}

// one axis of coord2Cell on the host (tsd_device.hpp): the cell index, < 0 or >= N where it fails
static int host_cell_index(double v, double cs, double inv_cs)
{
  int i = (int)std::floor(v * inv_cs);
  const double d = ((double)i + 0.5) * cs;
  if (v < d) i--;
  return i;
}

// device staging of the frames: [surface count | pxs | pys | col0 | row0 | map | image], the tables written once
static int ensure_frame_staging(tsd_ctx* ctx, bool image)
{
  const GridDev& g = ctx->grid;
  const size_t N = (size_t)g.N, PX = (size_t)g.PX;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t tab_bytes = up(256 + 2 * N * sizeof(double) + 2 * (PX + 1) * sizeof(int));
  const size_t need = tab_bytes + up(N * N) + (image ? up(3 * N * N) : 0);
  if (ctx->frame_bytes >= need) return TSD_OK;
  if (!ctx->stream_io) {
    TSD_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->stream_io, hipStreamNonBlocking));
    TSD_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_io, hipEventDisableTiming));
  }
  if (!ctx->ev_frame) TSD_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_frame, hipEventDisableTiming));
  if (!ctx->ev_frame_done) TSD_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_frame_done, hipEventDisableTiming));
  if (!ctx->h_frame_count) TSD_HIP_CHECK(ctx, hipHostMalloc(&ctx->h_frame_count, sizeof(int), hipHostMallocDefault));
  // (a frame's staging is only replaced between frames: the last one's copies are done, tsd_map_frame_wait has seen them)
  if (ctx->d_frame) hipFree(ctx->d_frame);
  ctx->d_frame = nullptr; ctx->frame_bytes = 0; ctx->frame_map_valid = false;
  ctx->ledger.frame_lost();               // (a windowed frame has nothing to build on)
  TSD_HIP_CHECK(ctx, hipMalloc(&ctx->d_frame, need));
  // px / py exactly as the reference accumulates them (TsdGrid.cpp:433-486), then the tile ranges of the monotone tables
  std::vector<char> h(tab_bytes - 256);
  double* pq = reinterpret_cast<double*>(h.data());
  int* col0 = reinterpret_cast<int*>(pq + 2 * N);
  int* row0 = col0 + PX + 1;
  const double stepW = g.max_x / (double)N, stepH = g.max_y / (double)N;
  { double v = 0.0; for (size_t w = 0; w < N; w++) { pq[w] = v; v += stepW; } }
  { double v = 0.0; for (size_t r = 0; r < N; r++) { pq[N + r] = v; v += stepH; } }
  for (int axis = 0; axis < 2; axis++) {
    const double* c = pq + axis * N;
    int* t = axis ? row0 : col0;
    t[0] = 0; t[PX] = (int)N;
    size_t k = 0;
    for (size_t X = 1; X < PX; X++) {
      while (k < N && host_cell_index(c[k], g.cs, g.inv_cs) < (int)(X * TILE_DIM)) k++;
      t[X] = (int)k;
    }
  }
  hipError_t e = hipMemcpyAsync(ctx->d_frame + 256, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream_io);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream_io);        // (once per context: `h` must outlive its copy)
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, "tsd_map_frame_begin: coordinate tables", e);
  ctx->frame_bytes = need;
  return TSD_OK;
}

// tsd_map_frame_begin (win == nullptr) and tsd_map_update_begin: the whole map, or -- where the staging holds the previous frame of the
// same parameters and the grid was not rewritten wholesale since -- the window around the ledger's frame box
static int frame_begin(tsd_ctx* ctx, const tsd_map_params* prm, int8_t* occ_host, uint8_t* rgb_host, tsd_map_window* win, const char* who)
{
  if (!ctx || !prm || !occ_host) return TSD_E_ARG;
  if (ctx->frame_inflight) return set_error(ctx, TSD_E_ARG, (std::string(who) + ": a frame is in flight (tsd_map_frame_wait first)").c_str(), hipSuccess);
  // (a cost map in flight still reads the staged map on the copy stream)
  if (ctx->clearance.inflight) return set_error(ctx, TSD_E_ARG, (std::string(who) + ": a cost map is in flight (tsd_costmap_wait first)").c_str(), hipSuccess);
  if (int rc = enter(ctx)) return rc;
  std::lock_guard<std::mutex> lk_order(ctx->order_mutex);
  const bool image = rgb_host != nullptr;
  if (int rc = ensure_frame_staging(ctx, image)) return rc;
  const GridDev& g = ctx->grid;
  const size_t N = (size_t)g.N, PX = (size_t)g.PX, cells = N * N;
  const int inflate = prm->inflate ? 1 : 0, factor = prm->inflate_factor;
  const bool windowed = win && ctx->ledger.frame_may_be_windowed(image, inflate, factor);
  if (windowed && ctx->ledger.frame_box().empty()) {
    win->x = win->y = win->width = win->height = 0;
    *ctx->h_frame_count = 0;
    ctx->frame_empty = true; ctx->frame_inflight = true;
    return TSD_OK;
  }
  ctx->ledger.frame_started();
  ctx->frame_map_valid = false;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t tab_bytes = up(256 + 2 * N * sizeof(double) + 2 * (PX + 1) * sizeof(int));
  int* d_count = reinterpret_cast<int*>(ctx->d_frame);
  FrameTables tab;
  tab.pxs = reinterpret_cast<const double*>(ctx->d_frame + 256);
  tab.pys = tab.pxs + N;
  tab.col0 = reinterpret_cast<const int*>(tab.pys + N);
  tab.row0 = tab.col0 + PX + 1;
  tab.width = tab.height = (unsigned)N;
  int8_t* d_occ = reinterpret_cast<int8_t*>(ctx->d_frame + tab_bytes);
  uint8_t* d_img = reinterpret_cast<uint8_t*>(ctx->d_frame + tab_bytes + up(cells));
  // every push enqueued before this call is ahead of the frame on the grid's stream: the fused scan's deferred halo pass runs in the ray
  // cast that the same tsd_scan_submit enqueues behind its push, the batched push enqueues its own, an asynchronous push was drained above
  const OccHeads hd = next_occ_heads(ctx);
  TileBox u; u.x0 = 0; u.y0 = 0; u.x1 = (int)PX - 1; u.y1 = (int)PX - 1;
  if (windowed) {
    const int grow = window_growth(inflate, factor);
    u = grow_box(ctx->ledger.frame_box(), grow, (int)PX);
    const TileBox m = grow_box(u, grow, (int)PX);
    const FrameWindow fw{u.x0, u.y0, u.x1, u.y1, m.x0, m.y0, m.x1 - m.x0 + 1};
    const int n_m = fw.mnx * (m.y1 - m.y0 + 1);
    if (image)
      hipLaunchKernelGGL(k_map_frame_window<true>, dim3(n_m), dim3(256), 0, ctx->stream, g, ctx->d_occ, d_occ, hd.cur, ctx->d_occ_list,
                         hd.next, d_count, tab, d_img, fw);
    else
      hipLaunchKernelGGL(k_map_frame_window<false>, dim3(n_m), dim3(256), 0, ctx->stream, g, ctx->d_occ, d_occ, hd.cur, ctx->d_occ_list,
                         hd.next, d_count, tab, nullptr, fw);
    TSD_HIP_CHECK(ctx, hipGetLastError());
    if (int rc = launch_occ_mark(ctx, d_occ, d_count, inflate, factor, hd.cur, n_m)) return rc;
  } else {
    if (image)
      hipLaunchKernelGGL(k_map_frame<true>, dim3(g.tiles), dim3(256), 0, ctx->stream, g, ctx->d_occ, d_occ, hd.cur, ctx->d_occ_list,
                         hd.next, d_count, tab, d_img);
    else
      hipLaunchKernelGGL(k_map_frame<false>, dim3(g.tiles), dim3(256), 0, ctx->stream, g, ctx->d_occ, d_occ, hd.cur, ctx->d_occ_list,
                         hd.next, d_count, tab, nullptr);
    TSD_HIP_CHECK(ctx, hipGetLastError());
    if (int rc = launch_occ_mark(ctx, d_occ, d_count, prm->inflate, prm->inflate_factor, hd.cur)) return rc;
  }
  // The copies leave on stream_io behind the kernels' event: the grid's stream goes on with the next scans at once.
  TSD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_frame, ctx->stream));
  TSD_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream_io, ctx->ev_frame, 0));
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_frame_count, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream_io));
  if (windowed) {
    // The window's rows and columns only.  Pixel and cell grids coincide up to one pixel at a tile border (the pixel coordinates are
    // accumulated), and the tiles that changed lie a whole tile inside u wherever u was not clipped by the grid's edge: the pixels of
    // u's cell rectangle hold every pixel that can differ.  Its rows start on a dword (32 cells = 96 bytes).
    const size_t x = (size_t)u.x0 * TILE_DIM, y = (size_t)u.y0 * TILE_DIM;
    const size_t w = (size_t)(u.x1 - u.x0 + 1) * TILE_DIM, h = (size_t)(u.y1 - u.y0 + 1) * TILE_DIM;
    const size_t o = y * N + x;
    TSD_HIP_CHECK(ctx, hipMemcpy2DAsync(occ_host + o, N, d_occ + o, N, w, h, hipMemcpyDeviceToHost, ctx->stream_io));
    if (image) TSD_HIP_CHECK(ctx, hipMemcpy2DAsync(rgb_host + 3 * o, 3 * N, d_img + 3 * o, 3 * N, 3 * w, h, hipMemcpyDeviceToHost, ctx->stream_io));
  } else {
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(occ_host, d_occ, cells, hipMemcpyDeviceToHost, ctx->stream_io));
    if (image) TSD_HIP_CHECK(ctx, hipMemcpyAsync(rgb_host, d_img, 3 * cells, hipMemcpyDeviceToHost, ctx->stream_io));
  }
  TSD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_frame_done, ctx->stream_io));
  if (win) {
    win->x = u.x0 * TILE_DIM; win->y = u.y0 * TILE_DIM;
    win->width = (u.x1 - u.x0 + 1) * TILE_DIM; win->height = (u.y1 - u.y0 + 1) * TILE_DIM;
  }
  ctx->ledger.frame_enqueued(image, inflate, factor);
  ctx->frame_empty = false; ctx->frame_inflight = true; ctx->frame_map_valid = true;
  return TSD_OK;
}

static int frame_wait(tsd_ctx* ctx, int* n_surface, const char* who)
{
  if (!ctx) return TSD_E_ARG;
  if (!ctx->frame_inflight) return set_error(ctx, TSD_E_ARG, (std::string(who) + ": no frame in flight").c_str(), hipSuccess);
  ctx->frame_inflight = false;
  if (!ctx->frame_empty) {
    const hipError_t e = hipEventSynchronize(ctx->ev_frame_done);
    if (e != hipSuccess) { ctx->ledger.frame_lost(); ctx->frame_map_valid = false; return set_error(ctx, TSD_E_HIP, who, e); }
  }
  ctx->frame_empty = false;
  if (n_surface) *n_surface = *ctx->h_frame_count;
  return TSD_OK;
}

int8_t* frame_staged_map(const tsd_ctx* ctx)
{
  if (!ctx->d_frame) return nullptr;
  const size_t N = (size_t)ctx->grid.N, PX = (size_t)ctx->grid.PX;
  const size_t tab_bytes = (256 + 2 * N * sizeof(double) + 2 * (PX + 1) * sizeof(int) + 255) & ~(size_t)255;
  return reinterpret_cast<int8_t*>(ctx->d_frame + tab_bytes);
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_map_frame_begin(tsd_ctx* ctx, const tsd_map_params* prm, int8_t* occ_host, uint8_t* rgb_host)
{
  return frame_begin(ctx, prm, occ_host, rgb_host, nullptr, "tsd_map_frame_begin");
}

int tsd_map_frame_wait(tsd_ctx* ctx, int* n_surface) { return frame_wait(ctx, n_surface, "tsd_map_frame_wait"); }

int tsd_map_update_begin(tsd_ctx* ctx, const tsd_map_params* prm, int8_t* occ_host, uint8_t* rgb_host, tsd_map_window* win)
{
  if (!win) return TSD_E_ARG;
  return frame_begin(ctx, prm, occ_host, rgb_host, win, "tsd_map_update_begin");
}

int tsd_map_update_wait(tsd_ctx* ctx, int* n_surface) { return frame_wait(ctx, n_surface, "tsd_map_update_wait"); }

void* tsd_host_alloc(uint64_t bytes)
{
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}

void tsd_host_free(void* p)
{
  if (p) hipHostFree(p);
}

}  // extern "C"
