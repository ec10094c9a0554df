// frontier.hip -- the frontiers of an int8 map: the traversable cells that border unknown space as 8-connected components, each with
// its size, sums, bounding box and reachability from seed cells (tsd_frontiers_dev / _frame / _fetch / _dev_ptrs of include/tsd_hip.h,
// where the rules are written out).  One labelling engine, instantiated twice -- frontier cells at 8-connectivity, traversable cells
// at 4-connectivity -- and the passes that turn labels into an ordered list, all in integers:
//
// k_fr_tile      one workgroup per 32 x 32 tile: the tile's cells (for frontier cells with a one-cell apron) into LDS, classified, and
//                the tile's components labelled by a union-find in LDS.  A label is a cell's linear index y * W + x; inside a tile
//                the row-major order of the cells is the order of their linear indices, so a tile's roots are already the smallest
//                index of their component within the tile.  Writes every cell of the label image (FR_NONE where the predicate fails)
//                and the tile's "has any" byte.
// k_fr_seam      one wave per tile: the cells of its right column and bottom row are united with their neighbours in the next tiles
//                (for the 8-neighbourhood both diagonals of a corner) by a lock-free union-find on the label image.
// k_fr_flatten   every labelled cell replaces its label by its root.
// k_fr_roots     roots (label == own index) per segment -- 32 consecutive cells of a row, so that segments in row-major order carry
// (+ scan)       ascending indices -- counted, scanned (1 024 segments per workgroup, then one workgroup over the totals), and on the
//                second visit ranked: rank[root] = its place in the list, the record initialised.
// k_fr_stats     one workgroup per tile: every frontier cell adds to records[rank[label]], through a 64-slot table in LDS first.
// k_fr_compact   min_size: one workgroup moves the records that stay to the front, in order.
//
// No loop in these kernels waits for another wave: the only retry loop is the union's, and it strictly lowers a label or exits (see
// fr_union).  The order between the passes is the stream's.  The host waits twice: for the number of roots (the records are sized by
// it) and for the result.
#include "map_product.hpp"

#include <climits>

namespace tsd {

constexpr uint32_t FR_NONE = TSD_FRONTIER_NONE;
constexpr int FR_FRONTIER = 0, FR_REGION = 1;        // the two predicates (8- and 4-connected)
constexpr int FR_SCAN_BLOCK = 1024;                  // segments per workgroup of the scan
constexpr int FR_SLOTS = 64;                         // the stats pass's table in LDS
// d_res / h_res, in uint32
constexpr int FR_RES_N_ALL = 0, FR_RES_N = 1, FR_RES_USED = 2, FR_RES_UNIONS = 3, FR_RES_UNIONS_T = 4, FR_RES_SEED_ROOTS = 8;
constexpr int FR_RES_WORDS = FR_RES_SEED_ROOTS + TSD_FRONTIER_MAX_SEEDS;

struct FrMap : MapView { int free_max; };             // (the same bytes as the map's four fields followed by free_max)

#define FR_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define FR_AGENT __HIP_MEMORY_SCOPE_AGENT

// The union-find.  Invariant: L[i] <= i for every labelled cell i, L[i] is a cell of i's component, and a label is only ever lowered
// (by fetch_min).  A read may return an older label than the newest: that is a higher cell of the same chain, so nothing below depends
// on reads being fresh, only on the atomics being atomic.
template <int SCOPE>
__device__ __forceinline__ uint32_t fr_find(const uint32_t* L, uint32_t x)
{
  // x strictly descends (L[x] < x unless x is a root) and is bounded below by 0: at most x steps
  for (;;) {
    const uint32_t p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
    if (p >= x) return x;          // (p == x; ">=" only so that a torn invariant could not loop)
    x = p;
  }
}

// Unites the components of a and b; true where this call made the link (one root fewer).
template <int SCOPE>
__device__ __forceinline__ bool fr_union(uint32_t* L, uint32_t a, uint32_t b)
{
  // TERMINATION.  Every pass either exits or continues with a pair whose larger member is strictly smaller: fetch_min(L[a], b) with
  // b < a returns `old`; old == a means a was a root and now points to b -- done; otherwise old < a (another wave lowered L[a]
  // before us, L[a] <= a always) and the pass goes on with (old, b) in place of (a, b), which keeps a's old parent and b in one
  // component.  max(a, b) is bounded below by 0, so the loop ends after finitely many passes whatever other waves do; it never
  // waits for a value that someone else has to write.
  for (;;) {
    a = fr_find<SCOPE>(L, a);
    b = fr_find<SCOPE>(L, b);
    if (a == b) return false;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return true;
    a = old;
  }
}

// ---- tile pass
template <int KIND>
__global__ void __launch_bounds__(256)
k_fr_tile(FrMap m, uint32_t* __restrict__ L, uint8_t* __restrict__ any)
{
  constexpr int A = KIND == FR_FRONTIER ? 1 : 0, P = 32 + 2 * A;      // apron, pitch
  __shared__ int8_t s_v[P * P];
  __shared__ uint32_t s_lab[1024];
  const int bx = (int)blockIdx.x * 32, by = (int)blockIdx.y * 32;
  // outside the map: 0, which is not unknown (the border is not unknown space) and, in the tile, is masked by `in` below
  for (int i = (int)threadIdx.x; i < P * P; i += 256) {
    const int gx = bx + i % P - A, gy = by + i / P - A;
    s_v[i] = (gx >= 0 && gx < m.W && gy >= 0 && gy < m.H) ? m.map[(size_t)gy * m.stride + gx] : (int8_t)0;
  }
  __syncthreads();
  bool set[4];
  int some = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j, lx = c & 31, ly = c >> 5;
    const int8_t* v = s_v + (ly + A) * P + lx + A;
    bool s = bx + lx < m.W && by + ly < m.H && v[0] >= 0 && v[0] <= m.free_max;
    if (KIND == FR_FRONTIER) s = s && (v[-1] < 0 || v[1] < 0 || v[-P] < 0 || v[P] < 0);
    set[j] = s;
    some |= s ? 1 : 0;
    s_lab[c] = s ? (uint32_t)c : FR_NONE;
  }
  some = __syncthreads_or(some);
  if (threadIdx.x == 0) any[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (uint8_t)(some ? 1 : 0);
  if (some) {
    // forward neighbours only: every pair is seen from its smaller cell.  Whether a cell is labelled never changes (a label is lowered
    // to another label, never to or from FR_NONE), so `set` of a neighbour may be read while labels move.
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = (int)threadIdx.x + 256 * j, lx = c & 31, ly = c >> 5;
      if (!set[j]) continue;
      auto labelled = [&](int d) { return __hip_atomic_load(s_lab + d, __ATOMIC_RELAXED, FR_WG) != FR_NONE; };
      if (lx < 31 && labelled(c + 1)) fr_union<FR_WG>(s_lab, (uint32_t)c, (uint32_t)(c + 1));
      if (ly < 31) {
        if (labelled(c + 32)) fr_union<FR_WG>(s_lab, (uint32_t)c, (uint32_t)(c + 32));
        else if (KIND == FR_FRONTIER) {
          // (with the cell below labelled, its row neighbours are united with it from their own side)
          if (lx > 0 && labelled(c + 31)) fr_union<FR_WG>(s_lab, (uint32_t)c, (uint32_t)(c + 31));
          if (lx < 31 && labelled(c + 33)) fr_union<FR_WG>(s_lab, (uint32_t)c, (uint32_t)(c + 33));
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j, lx = c & 31, ly = c >> 5;
    const int gx = bx + lx, gy = by + ly;
    if (gx >= m.W || gy >= m.H) continue;
    uint32_t out = FR_NONE;
    if (set[j]) {
      const uint32_t r = fr_find<FR_WG>(s_lab, (uint32_t)c);
      out = (uint32_t)(by + (int)(r >> 5)) * (uint32_t)m.W + (uint32_t)(bx + (int)(r & 31));
    }
    L[(size_t)gy * m.W + gx] = out;
  }
}

// ---- seam pass: lanes 0 .. 31 the tile's right column, 32 .. 63 its bottom row
template <int KIND>
__global__ void __launch_bounds__(64)
k_fr_seam(uint32_t* L, const uint8_t* __restrict__ any, int W, int H, uint32_t* __restrict__ unions)
{
  int made = 0;
  if (any[(size_t)blockIdx.y * gridDim.x + blockIdx.x]) {
    const int t = (int)threadIdx.x;
    const bool right = t < 32;
    const int x = (int)blockIdx.x * 32 + (right ? 31 : t - 32), y = (int)blockIdx.y * 32 + (right ? t : 31);
    if (x < W && y < H) {
      const uint32_t me = (uint32_t)y * (uint32_t)W + (uint32_t)x;
      if (__hip_atomic_load(L + me, __ATOMIC_RELAXED, FR_AGENT) != FR_NONE) {
        // the three cells across the seam: (x + 1, y + d) for the column, (x + d, y + 1) for the row; d != 0 only at 8-connectivity
        for (int d = -1; d <= 1; d++) {
          if (KIND == FR_REGION && d != 0) continue;
          const int nx = right ? x + 1 : x + d, ny = right ? y + d : y + 1;
          if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
          const uint32_t nb = (uint32_t)ny * (uint32_t)W + (uint32_t)nx;
          if (__hip_atomic_load(L + nb, __ATOMIC_RELAXED, FR_AGENT) == FR_NONE) continue;
          if (fr_union<FR_AGENT>(L, me, nb)) made++;
        }
      }
    }
  }
  made = wave_sum_i(made);
  if (threadIdx.x == 0 && made) atomicAdd(unions, (uint32_t)made);
}

// ---- flatten.  Roots do not move in this pass (nothing unites any more), so every cell ends at its component's smallest index
// whatever the other cells' labels are at the time it walks.
__global__ void __launch_bounds__(256)
k_fr_flatten(uint32_t* L, const uint8_t* __restrict__ any, int W, int H)
{
  if (!any[(size_t)blockIdx.y * gridDim.x + blockIdx.x]) return;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j;
    const int x = (int)blockIdx.x * 32 + (c & 31), y = (int)blockIdx.y * 32 + (c >> 5);
    if (x >= W || y >= H) continue;
    const uint32_t me = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    const uint32_t l = __hip_atomic_load(L + me, __ATOMIC_RELAXED, FR_AGENT);
    if (l == FR_NONE || l == me) continue;
    const uint32_t r = fr_find<FR_AGENT>(L, l);
    if (r != l) __hip_atomic_store(L + me, r, __ATOMIC_RELAXED, FR_AGENT);
  }
}

// ---- roots to ranks.  Segment s = 32 cells of row s / tw starting at column 32 * (s % tw); 8 segments per workgroup.
// kEmit false: counts[s].  kEmit true: offs[s] + bsum[s / 1024] + the root's place in its segment -> rank[root], records[rank] initialised.
template <bool kEmit>
__global__ void __launch_bounds__(256)
k_fr_roots(const uint32_t* __restrict__ L, const uint8_t* __restrict__ any, int W, int H, int tw, uint32_t n_seg,
           uint32_t* __restrict__ seg, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ rank, tsd_frontier* __restrict__ rec,
           int reach0)
{
  const uint32_t s = blockIdx.x * 8u + (threadIdx.x >> 5);
  const int l32 = (int)threadIdx.x & 31;
  bool root = false;
  uint32_t me = 0;
  int x = 0, y = 0;
  if (s < n_seg) {
    y = (int)(s / (uint32_t)tw);
    const int tx = (int)(s % (uint32_t)tw);
    x = tx * 32 + l32;
    if (x < W && any[(size_t)(y >> 5) * tw + tx]) {
      me = (uint32_t)y * (uint32_t)W + (uint32_t)x;
      root = L[me] == me;
    }
  }
  const unsigned long long bal = __ballot(root);
  const uint32_t half = (threadIdx.x & 32) ? (uint32_t)(bal >> 32) : (uint32_t)bal;
  if (!kEmit) {
    if (l32 == 0 && s < n_seg) seg[s] = (uint32_t)__popc(half);
  } else if (root) {
    const uint32_t r = seg[s] + bsum[s / FR_SCAN_BLOCK] + (uint32_t)__popc(half & ((1u << l32) - 1u));
    rank[me] = r;
    tsd_frontier f;
    f.root_x = x; f.root_y = y; f.size = 0u; f.reachable = reach0; f.sum_x = 0ull; f.sum_y = 0ull;
    f.min_x = INT_MAX; f.min_y = INT_MAX; f.max_x = -1; f.max_y = -1;
    rec[r] = f;
  }
}

// Exclusive sums of v[base .. base + 1024) (4 per lane), in place, relative to `carry`; the 1 024 entries' total in every lane.
__device__ __forceinline__ uint32_t fr_scan_1024(uint32_t* v, uint32_t base, uint32_t n, uint32_t carry, uint32_t* s_wave)
{
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const uint32_t i0 = base + threadIdx.x * 4u;
  uint32_t e[4], mine = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { e[k] = i0 + k < n ? v[i0 + k] : 0u; mine += e[k]; }
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64); if (lane >= off) incl += t; }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { const uint32_t t = s_wave[k]; total += t; if (k < wave) before += t; }
  uint32_t run = carry + before + incl - mine;
#pragma unroll
  for (int k = 0; k < 4; k++) { if (i0 + k < n) v[i0 + k] = run; run += e[k]; }
  __syncthreads();               // (s_wave is free again)
  return total;
}

__global__ void __launch_bounds__(256)
k_fr_scan(uint32_t* __restrict__ seg, uint32_t n, uint32_t* __restrict__ bsum)
{
  __shared__ uint32_t s_wave[4];
  const uint32_t total = fr_scan_1024(seg, blockIdx.x * (uint32_t)FR_SCAN_BLOCK, n, 0u, s_wave);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: the scan's block totals into their bases, 1 024 at a time with the running sum carried along; the grand total
__global__ void __launch_bounds__(256)
k_fr_scan_top(uint32_t* __restrict__ bsum, uint32_t nb, uint32_t* __restrict__ total_out)
{
  __shared__ uint32_t s_wave[4];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += FR_SCAN_BLOCK) carry += fr_scan_1024(bsum, base, nb, carry, s_wave);
  if (threadIdx.x == 0) *total_out = carry;
}

// ---- seeds: the root of each seed's region (FR_NONE for a seed outside the map or on a cell that is not traversable)
__global__ void __launch_bounds__(64)
k_fr_seeds(const uint32_t* __restrict__ Lt, int W, int H, MapSeeds sd, uint32_t* __restrict__ res)
{
  const int k = (int)threadIdx.x;
  uint32_t r = FR_NONE;
  if (k < sd.n) {
    const int x = sd.xy[2 * k], y = sd.xy[2 * k + 1];
    if (x >= 0 && x < W && y >= 0 && y < H) r = Lt[(size_t)y * W + x];
  }
  if (k < TSD_FRONTIER_MAX_SEEDS) res[FR_RES_SEED_ROOTS + k] = r;
  const unsigned long long bal = __ballot(r != FR_NONE);
  if (k == 0) res[FR_RES_USED] = (uint32_t)__popcll(bal);
}

// ---- stats
__device__ __forceinline__ void fr_rec_add(tsd_frontier* f, uint32_t n, uint32_t sx, uint32_t sy, int x0, int y0, int x1, int y1, uint32_t reach)
{
  atomicAdd(&f->size, n);
  atomicAdd(reinterpret_cast<unsigned long long*>(&f->sum_x), (unsigned long long)sx);
  atomicAdd(reinterpret_cast<unsigned long long*>(&f->sum_y), (unsigned long long)sy);
  atomicMin(&f->min_x, x0); atomicMin(&f->min_y, y0);
  atomicMax(&f->max_x, x1); atomicMax(&f->max_y, y1);
  if (reach) atomicOr(&f->reachable, 1);
}

// A tile's cells meet in a table of 64 slots keyed by rank (slot = rank % 64; a tile seldom holds more than a few frontiers); a cell
// whose slot is taken by another rank adds to its record directly.  One tile's sums fit 32 bits: 1 024 cells x 32 767.
__global__ void __launch_bounds__(256)
k_fr_stats(const uint32_t* __restrict__ L, const uint32_t* __restrict__ Lt, const uint32_t* __restrict__ rank, const uint8_t* __restrict__ any,
           int W, int H, int n_seeds, const uint32_t* __restrict__ res, tsd_frontier* __restrict__ rec)
{
  if (!any[(size_t)blockIdx.y * gridDim.x + blockIdx.x]) return;
  __shared__ uint32_t s_key[FR_SLOTS], s_n[FR_SLOTS], s_sx[FR_SLOTS], s_sy[FR_SLOTS], s_reach[FR_SLOTS], s_seed[TSD_FRONTIER_MAX_SEEDS];
  __shared__ int s_x0[FR_SLOTS], s_y0[FR_SLOTS], s_x1[FR_SLOTS], s_y1[FR_SLOTS];
  const int t = (int)threadIdx.x;
  if (t < FR_SLOTS) {
    s_key[t] = FR_NONE; s_n[t] = 0u; s_sx[t] = 0u; s_sy[t] = 0u; s_reach[t] = 0u;
    s_x0[t] = INT_MAX; s_y0[t] = INT_MAX; s_x1[t] = -1; s_y1[t] = -1;
  }
  if (t < TSD_FRONTIER_MAX_SEEDS) s_seed[t] = t < n_seeds ? res[FR_RES_SEED_ROOTS + t] : FR_NONE;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = t + 256 * j;
    const int x = (int)blockIdx.x * 32 + (c & 31), y = (int)blockIdx.y * 32 + (c >> 5);
    if (x >= W || y >= H) continue;
    const size_t me = (size_t)y * W + x;
    const uint32_t l = L[me];
    if (l == FR_NONE) continue;
    const uint32_t r = rank[l];
    uint32_t reach = 0u;
    if (n_seeds > 0) {
      const uint32_t lt = Lt[me];            // (a frontier cell is traversable: never FR_NONE, so it meets no unused seed)
      for (int k = 0; k < n_seeds; k++) reach |= (lt == s_seed[k]) ? 1u : 0u;
    }
    const int slot = (int)(r & (FR_SLOTS - 1));
    const uint32_t prev = atomicCAS(&s_key[slot], FR_NONE, r);
    if (prev == FR_NONE || prev == r) {
      atomicAdd(&s_n[slot], 1u); atomicAdd(&s_sx[slot], (uint32_t)x); atomicAdd(&s_sy[slot], (uint32_t)y);
      atomicMin(&s_x0[slot], x); atomicMin(&s_y0[slot], y); atomicMax(&s_x1[slot], x); atomicMax(&s_y1[slot], y);
      if (reach) atomicOr(&s_reach[slot], 1u);
    } else {
      fr_rec_add(rec + r, 1u, (uint32_t)x, (uint32_t)y, x, y, x, y, reach);
    }
  }
  __syncthreads();
  if (t < FR_SLOTS && s_key[t] != FR_NONE) fr_rec_add(rec + s_key[t], s_n[t], s_sx[t], s_sy[t], s_x0[t], s_y0[t], s_x1[t], s_y1[t], s_reach[t]);
}

// ---- min_size: one workgroup, 256 records at a time, in place.  A record moves to an index at or below its own, and a chunk is read
// whole before any of it is written, so nothing unread is overwritten; the order is kept.
__global__ void __launch_bounds__(256)
k_fr_compact(tsd_frontier* rec, uint32_t n_all, uint32_t min_size, uint32_t* __restrict__ n_out)
{
  __shared__ uint32_t s_wave[4];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  uint32_t base_out = 0;
  for (uint32_t base = 0; base < n_all; base += 256u) {
    const uint32_t i = base + threadIdx.x;
    tsd_frontier f;
    bool keep = false;
    if (i < n_all) { f = rec[i]; keep = f.size >= min_size; }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t c = s_wave[k]; total += c; if (k < wave) before += c; }
    if (keep) rec[base_out + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = f;
    base_out += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = base_out;
}

// ---- host
template <int KIND>
static void fr_label(tsd_ctx* ctx, hipStream_t stream, const FrMap& m, uint32_t* L, uint8_t* any, uint32_t* unions, dim3 tiles, bool timed)
{
  { ScopedKernelTimer t(ctx, timed ? "frontier_tile" : "", true);
    hipLaunchKernelGGL(k_fr_tile<KIND>, tiles, dim3(256), 0, stream, m, L, any); }
  { ScopedKernelTimer t(ctx, timed ? "frontier_seam" : "", true);
    hipLaunchKernelGGL(k_fr_seam<KIND>, tiles, dim3(64), 0, stream, L, any, m.W, m.H, unions); }
  { ScopedKernelTimer t(ctx, timed ? "frontier_flatten" : "", true);
    hipLaunchKernelGGL(k_fr_flatten, tiles, dim3(256), 0, stream, L, any, m.W, m.H); }
}

// The whole pipeline on the source's stream, entered here, which it waits for.  The caller has checked the arguments.
static int run_frontiers(tsd_ctx* ctx, const MapSource& src, const tsd_frontier_params* prm, int* n_out, int* used_out)
{
  constexpr const char* who = "tsd_frontiers";
  if (int rc = map_source_enter(ctx, src)) return rc;
  tsd_ctx::Frontier& f = ctx->frontier;
  f.n = -1;                                            // (no result until this call has one: none where an allocation below fails)
  const auto& [map, stream, timed] = src;
  const FrMap m{map, prm->free_max};
  const int W = m.W, H = m.H, tw = (W + 31) / 32, th = (H + 31) / 32;
  const size_t cells = (size_t)W * H, tiles = (size_t)tw * th;
  const size_t n_seg = (size_t)tw * H, n_blk = (n_seg + FR_SCAN_BLOCK - 1) / FR_SCAN_BLOCK;
  const bool seeds = prm->n_seeds > 0;
  if (int rc = scratch_grow_all(ctx, who, &f.cells, cells, scratch_part(&f.d_lab, "the label image"), scratch_part(&f.d_rank, "the roots' ranks")))
    return rc;
  if (seeds) if (int rc = scratch_grow(ctx, who, &f.d_lab_t, &f.cells_t, cells, "the regions' label image")) return rc;
  if (int rc = scratch_grow_all(ctx, who, &f.tiles, tiles, scratch_part(&f.d_any, "the tile bytes", false, 2))) return rc;
  if (int rc = scratch_grow(ctx, who, &f.d_seg, &f.segs, n_seg + n_blk, "the segment counts")) return rc;
  if (!f.d_res) TSD_HIP_CHECK(ctx, hipMalloc(&f.d_res, FR_RES_WORDS * sizeof(uint32_t)));
  if (!f.h_res) TSD_HIP_CHECK(ctx, hipHostMalloc(&f.h_res, FR_RES_WORDS * sizeof(uint32_t), hipHostMallocDefault));

  const MapSeeds sd = map_seeds(prm->n_seeds, prm->seeds_xy);
  uint8_t* any_f = f.d_any;
  uint8_t* any_t = f.d_any + f.tiles;
  uint32_t* bsum = f.d_seg + n_seg;
  const dim3 tg(tw, th);
  const unsigned seg_blocks = (unsigned)((n_seg + 7) / 8);

  TSD_HIP_CHECK(ctx, hipMemsetAsync(f.d_res, 0, FR_RES_WORDS * sizeof(uint32_t), stream));
  fr_label<FR_FRONTIER>(ctx, stream, m, f.d_lab, any_f, f.d_res + FR_RES_UNIONS, tg, timed);
  if (seeds) {
    fr_label<FR_REGION>(ctx, stream, m, f.d_lab_t, any_t, f.d_res + FR_RES_UNIONS_T, tg, timed);
    hipLaunchKernelGGL(k_fr_seeds, dim3(1), dim3(64), 0, stream, f.d_lab_t, W, H, sd, f.d_res);
  }
  {
    ScopedKernelTimer t(ctx, timed ? "frontier_rank" : "", true);
    hipLaunchKernelGGL(k_fr_roots<false>, dim3(seg_blocks), dim3(256), 0, stream, f.d_lab, any_f, W, H, tw, (uint32_t)n_seg, f.d_seg, nullptr,
                       nullptr, nullptr, 0);
    hipLaunchKernelGGL(k_fr_scan, dim3((unsigned)n_blk), dim3(256), 0, stream, f.d_seg, (uint32_t)n_seg, bsum);
    hipLaunchKernelGGL(k_fr_scan_top, dim3(1), dim3(256), 0, stream, bsum, (uint32_t)n_blk, f.d_res + FR_RES_N_ALL);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(f.h_res, f.d_res, FR_RES_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
  const uint32_t n_all = f.h_res[FR_RES_N_ALL];
  if (int rc = scratch_grow(ctx, who, &f.d_rec, &f.recs, std::max<size_t>(n_all, 1), "the records")) return rc;
  uint32_t n = n_all;
  if (n_all > 0) {
    {
      ScopedKernelTimer t(ctx, timed ? "frontier_rank" : "", true);
      hipLaunchKernelGGL(k_fr_roots<true>, dim3(seg_blocks), dim3(256), 0, stream, f.d_lab, any_f, W, H, tw, (uint32_t)n_seg, f.d_seg, bsum,
                         f.d_rank, f.d_rec, seeds ? 0 : -1);
    }
    {
      ScopedKernelTimer t(ctx, timed ? "frontier_stats" : "", true);
      hipLaunchKernelGGL(k_fr_stats, tg, dim3(256), 0, stream, f.d_lab, f.d_lab_t, f.d_rank, any_f, W, H, prm->n_seeds, f.d_res, f.d_rec);
      if (prm->min_size > 1u)
        hipLaunchKernelGGL(k_fr_compact, dim3(1), dim3(256), 0, stream, f.d_rec, n_all, prm->min_size, f.d_res + FR_RES_N);
    }
    TSD_HIP_CHECK(ctx, hipGetLastError());
    if (prm->min_size > 1u)
      TSD_HIP_CHECK(ctx, hipMemcpyAsync(f.h_res + FR_RES_N, f.d_res + FR_RES_N, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    if (prm->min_size > 1u) n = f.h_res[FR_RES_N];
  }
  f.n = (int)n; f.n_all = (int)n_all; f.W = W; f.H = H;
  f.seam_unions = (int)f.h_res[FR_RES_UNIONS]; f.region_seam_unions = (int)f.h_res[FR_RES_UNIONS_T];
  *n_out = (int)n;
  if (used_out) *used_out = seeds ? (int)f.h_res[FR_RES_USED] : 0;
  return TSD_OK;
}

static const char* fr_params_wrong(const tsd_frontier_params* p, const int* n)
{
  if (!n) return "n is NULL";
  if (!p) return "params is NULL";
  if (p->free_max < 0 || p->free_max > 99) return "free_max is outside 0 .. 99";
  if (p->min_size < 1u) return "min_size is below 1";
  if (p->n_seeds < 0 || p->n_seeds > TSD_FRONTIER_MAX_SEEDS) return "n_seeds is outside 0 .. TSD_FRONTIER_MAX_SEEDS";
  if (p->n_seeds > 0 && !p->seeds_xy) return "seeds_xy is NULL with n_seeds > 0";
  return nullptr;
}

void frontier_free(tsd_ctx* ctx)
{
  tsd_ctx::Frontier& f = ctx->frontier;
  hipFree(f.d_lab); hipFree(f.d_rank); hipFree(f.d_lab_t); hipFree(f.d_any); hipFree(f.d_seg); hipFree(f.d_rec); hipFree(f.d_res);
  if (f.h_res) hipHostFree(f.h_res);
  f = tsd_ctx::Frontier{};
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_frontiers_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_frontier_params* params, int* n,
                      int* seeds_used)
{
  if (!ctx) return TSD_E_ARG;
  MapSource src{};
  if (int rc = map_source_caller(ctx, "tsd_frontiers_dev", map_dev, width, height, stride, &src)) return rc;
  if (const char* why = fr_params_wrong(params, n)) return map_refused(ctx, "tsd_frontiers_dev", why);
  return run_frontiers(ctx, src, params, n, seeds_used);
}

int tsd_frontiers_frame(tsd_ctx* ctx, const tsd_frontier_params* params, int* n, int* seeds_used)
{
  if (!ctx) return TSD_E_ARG;
  if (const char* why = fr_params_wrong(params, n)) return map_refused(ctx, "tsd_frontiers_frame", why);
  MapSource src{};
  if (int rc = map_source_frame(ctx, "tsd_frontiers_frame", false, &src)) return rc;
  return run_frontiers(ctx, src, params, n, seeds_used);
}

int tsd_frontiers_fetch(tsd_ctx* ctx, int first, int count, tsd_frontier* out)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Frontier& f = ctx->frontier;
  if (f.n < 0) return set_error(ctx, TSD_E_ARG, "tsd_frontiers_fetch: no result to fetch", hipSuccess);
  if (const char* why = fetch_range_wrong(first, count, f.n, out)) return map_refused(ctx, "tsd_frontiers_fetch", why);
  if (count == 0) return TSD_OK;
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  TSD_HIP_CHECK(ctx, hipMemcpy(out, f.d_rec + first, (size_t)count * sizeof(tsd_frontier), hipMemcpyDeviceToHost));
  return TSD_OK;
}

int tsd_frontiers_dev_ptrs(tsd_ctx* ctx, const void** records_dev, const void** labels_dev, int* n)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Frontier& f = ctx->frontier;
  if (f.n < 0) return set_error(ctx, TSD_E_ARG, "tsd_frontiers_dev_ptrs: no result", hipSuccess);
  if (records_dev) *records_dev = f.d_rec;
  if (labels_dev) *labels_dev = f.d_lab;
  if (n) *n = f.n;
  return TSD_OK;
}

int tsd_frontiers_counts(tsd_ctx* ctx, int* n_all, int* seam_unions, int* region_seam_unions)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Frontier& f = ctx->frontier;
  if (f.n < 0) return set_error(ctx, TSD_E_ARG, "tsd_frontiers_counts: no result", hipSuccess);
  if (n_all) *n_all = f.n_all;
  if (seam_unions) *seam_unions = f.seam_unions;
  if (region_seam_unions) *region_seam_unions = f.region_seam_unions;
  return TSD_OK;
}

}  // extern "C"
