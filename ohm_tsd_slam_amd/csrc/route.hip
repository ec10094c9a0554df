// route.hip -- the cost-to-go field of an int8 map from up to 16 seed cells, the cheapest cell of every frontier and the paths
// (tsd_route_dev / _frame / _goals / _trace / _dev_ptrs of include/tsd_hip.h, where the rule is written out), and the same with one
// field per seed (tsd_route_fields_*).  All in integers.
//
// LAYERS.  Every kernel takes a layer from blockIdx.z (the trace: from a byte per goal): layer l's keys lie at key + l * cells, its
// tile bytes at act + l * tiles.  A route call launches one layer that holds all seeds; a fields call launches one layer per seed,
// layer l started from seed l alone.  The weight image, the "any" word and the visit counter are one for all layers.  In the two
// kernels a route call spends its time in, k_route_relax and k_route_trace (and k_route_waypoints of waypoint.hip), the layer is
// behind a template flag, so that the one-layer launch carries no layer arithmetic at all: one body, two instantiations.
//
// k_route_init   one workgroup per 32 x 32 tile and layer: every key of the layer's image (a seed's cell its index, the lowest where
//                two share a cell, RT_NONE elsewhere; on a field's layer l only seed l counts), every cell's weight byte (W[v] on a
//                traversable cell, 0 elsewhere: what the later passes read in place of the map, so the map may go once the call has
//                returned; it does not depend on the seeds, so layer 0 alone writes it), the tile's two "active" bytes for round 0.
// k_route_relax  one round: one workgroup per tile, gone at once where the tile's active byte of this round is 0.  Otherwise the tile's
//                keys and weights with a one-cell apron go into LDS, and gather sweeps -- every cell takes the minimum over its
//                eight neighbours -- run until a sweep lowers no key.  The cells that fell are stored, and the eight neighbour tiles'
//                bytes of the NEXT round are set.  The bytes are double-buffered: a round reads one buffer, clears its own byte
//                there and writes the other, so no byte is read and written in one launch.
// k_route_count  the cells with a key.
// k_route_goals  every frontier cell with a key finds its record by binary search over the records' roots and lowers the record's
//                slot to (key << 32) | cell; k_route_goals_emit turns the slots into tsd_route_goal in place.
// k_route_trace  one wave per goal cell: lanes 0 .. 7 test the eight neighbours, the lowest lane that matches is the step.
//                (route_trace_enqueue: the launch both tsd_route_trace and waypoint.hip's tsd_route_waypoints use)
//
// ORDER.  Only kernel boundaries order anything between tiles.  Within a round an apron read may return a neighbour's key of the
// round before: that neighbour's keys fell in this round, so it has set this tile's byte for the next one.  Keys only fall and are
// bounded below, every round with an active tile lowers a key or ends, so the rounds end; the host caps them all the same.  No
// workgroup waits for another: no flag spin, no ticket, no persistent kernel.  The only atomics are the visit counter (one add per
// active workgroup, a statistic), the cell count and the goals' 64-bit minimum, which commutes.
// With layers the argument holds layer by layer: a workgroup reads and writes the keys and the tile bytes of its own layer only, so
// the layers of one round are independent launches that happen to share a grid.  What they share is written with one value by
// whoever writes it (the "any" word: 1; the weight image: layer 0 alone) or is a commuting add (the visits).  The word is set while
// ANY layer has an active tile, so the rounds go on until the slowest layer ends; a layer that has ended finds all its bytes 0 and
// its workgroups leave at once.  One goal slot per layer and record: the minimum is the only new atomic, and it stays per layer.
#include "map_product.hpp"

#include <algorithm>
#include <cstring>

namespace tsd {

constexpr uint32_t RT_NONE = TSD_ROUTE_NONE;
constexpr int RT_P = 34;                             // the pitch of a tile with its apron in LDS
constexpr int RT_SWEEPS = 2048;                      // sweeps per launch before a tile hands itself on to the next round
constexpr int RT_BATCH = 32;                         // rounds between two reads of the "any" word (8 and 16 for the first two batches)
// d_res / h_res, in uint32 (the visits are one uint64)
// USED: bit i where seed i is used; REACHED: one word per layer
constexpr int RT_RES_USED = 0, RT_RES_ANY = 1, RT_RES_VISITS = 2, RT_RES_REACHED = 4, RT_RES_WORDS = 4 + TSD_FRONTIER_MAX_SEEDS;

struct RtWeights { uint8_t w[128]; };                // by map value; 0 above free_max

#define RT_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define RT_AGENT __HIP_MEMORY_SCOPE_AGENT

// neighbour k of the rule: (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (1,-1) (-1,1) (1,1)
__device__ __forceinline__ int rt_dx(int k) { return k < 4 ? (k == 0 ? -1 : k == 1 ? 1 : 0) : ((k & 1) ? 1 : -1); }
__device__ __forceinline__ int rt_dy(int k) { return k < 4 ? (k == 2 ? -1 : k == 3 ? 1 : 0) : ((k & 2) ? 1 : -1); }

// ---- init
__global__ void __launch_bounds__(256)
k_route_init(MapView m, RtWeights wt, MapSeeds sd, int fields, size_t cells, size_t tiles, uint32_t* __restrict__ key,
             uint8_t* __restrict__ wimg, uint8_t* __restrict__ act0, uint8_t* __restrict__ act1, uint32_t* __restrict__ res)
{
  const int layer = (int)blockIdx.z;
  const int s_lo = fields ? layer : 0, s_hi = fields ? layer + 1 : sd.n;       // the seeds of this layer
  key += (size_t)layer * cells;
  __shared__ uint8_t s_wt[128];
  const int t = (int)threadIdx.x;
  if (t < 128) s_wt[t] = wt.w[t];
  __syncthreads();
  const int bx = (int)blockIdx.x * 32, by = (int)blockIdx.y * 32;
  int some = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = t + 256 * j, gx = bx + (c & 31), gy = by + (c >> 5);
    if (gx >= m.W || gy >= m.H) continue;
    const int v = m.map[(size_t)gy * m.stride + gx];
    const uint8_t w = v >= 0 ? s_wt[v] : (uint8_t)0;
    uint32_t k = RT_NONE;
    if (w)
      for (int i = s_hi - 1; i >= s_lo; i--)
        if (sd.xy[2 * i] == gx && sd.xy[2 * i + 1] == gy) k = (uint32_t)i;
    const size_t me = (size_t)gy * m.W + gx;
    key[me] = k;
    if (layer == 0) wimg[me] = w;
    some |= k != RT_NONE ? 1 : 0;
  }
  some = __syncthreads_or(some);
  if (t == 0) {
    const size_t tile = (size_t)layer * tiles + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    act0[tile] = (uint8_t)(some ? 1 : 0);
    act1[tile] = 0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && layer == 0 && t < 64) {            // (one whole wave)
    bool used = false;
    if (t < sd.n) {
      const int x = sd.xy[2 * t], y = sd.xy[2 * t + 1];
      if (x >= 0 && x < m.W && y >= 0 && y < m.H) {
        const int v = m.map[(size_t)y * m.stride + x];
        used = v >= 0 && s_wt[v] != 0;
      }
    }
    const unsigned long long bal = __ballot(used);
    if (t == 0) res[RT_RES_USED] = (uint32_t)bal;
  }
}

// ---- one round.  LAYERS: the launch has a layer per blockIdx.z; a route call's launch (false) carries no layer arithmetic.
template <bool LAYERS>
__global__ void __launch_bounds__(256)
k_route_relax(uint32_t* key, const uint8_t* __restrict__ wimg, uint8_t* act_cur, uint8_t* act_next, int W, int H, size_t cells, size_t tiles,
              uint32_t lim_key, int max_sweeps, uint32_t* any, unsigned long long* visits)
{
  const int tw = (int)gridDim.x, th = (int)gridDim.y, tx = (int)blockIdx.x, ty = (int)blockIdx.y;
  const size_t tile = (size_t)ty * tw + tx;
  if constexpr (LAYERS) act_cur += (size_t)blockIdx.z * tiles;       // this layer's bytes ...
  if (!act_cur[tile]) return;                        // (the same byte for every lane; it is cleared behind the barrier below)
  if constexpr (LAYERS) {
    act_next += (size_t)blockIdx.z * tiles;
    key += (size_t)blockIdx.z * cells;               // ... and keys
  }
  __shared__ uint32_t s_key[RT_P * RT_P];
  __shared__ uint8_t s_w[RT_P * RT_P];
  const int t = (int)threadIdx.x, bx = tx * 32, by = ty * 32;
  // cells outside the map: not traversable, no key
  for (int i = t; i < RT_P * RT_P; i += 256) {
    const int gx = bx + i % RT_P - 1, gy = by + i / RT_P - 1;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
    const size_t g = in ? (size_t)gy * W + gx : 0;
    s_w[i] = in ? wimg[g] : (uint8_t)0;
    s_key[i] = in ? __hip_atomic_load(key + g, __ATOMIC_RELAXED, RT_AGENT) : RT_NONE;
  }
  __syncthreads();
  if (t == 0) { act_cur[tile] = 0; atomicAdd(visits, 1ull); }
  // a cell's moves do not change: bit k where neighbour k may step onto the cell (the neighbour's own traversability is its key's)
  int p[4];
  uint32_t cur[4], first[4], wb[4], moves[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = t + 256 * j;
    p[j] = ((c >> 5) + 1) * RT_P + (c & 31) + 1;
    wb[j] = s_w[p[j]];
    cur[j] = first[j] = s_key[p[j]];
    uint32_t mv = 0;
    if (wb[j]) {
      mv = 0xFu;
#pragma unroll
      for (int k = 4; k < 8; k++)
        if (s_w[p[j] + rt_dx(k)] && s_w[p[j] + rt_dy(k) * RT_P]) mv |= 1u << k;
    }
    moves[j] = mv;
  }
  int sweeps = 0, more = 0;
  for (;;) {
    int ch = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!moves[j]) continue;
      uint32_t best = cur[j];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        if (!((moves[j] >> k) & 1u)) continue;
        const uint32_t ka = __hip_atomic_load(s_key + p[j] + rt_dy(k) * RT_P + rt_dx(k), __ATOMIC_RELAXED, RT_WG);
        if (ka == RT_NONE) continue;
        const uint32_t cand = ka + (((k < 4 ? 5u : 7u) * wb[j]) << 4);          // (below 2^32: see the limit in tsd_hip.h)
        if (cand <= lim_key && cand < best) best = cand;
      }
      if (best < cur[j]) {
        cur[j] = best;
        __hip_atomic_store(s_key + p[j], best, __ATOMIC_RELAXED, RT_WG);
        ch = 1;
      }
    }
    sweeps++;
    more = __syncthreads_or(ch);
    if (!more || sweeps >= max_sweeps) break;
  }
  int fell = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (cur[j] == first[j]) continue;
    const int c = t + 256 * j;
    __hip_atomic_store(key + (size_t)(by + (c >> 5)) * W + bx + (c & 31), cur[j], __ATOMIC_RELAXED, RT_AGENT);   // (a cell with a weight is inside the map)
    fell = 1;
  }
  fell = __syncthreads_or(fell);
  if (fell && t < 8) {
    const int nx = tx + rt_dx(t), ny = ty + rt_dy(t);
    if (nx >= 0 && nx < tw && ny >= 0 && ny < th) act_next[(size_t)ny * tw + nx] = 1;
  }
  if (t == 8) {
    if (more) act_next[tile] = 1;                    // the sweeps ran out: this tile goes on in the next round
    if (more || fell) *any = 1u;
  }
}

__global__ void __launch_bounds__(256)
k_route_count(const uint32_t* __restrict__ key, int W, int H, size_t cells, uint32_t* __restrict__ reached)
{
  key += (size_t)blockIdx.z * cells;
  reached += blockIdx.z;
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j;
    const int x = (int)blockIdx.x * 32 + (c & 31), y = (int)blockIdx.y * 32 + (c >> 5);
    if (x < W && y < H && key[(size_t)y * W + x] != RT_NONE) n++;
  }
  n = wave_sum_i(n);
  if (((int)threadIdx.x & 63) == 0 && n) atomicAdd(reached, (uint32_t)n);
}

// ---- goals.  A slot is the first 8 bytes of its tsd_route_goal: (key << 32) | cell, all ones while no cell has lowered it.  The
// slots are a matrix [layers][n]; init and emit take it as one row of layers * n.
__global__ void __launch_bounds__(256)
k_route_goals_init(unsigned long long* __restrict__ slots, int n)
{
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) slots[2 * (size_t)i] = ~0ull;
}

__global__ void __launch_bounds__(256)
k_route_goals(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ key, size_t cells, int layers, const tsd_frontier* __restrict__ rec,
              int n, int W, int H, unsigned long long* slots)
{
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j;
    const int x = (int)blockIdx.x * 32 + (c & 31), y = (int)blockIdx.y * 32 + (c >> 5);
    if (x >= W || y >= H) continue;
    const uint32_t me = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    const uint32_t root = lab[me];
    if (root == TSD_FRONTIER_NONE) continue;
    int slot = -2;                                   // -2: not looked for yet; -1: the root has no record
    for (int l = 0; l < layers && slot != -1; l++) {
      const uint32_t k = key[(size_t)l * cells + me];
      if (k == RT_NONE) continue;
      if (slot == -2) {                              // one search per cell, at the first layer that has a key for it
        // the records are in ascending root index; a root that min_size dropped is not among them
        int lo = 0, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const uint32_t r = (uint32_t)rec[mid].root_y * (uint32_t)W + (uint32_t)rec[mid].root_x;
          if (r < root) lo = mid + 1; else hi = mid;
        }
        slot = lo < n && (uint32_t)rec[lo].root_y * (uint32_t)W + (uint32_t)rec[lo].root_x == root ? lo : -1;
        if (slot < 0) break;
      }
      atomicMin(slots + 2 * ((size_t)l * n + slot), ((unsigned long long)k << 32) | me);
    }
  }
}

__global__ void __launch_bounds__(256)
k_route_goals_emit(unsigned long long* __restrict__ slots, int n)
{
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const unsigned long long s = slots[2 * (size_t)i];
  const uint32_t k = (uint32_t)(s >> 32);
  const bool none = s == ~0ull;
  // cell, dist | seed, reserved
  slots[2 * (size_t)i] = none ? ~0ull : (((unsigned long long)(k >> 4) << 32) | (uint32_t)s);
  slots[2 * (size_t)i + 1] = none ? 0xFFFFFFFFull : (unsigned long long)(k & 15u);
}

// ---- trace: one wave per goal, on the layer layer_of_goal[g] (LAYERS false: layer 0 for every goal, layer_of_goal is not read)
template <bool LAYERS>
__global__ void __launch_bounds__(64)
k_route_trace(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, int W, int H, const uint32_t* __restrict__ goals,
              const uint8_t* __restrict__ layer_of_goal, size_t layer_stride, int max_len, uint32_t* __restrict__ paths, int32_t* __restrict__ len)
{
  const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
  if constexpr (LAYERS) key += (size_t)__builtin_amdgcn_readfirstlane((int)layer_of_goal[g]) * layer_stride;   // (one value per wave: kept scalar)
  const uint32_t cells = (uint32_t)W * (uint32_t)H;
  uint32_t b = goals[g];
  int n = 0;
  if (b < cells) {
    uint32_t kb = key[b];
    if (kb != RT_NONE) {
      uint32_t* out = paths + (size_t)g * max_len;
      const int dx = rt_dx(lane & 7), dy = rt_dy(lane & 7);
      const uint32_t ck = (lane & 7) < 4 ? 5u : 7u;
      // d falls strictly from step to step, so the walk ends; the bound only keeps a torn image from walking on
      while ((uint32_t)n < cells) {
        if (lane == 0 && n < max_len) out[n] = b;
        n++;
        if ((kb >> 4) == 0u) break;
        const int x = (int)(b % (uint32_t)W), y = (int)(b / (uint32_t)W);
        const int ax = x - dx, ay = y - dy;            // a = b - offset_k
        bool hit = false;
        uint32_t a = 0, ka = RT_NONE;
        if (lane < 8 && ax >= 0 && ax < W && ay >= 0 && ay < H) {
          a = (uint32_t)ay * (uint32_t)W + (uint32_t)ax;
          bool ok = wimg[a] != 0;
          if (lane >= 4) ok = ok && wimg[(size_t)y * W + ax] != 0 && wimg[(size_t)ay * W + x] != 0;
          if (ok) {
            ka = key[a];
            hit = ka != RT_NONE && ka + ((ck * (uint32_t)wimg[b]) << 4) == kb;
          }
        }
        const unsigned long long bal = __ballot(hit);
        if (!bal) { n = -1; break; }
        const int k = __ffsll((long long)bal) - 1;
        b = (uint32_t)__shfl((int)a, k, 64);
        kb = (uint32_t)__shfl((int)ka, k, 64);
      }
    }
  }
  if (lane == 0) len[g] = n;
}

// ---- host.  The context holds two instances of the result, tsd_ctx::route (one layer for all seeds) and tsd_ctx::fields (one layer
// per seed); every helper below takes the instance, and the instance's names say which entry speaks and which launches are timed.
struct RtNames { const char *who, *init, *relax, *goals, *trace; };
static const RtNames RT_ROUTE{"tsd_route", "route_init", "route_relax", "route_goals", "route_trace"};
static const RtNames RT_FIELDS{"tsd_route_fields", "route_fields_init", "route_fields_relax", "route_fields_goals", "route_fields_trace"};
static const RtNames& rt_names(const tsd_ctx* ctx, const tsd_ctx::Route& r) { return &r == &ctx->fields ? RT_FIELDS : RT_ROUTE; }

static const char* rt_params_wrong(const tsd_route_params* p, const void* info)
{
  if (!p) return "params is NULL";
  if (!info) return "info is NULL";
  if (p->free_max < 0 || p->free_max > 99) return "free_max is outside 0 .. 99";
  if (p->n_seeds < 1 || p->n_seeds > TSD_FRONTIER_MAX_SEEDS) return "n_seeds is outside 1 .. TSD_FRONTIER_MAX_SEEDS";
  if (!p->seeds_xy) return "seeds_xy is NULL";
  if (p->weights)
    for (int v = 0; v <= p->free_max; v++)
      if (p->weights[v] == 0) return "a weight is 0";
  if (p->limit > TSD_ROUTE_MAX_DIST) return "limit is above TSD_ROUTE_MAX_DIST";
  if (p->max_rounds < 0 || p->max_rounds > TSD_ROUTE_MAX_ROUNDS) return "max_rounds is outside 0 .. TSD_ROUTE_MAX_ROUNDS";
  return nullptr;
}

// The keys of instance r on the source's stream, entered here, which it waits for: one layer for all seeds, or (fields) one layer per
// seed.  The caller has checked the arguments.  *info is the fields' form; a route call reads its own four values out of it.
static int run_route(tsd_ctx* ctx, tsd_ctx::Route& r, const MapSource& src, const tsd_route_params* prm, bool fields, tsd_route_fields_info* info)
{
  if (int rc = map_source_enter(ctx, src)) return rc;
  const RtNames& nm = rt_names(ctx, r);
  r.valid = false; r.n_goals = -1;                     // (no result until this call has one: none where an allocation below fails)
  const auto& [m, stream, timed] = src;
  const int W = m.W, H = m.H, tw = (W + 31) / 32, th = (H + 31) / 32, L = fields ? prm->n_seeds : 1;
  const size_t cells = (size_t)W * H, tiles = (size_t)tw * th;
  if (int rc = scratch_grow(ctx, nm.who, &r.d_key, &r.keys, cells * L, "the key image")) return rc;
  if (int rc = scratch_grow(ctx, nm.who, &r.d_w, &r.cells, cells, "the cells' weights")) return rc;
  if (int rc = scratch_grow(ctx, nm.who, &r.d_act, &r.tiles, 2 * tiles * L, "the tile bytes")) return rc;
  if (!r.d_res) TSD_HIP_CHECK(ctx, hipMalloc(&r.d_res, RT_RES_WORDS * sizeof(uint32_t)));
  if (!r.h_res) TSD_HIP_CHECK(ctx, hipHostMalloc(&r.h_res, RT_RES_WORDS * sizeof(uint32_t), hipHostMallocDefault));

  RtWeights wt{};
  for (int v = 0; v <= prm->free_max; v++) wt.w[v] = prm->weights ? prm->weights[v] : (uint8_t)1;
  const MapSeeds sd = map_seeds(prm->n_seeds, prm->seeds_xy);
  const uint32_t limit = prm->limit ? prm->limit : TSD_ROUTE_MAX_DIST;
  const uint32_t lim_key = (limit << 4) | 15u;
  const int max_rounds = prm->max_rounds ? prm->max_rounds : 16 * (tw + th) + 64;
  const int sweeps = ctx->route.sweeps > 0 ? ctx->route.sweeps : RT_SWEEPS;      // (the test hook holds for both instances)
  uint8_t* act[2] = {r.d_act, r.d_act + tiles * L};
  const dim3 tg(tw, th, L);
  unsigned long long* visits = reinterpret_cast<unsigned long long*>(r.d_res + RT_RES_VISITS);

  TSD_HIP_CHECK(ctx, hipMemsetAsync(r.d_res, 0, RT_RES_WORDS * sizeof(uint32_t), stream));
  {
    ScopedKernelTimer t(ctx, timed ? nm.init : "", true);
    hipLaunchKernelGGL(k_route_init, tg, dim3(256), 0, stream, m, wt, sd, fields ? 1 : 0, cells, tiles, r.d_key, r.d_w, act[0], act[1], r.d_res);
  }
  int rounds = 0, waits = 0, converged = 0;
  for (int batch = 0; rounds < max_rounds && !converged; batch++) {
    const int nb = std::min(batch == 0 ? RT_BATCH / 4 : batch == 1 ? RT_BATCH / 2 : RT_BATCH, max_rounds - rounds);
    {
      ScopedKernelTimer t(ctx, timed ? nm.relax : "", true);
      for (int i = 0; i < nb; i++, rounds++) {
        // the word says whether the batch's LAST round left a tile active on any layer: cleared in front of that round only
        if (i == nb - 1) TSD_HIP_CHECK(ctx, hipMemsetAsync(r.d_res + RT_RES_ANY, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(fields ? k_route_relax<true> : k_route_relax<false>, tg, dim3(256), 0, stream, r.d_key, r.d_w, act[rounds & 1],
                           act[(rounds + 1) & 1], W, H, cells, tiles, lim_key, sweeps, r.d_res + RT_RES_ANY, visits);
      }
    }
    TSD_HIP_CHECK(ctx, hipGetLastError());
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_res + RT_RES_ANY, r.d_res + RT_RES_ANY, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    waits++;
    converged = r.h_res[RT_RES_ANY] == 0u ? 1 : 0;
  }
  hipLaunchKernelGGL(k_route_count, tg, dim3(256), 0, stream, r.d_key, W, H, cells, r.d_res + RT_RES_REACHED);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_res, r.d_res, RT_RES_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
  waits++;
  r.valid = true; r.W = W; r.H = H; r.layers = L; r.stream = stream;
  std::memcpy(&r.tile_visits, r.h_res + RT_RES_VISITS, sizeof(long long));
  r.host_waits = waits;
  *info = tsd_route_fields_info{};
  info->layers = L;
  info->rounds = rounds;
  info->converged = converged;
  info->seeds_used = __builtin_popcount(r.h_res[RT_RES_USED]);
  for (int i = 0; i < TSD_FRONTIER_MAX_SEEDS; i++) {
    info->used[i] = (uint8_t)((r.h_res[RT_RES_USED] >> i) & 1u);
    info->reached[i] = i < L ? r.h_res[RT_RES_REACHED + i] : 0u;
  }
  return TSD_OK;
}

static int run_route_one(tsd_ctx* ctx, const MapSource& src, const tsd_route_params* prm, tsd_route_info* info)
{
  tsd_route_fields_info fi{};
  if (int rc = run_route(ctx, ctx->route, src, prm, false, &fi)) return rc;
  *info = tsd_route_info{fi.seeds_used, fi.rounds, fi.converged, fi.reached[0]};
  return TSD_OK;
}

// nullptr, or why the layers of n_goals goals are refused on instance r
const char* route_goal_layers_wrong(const tsd_ctx::Route& r, const uint8_t* goal_layers, int n_goals)
{
  if (!goal_layers) return "goal_layers is NULL";
  for (int g = 0; g < n_goals; g++)
    if ((int)goal_layers[g] >= r.layers) return "a goal's layer is not below the result's layers";
  return nullptr;
}

// The trace of n_goals cells on the stream of instance r's result, into r's scratch and not waited for: what the trace entries copy
// back and what the waypoint entries (waypoint.hip) work on in place.  d_path holds the goal cells, the lengths, the paths and, where
// goal_layers is given, the goals' layer bytes, in this order.  The caller has checked the arguments and set the device.  Out of
// memory takes r's result and its goals along.
int route_trace_enqueue(tsd_ctx* ctx, tsd_ctx::Route& r, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals, int max_len,
                        RouteTrace* out)
{
  const RtNames& nm = rt_names(ctx, r);
  const size_t ng = (size_t)n_goals, head = 2 * ng + ng * (size_t)max_len;
  const int rc = scratch_grow(ctx, nm.who, &r.d_path, &r.path_words, head + (goal_layers ? (ng + 3) / 4 : 0), "the paths");
  if (rc == TSD_E_NOMEM) { r.valid = false; r.n_goals = -1; }
  if (rc) return rc;
  uint32_t* d_goals = r.d_path;
  int32_t* d_len = reinterpret_cast<int32_t*>(r.d_path + ng);
  uint32_t* d_paths = r.d_path + 2 * ng;
  uint8_t* d_layers = goal_layers ? reinterpret_cast<uint8_t*>(r.d_path + head) : nullptr;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(d_goals, goal_cells, ng * sizeof(uint32_t), hipMemcpyHostToDevice, r.stream));
  if (goal_layers) TSD_HIP_CHECK(ctx, hipMemcpyAsync(d_layers, goal_layers, ng, hipMemcpyHostToDevice, r.stream));
  {
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? nm.trace : "", true);
    hipLaunchKernelGGL(d_layers ? k_route_trace<true> : k_route_trace<false>, dim3((unsigned)n_goals), dim3(64), 0, r.stream, r.d_key, r.d_w, r.W,
                       r.H, d_goals, d_layers, (size_t)r.W * r.H, max_len, d_paths, d_len);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  *out = RouteTrace{d_goals, d_len, d_paths, d_layers};
  return TSD_OK;
}

static void route_free_one(tsd_ctx::Route& r)
{
  hipFree(r.d_key); hipFree(r.d_w); hipFree(r.d_act); hipFree(r.d_goal); hipFree(r.d_path); hipFree(r.d_res); hipFree(r.d_way);
  if (r.h_path) hipHostFree(r.h_path);
  if (r.h_way) hipHostFree(r.h_way);
  if (r.h_res) hipHostFree(r.h_res);
  r = tsd_ctx::Route{};
}

void route_free(tsd_ctx* ctx)
{
  route_free_one(ctx->route);
  route_free_one(ctx->fields);
}

// The goals of the frontier result on instance r's keys: the matrix [r.layers][n], one row per layer.
static int route_goals(tsd_ctx* ctx, tsd_ctx::Route& r, const char* who, int* n)
{
  const RtNames& nm = rt_names(ctx, r);
  const tsd_ctx::Frontier& f = ctx->frontier;
  if (!n) return map_refused(ctx, who, "n is NULL");
  if (!r.valid) return map_refused(ctx, who, "no route result");
  if (f.n < 0) return map_refused(ctx, who, "no frontier result");
  if (f.W != r.W || f.H != r.H) return map_refused(ctx, who, "the frontier result and the route result differ in size");
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  r.n_goals = -1;
  const size_t all = (size_t)f.n * r.layers;
  const int rc = scratch_grow(ctx, nm.who, &r.d_goal, &r.goals, std::max<size_t>(all, 1), "the goals");
  if (rc == TSD_E_NOMEM) r.valid = false;              // out of memory takes the route result along with the goals
  if (rc) return rc;
  if (f.n > 0) {
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(r.d_goal);
    const unsigned nb = (unsigned)((all + 255) / 256);
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? nm.goals : "", true);
    hipLaunchKernelGGL(k_route_goals_init, dim3(nb), dim3(256), 0, r.stream, slots, (int)all);
    hipLaunchKernelGGL(k_route_goals, dim3((r.W + 31) / 32, (r.H + 31) / 32), dim3(256), 0, r.stream, f.d_lab, r.d_key, (size_t)r.W * r.H, r.layers,
                       f.d_rec, f.n, r.W, r.H, slots);
    hipLaunchKernelGGL(k_route_goals_emit, dim3(nb), dim3(256), 0, r.stream, slots, (int)all);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  r.n_goals = f.n;
  *n = f.n;
  return TSD_OK;
}

static int route_goals_fetch(tsd_ctx* ctx, const tsd_ctx::Route& r, const char* who, int layer, int first, int count, tsd_route_goal* out)
{
  if (!r.valid || r.n_goals < 0) return map_refused(ctx, who, "no goals to fetch");
  if (layer < 0 || layer >= r.layers) return map_refused(ctx, who, "layer is outside 0 .. layers - 1");
  if (const char* why = fetch_range_wrong(first, count, r.n_goals, out)) return map_refused(ctx, who, why);
  if (count == 0) return TSD_OK;
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  TSD_HIP_CHECK(ctx, hipMemcpy(out, r.d_goal + (size_t)layer * r.n_goals + first, (size_t)count * sizeof(tsd_route_goal), hipMemcpyDeviceToHost));
  return TSD_OK;
}

// goal_layers: nullptr for the route entry (every goal on the one layer)
static int route_trace(tsd_ctx* ctx, tsd_ctx::Route& r, const char* who, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals,
                       int max_len, uint32_t* paths_host, int32_t* len_host)
{
  const RtNames& nm = rt_names(ctx, r);
  if (!goal_cells || !paths_host || !len_host || n_goals < 1 || n_goals > TSD_ROUTE_MAX_GOALS || max_len < 1 ||
      (long long)n_goals * max_len > (1ll << 24))
    return map_refused(ctx, who, "a null argument, n_goals outside 1 .. TSD_ROUTE_MAX_GOALS, max_len < 1 or n_goals * max_len > 1 << 24");
  if (!r.valid) return map_refused(ctx, who, "no route result");
  if (&r == &ctx->fields)
    if (const char* why = route_goal_layers_wrong(r, goal_layers, n_goals)) return map_refused(ctx, who, why);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // h_path: the lengths, the paths
  const size_t ng = (size_t)n_goals, back = ng + ng * (size_t)max_len;
  if (int rc = scratch_grow(ctx, nm.who, &r.h_path, &r.h_path_words, back, "the paths' pinned copy", true)) {
    if (rc == TSD_E_NOMEM) { r.valid = false; r.n_goals = -1; }        // out of memory takes the route result and its goals along
    return rc;
  }
  RouteTrace tr{};
  if (int rc = route_trace_enqueue(ctx, r, goal_cells, goal_layers, n_goals, max_len, &tr)) return rc;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_path, tr.d_len, back * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream));   // (the lengths, then the paths)
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  const int32_t* h_len = reinterpret_cast<const int32_t*>(r.h_path);
  for (size_t g = 0; g < ng; g++) {
    len_host[g] = h_len[g];
    const size_t n = (size_t)std::min(std::max(h_len[g], 0), max_len);
    if (n) std::memcpy(paths_host + g * (size_t)max_len, r.h_path + ng + g * (size_t)max_len, n * sizeof(uint32_t));
  }
  return TSD_OK;
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_route_weights(int free_max, int max_weight, uint8_t* table)
{
  if (!table || free_max < 0 || free_max > 99 || max_weight < 1 || max_weight > 255) return TSD_E_ARG;
  for (int v = 0; v <= free_max; v++) table[v] = (uint8_t)std::min(255, 1 + v * (max_weight - 1) / 98);   // (v = 99 alone can pass 255)
  return TSD_OK;
}

int tsd_route_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_route_params* params, tsd_route_info* info)
{
  if (!ctx) return TSD_E_ARG;
  MapSource src{};
  if (int rc = map_source_caller(ctx, "tsd_route_dev", map_dev, width, height, stride, &src)) return rc;
  if (const char* why = rt_params_wrong(params, info)) return map_refused(ctx, "tsd_route_dev", why);
  return run_route_one(ctx, src, params, info);
}

int tsd_route_frame(tsd_ctx* ctx, int source, const tsd_route_params* params, tsd_route_info* info)
{
  if (!ctx) return TSD_E_ARG;
  if (source != TSD_ROUTE_MAP && source != TSD_ROUTE_COSTMAP) return set_error(ctx, TSD_E_ARG, "tsd_route_frame: no such source", hipSuccess);
  if (const char* why = rt_params_wrong(params, info)) return map_refused(ctx, "tsd_route_frame", why);
  MapSource src{};
  if (int rc = map_source_frame(ctx, "tsd_route_frame", source == TSD_ROUTE_COSTMAP, &src)) return rc;
  return run_route_one(ctx, src, params, info);
}

int tsd_route_fields_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_route_params* params,
                         tsd_route_fields_info* info)
{
  if (!ctx) return TSD_E_ARG;
  MapSource src{};
  if (int rc = map_source_caller(ctx, "tsd_route_fields_dev", map_dev, width, height, stride, &src)) return rc;
  if (const char* why = rt_params_wrong(params, info)) return map_refused(ctx, "tsd_route_fields_dev", why);
  return run_route(ctx, ctx->fields, src, params, true, info);
}

int tsd_route_fields_frame(tsd_ctx* ctx, int source, const tsd_route_params* params, tsd_route_fields_info* info)
{
  if (!ctx) return TSD_E_ARG;
  if (source != TSD_ROUTE_MAP && source != TSD_ROUTE_COSTMAP) return set_error(ctx, TSD_E_ARG, "tsd_route_fields_frame: no such source", hipSuccess);
  if (const char* why = rt_params_wrong(params, info)) return map_refused(ctx, "tsd_route_fields_frame", why);
  MapSource src{};
  if (int rc = map_source_frame(ctx, "tsd_route_fields_frame", source == TSD_ROUTE_COSTMAP, &src)) return rc;
  return run_route(ctx, ctx->fields, src, params, true, info);
}

int tsd_route_goals(tsd_ctx* ctx, int* n)
{
  if (!ctx) return TSD_E_ARG;
  return route_goals(ctx, ctx->route, "tsd_route_goals", n);
}

int tsd_route_fields_goals(tsd_ctx* ctx, int* n)
{
  if (!ctx) return TSD_E_ARG;
  return route_goals(ctx, ctx->fields, "tsd_route_fields_goals", n);
}

int tsd_route_goals_fetch(tsd_ctx* ctx, int first, int count, tsd_route_goal* out)
{
  if (!ctx) return TSD_E_ARG;
  return route_goals_fetch(ctx, ctx->route, "tsd_route_goals_fetch", 0, first, count, out);
}

int tsd_route_fields_goals_fetch(tsd_ctx* ctx, int layer, int first, int count, tsd_route_goal* out)
{
  if (!ctx) return TSD_E_ARG;
  return route_goals_fetch(ctx, ctx->fields, "tsd_route_fields_goals_fetch", layer, first, count, out);
}

int tsd_route_trace(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, int max_len, uint32_t* paths_host, int32_t* len_host)
{
  if (!ctx) return TSD_E_ARG;
  return route_trace(ctx, ctx->route, "tsd_route_trace", goal_cells, nullptr, n_goals, max_len, paths_host, len_host);
}

int tsd_route_fields_trace(tsd_ctx* ctx, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals, int max_len, uint32_t* paths_host,
                           int32_t* len_host)
{
  if (!ctx) return TSD_E_ARG;
  return route_trace(ctx, ctx->fields, "tsd_route_fields_trace", goal_cells, goal_layers, n_goals, max_len, paths_host, len_host);
}

int tsd_route_dev_ptrs(tsd_ctx* ctx, const void** keys_dev, int* width, int* height)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Route& r = ctx->route;
  if (!r.valid) return set_error(ctx, TSD_E_ARG, "tsd_route_dev_ptrs: no result", hipSuccess);
  if (keys_dev) *keys_dev = r.d_key;
  if (width) *width = r.W;
  if (height) *height = r.H;
  return TSD_OK;
}

int tsd_route_fields_dev_ptrs(tsd_ctx* ctx, const void** keys_dev, int* width, int* height, int* layers)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Route& r = ctx->fields;
  if (!r.valid) return set_error(ctx, TSD_E_ARG, "tsd_route_fields_dev_ptrs: no result", hipSuccess);
  if (keys_dev) *keys_dev = r.d_key;
  if (width) *width = r.W;
  if (height) *height = r.H;
  if (layers) *layers = r.layers;
  return TSD_OK;
}

static int route_counts(tsd_ctx* ctx, const tsd_ctx::Route& r, const char* who, long long* tile_visits, int* host_waits)
{
  if (!r.valid) return map_refused(ctx, who, "no result");
  if (tile_visits) *tile_visits = r.tile_visits;
  if (host_waits) *host_waits = r.host_waits;
  return TSD_OK;
}

int tsd_route_counts(tsd_ctx* ctx, long long* tile_visits, int* host_waits)
{
  if (!ctx) return TSD_E_ARG;
  return route_counts(ctx, ctx->route, "tsd_route_counts", tile_visits, host_waits);
}

int tsd_route_fields_counts(tsd_ctx* ctx, long long* tile_visits, int* host_waits)
{
  if (!ctx) return TSD_E_ARG;
  return route_counts(ctx, ctx->fields, "tsd_route_fields_counts", tile_visits, host_waits);
}

int tsd_debug_set_route_sweeps(tsd_ctx* ctx, int n)
{
  if (!ctx) return TSD_E_ARG;
  ctx->route.sweeps = n > 0 ? n : 0;
  return TSD_OK;
}

}  // extern "C"
