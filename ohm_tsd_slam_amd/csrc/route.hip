// route.hip -- the cost-to-go field of an int8 map from up to 16 seed cells, the cheapest cell of every frontier and the paths
// (tsd_route_dev / _frame / _goals / _trace / _dev_ptrs of include/tsd_hip.h, where the rule is written out).  All in integers:
//
// k_route_init   one workgroup per 32 x 32 tile: every key of the image (a seed's cell its index, the lowest where two share a cell,
//                RT_NONE elsewhere), every cell's weight byte (W[v] on a traversable cell, 0 elsewhere: what the later passes read in
//                place of the map, so the map may go once the call has returned), the tile's two "active" bytes for round 0.
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
#include "map_product.hpp"

#include <algorithm>
#include <cstring>

namespace tsd {

constexpr uint32_t RT_NONE = TSD_ROUTE_NONE;
constexpr int RT_P = 34;                             // the pitch of a tile with its apron in LDS
constexpr int RT_SWEEPS = 2048;                      // sweeps per launch before a tile hands itself on to the next round
constexpr int RT_BATCH = 32;                         // rounds between two reads of the "any" word (8 and 16 for the first two batches)
constexpr const char* RT_WHO = "tsd_route";          // the scratch's owner in an out-of-memory message
// d_res / h_res, in uint32 (the visits are one uint64)
constexpr int RT_RES_USED = 0, RT_RES_REACHED = 1, RT_RES_ANY = 2, RT_RES_VISITS = 4, RT_RES_WORDS = 8;

struct RtWeights { uint8_t w[128]; };                // by map value; 0 above free_max

#define RT_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define RT_AGENT __HIP_MEMORY_SCOPE_AGENT

// neighbour k of the rule: (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (1,-1) (-1,1) (1,1)
__device__ __forceinline__ int rt_dx(int k) { return k < 4 ? (k == 0 ? -1 : k == 1 ? 1 : 0) : ((k & 1) ? 1 : -1); }
__device__ __forceinline__ int rt_dy(int k) { return k < 4 ? (k == 2 ? -1 : k == 3 ? 1 : 0) : ((k & 2) ? 1 : -1); }

// ---- init
__global__ void __launch_bounds__(256)
k_route_init(MapView m, RtWeights wt, MapSeeds sd, uint32_t* __restrict__ key, uint8_t* __restrict__ wimg, uint8_t* __restrict__ act0,
             uint8_t* __restrict__ act1, uint32_t* __restrict__ res)
{
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
      for (int i = sd.n - 1; i >= 0; i--)
        if (sd.xy[2 * i] == gx && sd.xy[2 * i + 1] == gy) k = (uint32_t)i;
    const size_t me = (size_t)gy * m.W + gx;
    key[me] = k;
    wimg[me] = w;
    some |= k != RT_NONE ? 1 : 0;
  }
  some = __syncthreads_or(some);
  if (t == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    act0[tile] = (uint8_t)(some ? 1 : 0);
    act1[tile] = 0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && t < 64) {            // (one whole wave)
    bool used = false;
    if (t < sd.n) {
      const int x = sd.xy[2 * t], y = sd.xy[2 * t + 1];
      if (x >= 0 && x < m.W && y >= 0 && y < m.H) {
        const int v = m.map[(size_t)y * m.stride + x];
        used = v >= 0 && s_wt[v] != 0;
      }
    }
    const unsigned long long bal = __ballot(used);
    if (t == 0) res[RT_RES_USED] = (uint32_t)__popcll(bal);
  }
}

// ---- one round
__global__ void __launch_bounds__(256)
k_route_relax(uint32_t* key, const uint8_t* __restrict__ wimg, uint8_t* act_cur, uint8_t* act_next, int W, int H, uint32_t lim_key,
              int max_sweeps, uint32_t* any, unsigned long long* visits)
{
  const int tw = (int)gridDim.x, th = (int)gridDim.y, tx = (int)blockIdx.x, ty = (int)blockIdx.y;
  const size_t tile = (size_t)ty * tw + tx;
  if (!act_cur[tile]) return;                        // (the same byte for every lane; it is cleared behind the barrier below)
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
k_route_count(const uint32_t* __restrict__ key, int W, int H, uint32_t* __restrict__ reached)
{
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

// ---- goals.  A slot is the first 8 bytes of its tsd_route_goal: (key << 32) | cell, all ones while no cell has lowered it.
__global__ void __launch_bounds__(256)
k_route_goals_init(unsigned long long* __restrict__ slots, int n)
{
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) slots[2 * (size_t)i] = ~0ull;
}

__global__ void __launch_bounds__(256)
k_route_goals(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ key, const tsd_frontier* __restrict__ rec, int n, int W, int H,
              unsigned long long* slots)
{
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = (int)threadIdx.x + 256 * j;
    const int x = (int)blockIdx.x * 32 + (c & 31), y = (int)blockIdx.y * 32 + (c >> 5);
    if (x >= W || y >= H) continue;
    const uint32_t me = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    const uint32_t root = lab[me];
    if (root == TSD_FRONTIER_NONE) continue;
    const uint32_t k = key[me];
    if (k == RT_NONE) continue;
    // the records are in ascending root index; a root that min_size dropped is not among them
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const uint32_t r = (uint32_t)rec[mid].root_y * (uint32_t)W + (uint32_t)rec[mid].root_x;
      if (r < root) lo = mid + 1; else hi = mid;
    }
    if (lo < n && (uint32_t)rec[lo].root_y * (uint32_t)W + (uint32_t)rec[lo].root_x == root)
      atomicMin(slots + 2 * (size_t)lo, ((unsigned long long)k << 32) | me);
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

// ---- trace: one wave per goal
__global__ void __launch_bounds__(64)
k_route_trace(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, int W, int H, const uint32_t* __restrict__ goals, int max_len,
              uint32_t* __restrict__ paths, int32_t* __restrict__ len)
{
  const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
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

// ---- host
static const char* rt_params_wrong(const tsd_route_params* p, const tsd_route_info* info)
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

// The field on the source's stream, entered here, which it waits for.  The caller has checked the arguments.
static int run_route(tsd_ctx* ctx, const MapSource& src, const tsd_route_params* prm, tsd_route_info* info)
{
  if (int rc = map_source_enter(ctx, src)) return rc;
  tsd_ctx::Route& r = ctx->route;
  r.valid = false; r.n_goals = -1;                     // (no result until this call has one: none where an allocation below fails)
  const auto& [m, stream, timed] = src;
  const int W = m.W, H = m.H, tw = (W + 31) / 32, th = (H + 31) / 32;
  const size_t cells = (size_t)W * H, tiles = (size_t)tw * th;
  if (int rc = scratch_grow_all(ctx, RT_WHO, &r.cells, cells, scratch_part(&r.d_key, "the key image"), scratch_part(&r.d_w, "the cells' weights")))
    return rc;
  if (int rc = scratch_grow_all(ctx, RT_WHO, &r.tiles, tiles, scratch_part(&r.d_act, "the tile bytes", false, 2))) return rc;
  if (!r.d_res) TSD_HIP_CHECK(ctx, hipMalloc(&r.d_res, RT_RES_WORDS * sizeof(uint32_t)));
  if (!r.h_res) TSD_HIP_CHECK(ctx, hipHostMalloc(&r.h_res, RT_RES_WORDS * sizeof(uint32_t), hipHostMallocDefault));

  RtWeights wt{};
  for (int v = 0; v <= prm->free_max; v++) wt.w[v] = prm->weights ? prm->weights[v] : (uint8_t)1;
  const MapSeeds sd = map_seeds(prm->n_seeds, prm->seeds_xy);
  const uint32_t limit = prm->limit ? prm->limit : TSD_ROUTE_MAX_DIST;
  const uint32_t lim_key = (limit << 4) | 15u;
  const int max_rounds = prm->max_rounds ? prm->max_rounds : 16 * (tw + th) + 64;
  const int sweeps = r.sweeps > 0 ? r.sweeps : RT_SWEEPS;
  uint8_t* act[2] = {r.d_act, r.d_act + r.tiles};
  const dim3 tg(tw, th);
  unsigned long long* visits = reinterpret_cast<unsigned long long*>(r.d_res + RT_RES_VISITS);

  TSD_HIP_CHECK(ctx, hipMemsetAsync(r.d_res, 0, RT_RES_WORDS * sizeof(uint32_t), stream));
  {
    ScopedKernelTimer t(ctx, timed ? "route_init" : "", true);
    hipLaunchKernelGGL(k_route_init, tg, dim3(256), 0, stream, m, wt, sd, r.d_key, r.d_w, act[0], act[1], r.d_res);
  }
  int rounds = 0, waits = 0, converged = 0;
  for (int batch = 0; rounds < max_rounds && !converged; batch++) {
    const int nb = std::min(batch == 0 ? RT_BATCH / 4 : batch == 1 ? RT_BATCH / 2 : RT_BATCH, max_rounds - rounds);
    {
      ScopedKernelTimer t(ctx, timed ? "route_relax" : "", true);
      for (int i = 0; i < nb; i++, rounds++) {
        // the word says whether the batch's LAST round left a tile active: cleared in front of that round only
        if (i == nb - 1) TSD_HIP_CHECK(ctx, hipMemsetAsync(r.d_res + RT_RES_ANY, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_route_relax, tg, dim3(256), 0, stream, r.d_key, r.d_w, act[rounds & 1], act[(rounds + 1) & 1], W, H, lim_key,
                           sweeps, r.d_res + RT_RES_ANY, visits);
      }
    }
    TSD_HIP_CHECK(ctx, hipGetLastError());
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_res + RT_RES_ANY, r.d_res + RT_RES_ANY, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
    waits++;
    converged = r.h_res[RT_RES_ANY] == 0u ? 1 : 0;
  }
  hipLaunchKernelGGL(k_route_count, tg, dim3(256), 0, stream, r.d_key, W, H, r.d_res + RT_RES_REACHED);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_res, r.d_res, RT_RES_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
  waits++;
  r.valid = true; r.W = W; r.H = H; r.stream = stream;
  std::memcpy(&r.tile_visits, r.h_res + RT_RES_VISITS, sizeof(long long));
  r.host_waits = waits;
  info->seeds_used = (int32_t)r.h_res[RT_RES_USED];
  info->rounds = rounds;
  info->converged = converged;
  info->reached = r.h_res[RT_RES_REACHED];
  return TSD_OK;
}

// The trace of n_goals cells on the route result's stream, into the route's scratch and not waited for: what tsd_route_trace copies
// back and what tsd_route_waypoints (waypoint.hip) works on in place.  d_path holds the goal cells, the lengths, the paths, in this
// order.  The caller has checked the arguments and set the device.  Out of memory takes the route result and its goals along.
int route_trace_enqueue(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, int max_len, RouteTrace* out)
{
  tsd_ctx::Route& r = ctx->route;
  const size_t ng = (size_t)n_goals;
  const int rc = scratch_grow(ctx, RT_WHO, &r.d_path, &r.path_words, 2 * ng + ng * (size_t)max_len, "the paths");
  if (rc == TSD_E_NOMEM) { r.valid = false; r.n_goals = -1; }
  if (rc) return rc;
  uint32_t* d_goals = r.d_path;
  int32_t* d_len = reinterpret_cast<int32_t*>(r.d_path + ng);
  uint32_t* d_paths = r.d_path + 2 * ng;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(d_goals, goal_cells, ng * sizeof(uint32_t), hipMemcpyHostToDevice, r.stream));
  {
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? "route_trace" : "", true);
    hipLaunchKernelGGL(k_route_trace, dim3((unsigned)n_goals), dim3(64), 0, r.stream, r.d_key, r.d_w, r.W, r.H, d_goals, max_len, d_paths, d_len);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  *out = RouteTrace{d_goals, d_len, d_paths};
  return TSD_OK;
}

void route_free(tsd_ctx* ctx)
{
  tsd_ctx::Route& r = ctx->route;
  hipFree(r.d_key); hipFree(r.d_w); hipFree(r.d_act); hipFree(r.d_goal); hipFree(r.d_path); hipFree(r.d_res); hipFree(r.d_way);
  if (r.h_path) hipHostFree(r.h_path);
  if (r.h_way) hipHostFree(r.h_way);
  if (r.h_res) hipHostFree(r.h_res);
  r = tsd_ctx::Route{};
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
  return run_route(ctx, src, params, info);
}

int tsd_route_frame(tsd_ctx* ctx, int source, const tsd_route_params* params, tsd_route_info* info)
{
  if (!ctx) return TSD_E_ARG;
  if (source != TSD_ROUTE_MAP && source != TSD_ROUTE_COSTMAP) return set_error(ctx, TSD_E_ARG, "tsd_route_frame: no such source", hipSuccess);
  if (const char* why = rt_params_wrong(params, info)) return map_refused(ctx, "tsd_route_frame", why);
  MapSource src{};
  if (int rc = map_source_frame(ctx, "tsd_route_frame", source == TSD_ROUTE_COSTMAP, &src)) return rc;
  return run_route(ctx, src, params, info);
}

int tsd_route_goals(tsd_ctx* ctx, int* n)
{
  if (!ctx) return TSD_E_ARG;
  tsd_ctx::Route& r = ctx->route;
  const tsd_ctx::Frontier& f = ctx->frontier;
  if (!n) return set_error(ctx, TSD_E_ARG, "tsd_route_goals: n is NULL", hipSuccess);
  if (!r.valid) return set_error(ctx, TSD_E_ARG, "tsd_route_goals: no route result", hipSuccess);
  if (f.n < 0) return set_error(ctx, TSD_E_ARG, "tsd_route_goals: no frontier result", hipSuccess);
  if (f.W != r.W || f.H != r.H) return set_error(ctx, TSD_E_ARG, "tsd_route_goals: the frontier result and the route result differ in size", hipSuccess);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  r.n_goals = -1;
  const int rc = scratch_grow(ctx, RT_WHO, &r.d_goal, &r.goals, std::max<size_t>((size_t)f.n, 1), "the goals");
  if (rc == TSD_E_NOMEM) r.valid = false;              // out of memory takes the route result along with the goals
  if (rc) return rc;
  if (f.n > 0) {
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(r.d_goal);
    const unsigned nb = (unsigned)((f.n + 255) / 256);
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? "route_goals" : "", true);
    hipLaunchKernelGGL(k_route_goals_init, dim3(nb), dim3(256), 0, r.stream, slots, f.n);
    hipLaunchKernelGGL(k_route_goals, dim3((r.W + 31) / 32, (r.H + 31) / 32), dim3(256), 0, r.stream, f.d_lab, r.d_key, f.d_rec, f.n, r.W, r.H, slots);
    hipLaunchKernelGGL(k_route_goals_emit, dim3(nb), dim3(256), 0, r.stream, slots, f.n);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  r.n_goals = f.n;
  *n = f.n;
  return TSD_OK;
}

int tsd_route_goals_fetch(tsd_ctx* ctx, int first, int count, tsd_route_goal* out)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Route& r = ctx->route;
  if (!r.valid || r.n_goals < 0) return set_error(ctx, TSD_E_ARG, "tsd_route_goals_fetch: no goals to fetch", hipSuccess);
  if (const char* why = fetch_range_wrong(first, count, r.n_goals, out)) return map_refused(ctx, "tsd_route_goals_fetch", why);
  if (count == 0) return TSD_OK;
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  TSD_HIP_CHECK(ctx, hipMemcpy(out, r.d_goal + first, (size_t)count * sizeof(tsd_route_goal), hipMemcpyDeviceToHost));
  return TSD_OK;
}

int tsd_route_trace(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, int max_len, uint32_t* paths_host, int32_t* len_host)
{
  if (!ctx) return TSD_E_ARG;
  tsd_ctx::Route& r = ctx->route;
  if (!goal_cells || !paths_host || !len_host || n_goals < 1 || n_goals > TSD_ROUTE_MAX_GOALS || max_len < 1 ||
      (long long)n_goals * max_len > (1ll << 24))
    return set_error(ctx, TSD_E_ARG, "tsd_route_trace: a null argument, n_goals outside 1 .. TSD_ROUTE_MAX_GOALS, max_len < 1 or n_goals * max_len > 1 << 24",
                     hipSuccess);
  if (!r.valid) return set_error(ctx, TSD_E_ARG, "tsd_route_trace: no route result", hipSuccess);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // h_path: the lengths, the paths
  const size_t ng = (size_t)n_goals, back = ng + ng * (size_t)max_len;
  if (int rc = scratch_grow(ctx, RT_WHO, &r.h_path, &r.h_path_words, back, "the paths' pinned copy", true)) {
    if (rc == TSD_E_NOMEM) { r.valid = false; r.n_goals = -1; }        // out of memory takes the route result and its goals along
    return rc;
  }
  RouteTrace tr{};
  if (int rc = route_trace_enqueue(ctx, goal_cells, n_goals, max_len, &tr)) return rc;
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

int tsd_route_counts(tsd_ctx* ctx, long long* tile_visits, int* host_waits)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Route& r = ctx->route;
  if (!r.valid) return set_error(ctx, TSD_E_ARG, "tsd_route_counts: no result", hipSuccess);
  if (tile_visits) *tile_visits = r.tile_visits;
  if (host_waits) *host_waits = r.host_waits;
  return TSD_OK;
}

int tsd_debug_set_route_sweeps(tsd_ctx* ctx, int n)
{
  if (!ctx) return TSD_E_ARG;
  ctx->route.sweeps = n > 0 ? n : 0;
  return TSD_OK;
}

}  // extern "C"
