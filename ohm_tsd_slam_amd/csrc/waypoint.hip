// waypoint.hip -- a traced path straightened into waypoints joined by straight drivable segments (tsd_route_waypoints and
// tsd_route_fields_waypoints of include/tsd_hip.h, where the rule is written out).  All in integers.
//
// k_route_waypoints  one workgroup of 256 threads (four waves) per goal, launched behind k_route_trace on the same stream; it reads
//                    the trace's path where the trace left it (goal first: driving index i is path word len - 1 - i), and the keys
//                    of the layer the trace walked (layer_of_goal[g]; nullptr: layer 0 for every goal).
//   window     Per anchor p_a the cells p_a .. p_hi (hi = min(a + lookahead, len - 1)) go into LDS as x | y << 16 (a side is at most
//              32768) together with their d: 8 bytes per path cell, 8200 B at lookahead 1024.
//   pairs      A step's cell is a closed form of the step's number, so every (candidate, step) pair is independent: a lane loads the
//              cell it enters and, on a diagonal step, the two cells the step cuts -- three byte loads at most.  The division by 2N
//              is a multiplication by a reciprocal from a table in LDS, one entry per N, made once per workgroup: (n * r) >> 33
//              with r = ceil(2^33 / 2N) is n / 2N for every numerator n <= 2 N^2 + N of the rule at N <= 1024
//              (n * (r * 2N - 2^33) < 2^33).
//   screen     A wave takes four candidates at a time, 16 lanes each over the candidate's first 16 steps: one ballot says which of
//              the four have a refusal there.  In clutter most candidates end here, four per round of loads.
//   segment    A candidate the screen lets through is walked whole by the wave, the lanes over its steps in chunks of 64: a ballot
//              of the refusals, a shuffle sum of the costs.  No atomics on a candidate: the wave that owns it keeps the sum in
//              registers.  It ends at the first chunk with a refusal or with a partial sum above its bound (the costs are positive).
//   order      Wave w takes the groups of four hi - 4w, hi - 4w - 16, ... downwards and each group downwards, so the first
//              candidate of a wave that passes is the wave's largest; it leaves it in LDS and stops.  A wave also stops at a group
//              that is not above the largest candidate any wave has passed so far (one LDS word, raised with atomicMax): whatever
//              it skips lies below a candidate that passes, so the result -- the maximum over the waves behind one barrier -- is
//              the rule's largest j however the waves are scheduled.  Candidate a + 1 is not tested: it is a traced step and its
//              cost is the keys' difference.
//              In open space an anchor costs one screen and one segment per wave; where nothing passes, lookahead / 16 screens per
//              wave, each one round of independent loads.
//
// The workgroup's threads agree on every branch around a barrier: the anchor, the window and the outcome are read from LDS by all.
#include "map_product.hpp"

#include <algorithm>
#include <cstring>

namespace tsd {

constexpr int WP_THREADS = 256, WP_WAVES = WP_THREADS / 64;
constexpr int WP_MAX = TSD_WAYPOINT_MAX_LOOKAHEAD;

struct WpArgs {
  int W;                                             // the key image's width
  uint32_t cells;                                    // width * height
  int lookahead, max_len, max_way;
  uint32_t slack;
};

#define WP_WG __HIP_MEMORY_SCOPE_WORKGROUP

constexpr int WP_SCREEN = 16, WP_SIDE = 64 / WP_SCREEN;        // the screen: the first 16 steps of four candidates side by side in a wave

// The line from the anchor (ax, ay) to q: its signs, N, the minor axis' |d| and the reciprocal of 2N.
struct WpLine { int sx, sy, N; uint32_t M; bool xmaj; unsigned long long r; };

__device__ __forceinline__ WpLine wp_line(int ax, int ay, uint32_t q, const uint32_t* s_recip)
{
  const int dx = (int)(q & 0xFFFFu) - ax, dy = (int)(q >> 16) - ay;
  const int adx = abs(dx), ady = abs(dy);
  WpLine l;
  l.sx = (dx > 0) - (dx < 0); l.sy = (dy > 0) - (dy < 0);
  l.xmaj = adx >= ady;
  l.N = l.xmaj ? adx : ady;
  l.M = (uint32_t)(l.xmaj ? ady : adx);
  l.r = s_recip[l.N];
  return l;
}

// Step s (1 .. N) of the line: true where the step is refused; *cst: c * w of the cell entered.  Three byte loads at most.
__device__ __forceinline__ bool wp_step(const uint8_t* __restrict__ wimg, int W, int ax, int ay, const WpLine& l, int s, int* cst)
{
  const int om = (int)(((unsigned long long)(2u * (uint32_t)s * l.M + (uint32_t)l.N) * l.r) >> 33);
  const int op = (int)(((unsigned long long)(2u * (uint32_t)(s - 1) * l.M + (uint32_t)l.N) * l.r) >> 33);
  const int x = ax + l.sx * (l.xmaj ? s : om), y = ay + l.sy * (l.xmaj ? om : s);
  const int w = wimg[(size_t)y * W + x];                       // (inside the bounding box of two path cells: inside the map)
  bool bad = w == 0;
  const bool diag = om != op;
  if (diag) {                                                  // the two cells the step cuts
    const int xp = ax + l.sx * (l.xmaj ? s - 1 : op), yp = ay + l.sy * (l.xmaj ? op : s - 1);
    bad = bad || wimg[(size_t)yp * W + x] == 0 || wimg[(size_t)y * W + xp] == 0;
  }
  *cst = (diag ? 7 : 5) * w;
  return bad;
}

template <bool LAYERS>                                         // (false: layer 0 for every goal, layer_of_goal is not read)
__global__ void __launch_bounds__(WP_THREADS)
k_route_waypoints(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, WpArgs a, const uint32_t* __restrict__ goals,
                  const uint8_t* __restrict__ layer_of_goal, const int32_t* __restrict__ len, const uint32_t* __restrict__ paths,
                  uint32_t* __restrict__ way, tsd_waypoint_info* __restrict__ info)
{
  if constexpr (LAYERS) key += (size_t)__builtin_amdgcn_readfirstlane((int)layer_of_goal[blockIdx.x]) * a.cells;   // (one value per workgroup: kept scalar)
  __shared__ uint32_t s_xy[WP_MAX + 1], s_d[WP_MAX + 1];       // the window: entry i is p_{a + i}
  __shared__ uint32_t s_recip[WP_MAX + 1];                     // by N
  __shared__ int s_best[2][WP_WAVES];                          // per wave its largest passing candidate (1: the traced step) ...
  __shared__ uint32_t s_cost[2][WP_WAVES];                     // ... and that segment's cost; both by the anchor's parity
  __shared__ int s_hint[2];                                    // the largest candidate any wave has passed so far
  const int g = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = len[g];
  const uint32_t goal = goals[g];
  uint32_t dist = TSD_ROUTE_NONE;
  if (goal < a.cells) {
    const uint32_t k = key[goal];
    if (k != TSD_ROUTE_NONE) dist = k >> 4;
  }
  if (n <= 0 || n > a.max_len) {                     // (the same for every thread) nothing to straighten
    if (t == 0) info[g] = tsd_waypoint_info{n, 0, 0u, dist};
    return;
  }
  const uint32_t* path = paths + (size_t)g * a.max_len;        // p_i = path[n - 1 - i]
  uint32_t* out = way + (size_t)g * a.max_way;
  const int n_max = min(a.lookahead, n - 1);                   // the largest N of any segment (N <= the candidate's distance in path cells)
  for (int N = 1 + t; N <= n_max; N += WP_THREADS) {
    const unsigned long long r = ((1ull << 33) + 2ull * N - 1ull) / (2ull * N);
    s_recip[N] = (uint32_t)min(r, 0xFFFFFFFFull);              // (N = 1 alone gives 2^32; its numerators are 1 and 3, exact with 2^32 - 1)
  }
  if (t == 0) out[0] = path[n - 1];                            // p_0 (max_way >= 1)
  int anchor = 0, n_way = 1;
  uint32_t cost = 0;
  for (int it = 0; anchor < n - 1; it++) {
    const int par = it & 1;
    const int C = min(anchor + a.lookahead, n - 1) - anchor;   // candidates 1 .. C of this window
    for (int i = t; i <= C; i += WP_THREADS) {
      const uint32_t c = path[n - 1 - (anchor + i)];
      s_xy[i] = (c % (uint32_t)a.W) | ((c / (uint32_t)a.W) << 16);
      s_d[i] = key[c] >> 4;
    }
    if (t < WP_WAVES) {
      s_best[par][t] = 1;
      s_cost[par][t] = (key[path[n - 2 - anchor]] >> 4) - (key[path[n - 1 - anchor]] >> 4);
    }
    if (t == 0) s_hint[par] = 1;
    __syncthreads();
    const int ax = (int)(s_xy[0] & 0xFFFFu), ay = (int)(s_xy[0] >> 16);
    const uint32_t da = s_d[0];
    // groups of four candidates, wave w the groups C - 4w, C - 4w - 16, ... downwards
    bool found = false;
    for (int c0 = C - wave * WP_SIDE; c0 >= 2 && !found; c0 -= WP_WAVES * WP_SIDE) {
      if (c0 <= __hip_atomic_load(&s_hint[par], __ATOMIC_RELAXED, WP_WG)) break;
      // the screen: lane (k, s) takes step s + 1 of candidate c0 - k; a group with a refusal is out
      bool bad = false;
      const int mine = c0 - (lane >> 4);
      if (mine >= 2) {
        const WpLine l = wp_line(ax, ay, s_xy[mine], s_recip);
        int cst = 0;
        if ((lane & (WP_SCREEN - 1)) < l.N) bad = wp_step(wimg, a.W, ax, ay, l, (lane & (WP_SCREEN - 1)) + 1, &cst);
      }
      const unsigned long long refused = __ballot(bad);
      for (int k = 0; k < WP_SIDE && !found; k++) {
        const int c = c0 - k;
        if (c < 2) break;
        if ((refused >> (WP_SCREEN * k)) & ((1ull << WP_SCREEN) - 1ull)) continue;
        // the whole segment, the lanes over its steps in chunks of 64
        const WpLine l = wp_line(ax, ay, s_xy[c], s_recip);
        const unsigned long long bound = (unsigned long long)(s_d[c] - da) + a.slack;
        unsigned long long sum = 0;
        bool fail = false;
        for (int s0 = 0; s0 < l.N && !fail; s0 += 64) {
          const int s = s0 + lane + 1;
          bool no = false;
          int cst = 0;
          if (s <= l.N) no = wp_step(wimg, a.W, ax, ay, l, s, &cst);
          sum += (unsigned long long)__shfl(wave_sum_i(cst), 0, 64);
          fail = __ballot(no) != 0ull || sum > bound;
        }
        if (!fail) {
          if (lane == 0) {
            s_best[par][wave] = c;
            s_cost[par][wave] = (uint32_t)sum;
            atomicMax(&s_hint[par], c);
          }
          found = true;
        }
      }
    }
    __syncthreads();
    int best = 0;
    uint32_t seg = 0;
#pragma unroll
    for (int w = 0; w < WP_WAVES; w++)
      if (s_best[par][w] > best) { best = s_best[par][w]; seg = s_cost[par][w]; }
    anchor += best;
    cost += seg;
    if (t == 0 && n_way < a.max_way) out[n_way] = path[n - 1 - anchor];
    n_way++;
  }
  if (t == 0) info[g] = tsd_waypoint_info{n, n_way, cost, dist};
}

static const char* wp_args_wrong(const uint32_t* goal_cells, int n_goals, const tsd_waypoint_params* p, const uint32_t* way, const tsd_waypoint_info* info)
{
  if (!goal_cells) return "goal_cells is NULL";
  if (!p) return "params is NULL";
  if (!way) return "way_host is NULL";
  if (!info) return "info_host is NULL";
  if (n_goals < 1 || n_goals > TSD_ROUTE_MAX_GOALS) return "n_goals is outside 1 .. TSD_ROUTE_MAX_GOALS";
  if (p->lookahead < 1 || p->lookahead > TSD_WAYPOINT_MAX_LOOKAHEAD) return "lookahead is outside 1 .. TSD_WAYPOINT_MAX_LOOKAHEAD";
  if (p->max_len < 1) return "max_len is below 1";
  if (p->max_way < 1) return "max_way is below 1";
  if ((long long)n_goals * p->max_len > (1ll << 24)) return "n_goals * max_len is above 1 << 24";
  if ((long long)n_goals * p->max_way > (1ll << 24)) return "n_goals * max_way is above 1 << 24";
  return nullptr;
}

// The waypoints on instance r of the route result (tsd_ctx::route or ::fields); goal_layers: nullptr for the route entry.
static int route_waypoints(tsd_ctx* ctx, tsd_ctx::Route& r, const char* who, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals,
                           const tsd_waypoint_params* params, uint32_t* way_host, tsd_waypoint_info* info_host)
{
  if (const char* why = wp_args_wrong(goal_cells, n_goals, params, way_host, info_host)) return map_refused(ctx, who, why);
  if (!r.valid) return map_refused(ctx, who, "no route result");
  if (&r == &ctx->fields)
    if (const char* why = route_goal_layers_wrong(r, goal_layers, n_goals)) return map_refused(ctx, who, why);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // d_way / h_way: the records (four words each), then the waypoints
  const size_t ng = (size_t)n_goals, rec_words = ng * (sizeof(tsd_waypoint_info) / sizeof(uint32_t)), words = rec_words + ng * (size_t)params->max_way;
  int rc = scratch_grow(ctx, who, &r.d_way, &r.way_words, words, "the waypoints");
  if (!rc) rc = scratch_grow(ctx, who, &r.h_way, &r.h_way_words, words, "the waypoints' pinned copy", true);
  if (rc == TSD_E_NOMEM) { r.valid = false; r.n_goals = -1; }        // out of memory takes the route result and its goals along, like the trace's
  if (rc) return rc;
  RouteTrace tr{};
  if (int rc2 = route_trace_enqueue(ctx, r, goal_cells, goal_layers, n_goals, params->max_len, &tr)) return rc2;
  tsd_waypoint_info* d_info = reinterpret_cast<tsd_waypoint_info*>(r.d_way);
  uint32_t* d_ways = r.d_way + rec_words;
  const WpArgs a{r.W, (uint32_t)r.W * (uint32_t)r.H, params->lookahead, params->max_len, params->max_way, params->slack};
  {
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? "route_waypoints" : "", true);
    hipLaunchKernelGGL(tr.d_layers ? k_route_waypoints<true> : k_route_waypoints<false>, dim3((unsigned)n_goals), dim3(WP_THREADS), 0, r.stream,
                       r.d_key, r.d_w, a, tr.d_goals, tr.d_layers, tr.d_len, tr.d_paths, d_ways, d_info);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_way, r.d_way, words * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  const tsd_waypoint_info* h_info = reinterpret_cast<const tsd_waypoint_info*>(r.h_way);
  for (size_t g = 0; g < ng; g++) {
    info_host[g] = h_info[g];
    const size_t n = (size_t)std::min(std::max(h_info[g].n_way, 0), params->max_way);
    if (n) std::memcpy(way_host + g * (size_t)params->max_way, r.h_way + rec_words + g * (size_t)params->max_way, n * sizeof(uint32_t));
  }
  return TSD_OK;
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_route_waypoints(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, const tsd_waypoint_params* params, uint32_t* way_host,
                        tsd_waypoint_info* info_host)
{
  if (!ctx) return TSD_E_ARG;
  return route_waypoints(ctx, ctx->route, "tsd_route_waypoints", goal_cells, nullptr, n_goals, params, way_host, info_host);
}

int tsd_route_fields_waypoints(tsd_ctx* ctx, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals, const tsd_waypoint_params* params,
                               uint32_t* way_host, tsd_waypoint_info* info_host)
{
  if (!ctx) return TSD_E_ARG;
  return route_waypoints(ctx, ctx->fields, "tsd_route_fields_waypoints", goal_cells, goal_layers, n_goals, params, way_host, info_host);
}

}  // extern "C"
