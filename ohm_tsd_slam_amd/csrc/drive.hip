// drive.hip -- the velocity of the next step: (speed, turn) samples rolled out as arcs on the weight image of a route result and rated
// on its key image (tsd_drive_rollout, tsd_drive_fields_rollout, tsd_drive_table, tsd_drive_advance and tsd_drive_dev_ptrs of
// include/tsd_hip.h, where the rule is written out).  All in integers.
//
// k_drive_rollout    one wave per sample, four samples per workgroup of 256 threads, grid (ceil(V * Wn / 4), robots): one launch for
//                    all robots.
//   steps      A sample's X_k, Y_k are prefix sums of terms that depend only on (s, t, h0, k), so the 64 lanes take 64 consecutive
//              steps of the sample at once: a table read and a 64-bit product per lane, an in-wave scan (six shuffles per axis), and
//              the carry X, Y, c of the round's last step into the next round of 64.
//   tests      Per lane the byte of the cell entered and, on a diagonal step, the two bytes of the cells it cuts (the cell before
//              comes from the lane below, or from the carry); every address is tested against the map before it is read, a step
//              behind a refused one included.  One ballot gives the first lane refused by reasons 1 .. 3; only the lanes below it
//              walk the body points (a loop per lane, the points in LDS, ended at the first point refused); a second ballot gives
//              the round's first refusal and the sample ends after the round that holds it.  The smallest k wins because a round
//              is only begun when every step before it passed and the ballot's lowest bit is the round's smallest k.
//   rating     The wave sums w over its lanes once, reads the keys at c_T and at the nose, and lane 0 stores the score and `why`
//              and lowers the robot's (score << 16) | index by one 64-bit atomic minimum: the choice is that minimum, whatever the
//              order of the waves.  The admissible count is one atomic add per admissible sample.
//   table      2 * 4096 int32 in device memory behind the context's drive block, read-only: 32 KB that stay in the caches.  A
//              workgroup reads at most 4 * 256 of its entries, so a copy in LDS per workgroup would cost more than it saves.
// k_drive_pick       one wave per robot right behind it on the same stream: it rolls the winner out once more with the same device
//                    function and writes the robot's tsd_drive_choice; no per-sample record has to be kept for it.
// No workgroup waits for another; the two launches are ordered by the stream.
#include "map_product.hpp"

#include <cmath>
#include <cstring>

namespace tsd {

constexpr int DR_H = TSD_DRIVE_HEADINGS, DR_THREADS = 256, DR_WAVES = DR_THREADS / 64;
constexpr unsigned long long DR_NONE = TSD_DRIVE_NONE;

struct DrArgs {
  int W, H;                                          // the key image's sides
  uint32_t cells;                                    // W * H
  int T, V, Wn, B;
  uint32_t a_end, a_nose, a_cost, a_turn;
  int nose;
  uint32_t nose_miss;
};

// what a rollout leaves of one sample; the same in every lane
struct DrSample { uint32_t why, end_cell, d_end, d_nose, cost; unsigned long long score; };

// w of the cell (x, y), 0 outside the map
__device__ __forceinline__ int dr_w(const uint8_t* __restrict__ wimg, int W, int H, int x, int y)
{
  return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? (int)wimg[(uint32_t)y * (uint32_t)W + (uint32_t)x] : 0;
}

__device__ __forceinline__ int dr_q16(long long v) { return (int)((v + 32768) >> 16); }

__device__ __forceinline__ int dr_scan(int v, int lane)       // the inclusive sum over the lanes up to this one
{
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// Sample (s, t) of pose p, by the whole wave.  key: the sample's key image; s_body: the body points (LDS).
__device__ DrSample dr_sample(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, const DrArgs& a,
                              const tsd_drive_pose& p, int s, int t, const int2* s_body, int lane)
{
  int cX = p.fx, cY = p.fy;                          // X, Y and the centre cell of the last step done (step 0: the pose)
  int px = p.x, py = p.y, hT = p.heading;
  int wsum = 0;
  for (int k0 = 0; k0 < a.T; k0 += 64) {
    const int k = k0 + lane + 1;
    const bool act = k <= a.T;
    const int h = (p.heading + k * t) & (DR_H - 1);
    const int2 d = tab[h];
    const int X = cX + dr_scan(act ? dr_q16((long long)s * d.x) : 0, lane);
    const int Y = cY + dr_scan(act ? dr_q16((long long)s * d.y) : 0, lane);
    const int x = p.x + (X >> 16), y = p.y + (Y >> 16);
    int qx = __shfl_up(x, 1, 64), qy = __shfl_up(y, 1, 64);  // c_{k-1}
    if (lane == 0) { qx = px; qy = py; }
    int reason = 0, w = 0;
    if (act) {
      if ((unsigned)x >= (unsigned)a.W || (unsigned)y >= (unsigned)a.H) reason = 1;
      else {
        w = wimg[(uint32_t)y * (uint32_t)a.W + (uint32_t)x];
        if (w == 0) reason = 2;
        else if (x != qx && y != qy && (dr_w(wimg, a.W, a.H, qx, y) == 0 || dr_w(wimg, a.W, a.H, x, qy) == 0)) reason = 3;
      }
    }
    unsigned long long bad = __ballot(reason != 0);
    const int first = bad ? __builtin_ctzll(bad) : 64;
    if (act && lane < first) {                                 // (a lane behind a refused step has nothing to add)
      for (int b = 0; b < a.B; b++) {
        const long long bx = s_body[b].x, by = s_body[b].y;
        const int ux = X + dr_q16(bx * d.x - by * d.y), uy = Y + dr_q16(bx * d.y + by * d.x);
        if (dr_w(wimg, a.W, a.H, p.x + (ux >> 16), p.y + (uy >> 16)) == 0) { reason = 4; break; }
      }
    }
    bad = __ballot(reason != 0);
    if (bad) {
      const int f = __builtin_ctzll(bad);
      return DrSample{((uint32_t)__shfl(reason, f, 64) << 12) | (uint32_t)(k0 + f + 1), TSD_ROUTE_NONE, TSD_ROUTE_NONE, TSD_ROUTE_NONE, 0u, DR_NONE};
    }
    wsum += w;                                                 // (0 in a lane beyond T)
    const int last = min(a.T - k0, 64) - 1;
    cX = __shfl(X, last, 64); cY = __shfl(Y, last, 64);
    px = __shfl(x, last, 64); py = __shfl(y, last, 64); hT = __shfl(h, last, 64);
  }
  // every step passed: c_T = (px, py) lies inside the map
  const uint32_t end = (uint32_t)py * (uint32_t)a.W + (uint32_t)px;
  const uint32_t ke = key[end];
  if (ke == TSD_ROUTE_NONE) return DrSample{(5u << 12) | (uint32_t)a.T, TSD_ROUTE_NONE, TSD_ROUTE_NONE, TSD_ROUTE_NONE, 0u, DR_NONE};
  const uint32_t cost = (uint32_t)__shfl(wave_sum_i(wsum), 0, 64);
  const uint32_t d_end = ke >> 4;
  const int2 d = tab[hT];
  const int nx = p.x + ((cX + dr_q16((long long)a.nose * d.x)) >> 16), ny = p.y + ((cY + dr_q16((long long)a.nose * d.y)) >> 16);
  uint32_t kn = TSD_ROUTE_NONE;
  if ((unsigned)nx < (unsigned)a.W && (unsigned)ny < (unsigned)a.H) kn = key[(uint32_t)ny * (uint32_t)a.W + (uint32_t)nx];
  const uint32_t d_nose = kn != TSD_ROUTE_NONE ? kn >> 4 : d_end + a.nose_miss;
  const unsigned long long score = (unsigned long long)a.a_end * d_end + (unsigned long long)a.a_nose * d_nose +
                                   (unsigned long long)a.a_cost * cost + (unsigned long long)a.a_turn * (uint32_t)abs(t);
  return DrSample{0u, end, d_end, d_nose, cost, score};
}

__global__ void __launch_bounds__(DR_THREADS)
k_drive_rollout(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, DrArgs a,
                const tsd_drive_pose* __restrict__ poses, const int32_t* __restrict__ step, const int32_t* __restrict__ turn,
                const int2* __restrict__ body, unsigned long long* __restrict__ best, uint32_t* __restrict__ count,
                unsigned long long* __restrict__ scores, uint16_t* __restrict__ why)
{
  __shared__ int2 s_body[TSD_DRIVE_MAX_BODY];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  if (tid < a.B) s_body[tid] = body[tid];
  __syncthreads();
  const int r = (int)blockIdx.y, S = a.V * a.Wn;
  const int idx = (int)blockIdx.x * DR_WAVES + __builtin_amdgcn_readfirstlane(tid >> 6);       // (one sample per wave: kept scalar)
  if (idx >= S) return;
  const tsd_drive_pose p = poses[r];
  const int t = turn[idx % a.Wn];
  const DrSample o = dr_sample(key + (size_t)p.layer * a.cells, wimg, tab, a, p, step[idx / a.Wn], t, s_body, lane);
  if (lane == 0) {
    scores[(size_t)r * S + idx] = o.score;
    why[(size_t)r * S + idx] = (uint16_t)o.why;
    if (o.why == 0) {
      atomicMin(&best[r], (o.score << 16) | (unsigned long long)idx);
      atomicAdd(&count[r], 1u);
    }
  }
}

__global__ void __launch_bounds__(64)
k_drive_pick(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, DrArgs a,
             const tsd_drive_pose* __restrict__ poses, const int32_t* __restrict__ step, const int32_t* __restrict__ turn,
             const int2* __restrict__ body, const unsigned long long* __restrict__ best, const uint32_t* __restrict__ count,
             tsd_drive_choice* __restrict__ choice)
{
  __shared__ int2 s_body[TSD_DRIVE_MAX_BODY];
  const int lane = (int)threadIdx.x, r = (int)blockIdx.x;
  if (lane < a.B) s_body[lane] = body[lane];
  __syncthreads();
  const unsigned long long b = best[r];
  if (b == DR_NONE) {                                          // (the same for every lane)
    if (lane == 0) choice[r] = tsd_drive_choice{-1, -1, 0, TSD_ROUTE_NONE, TSD_ROUTE_NONE, TSD_ROUTE_NONE, 0u, 0u, DR_NONE};
    return;
  }
  const int idx = (int)(b & 0xFFFFull), i = idx / a.Wn, j = idx % a.Wn;
  const tsd_drive_pose p = poses[r];
  const DrSample o = dr_sample(key + (size_t)p.layer * a.cells, wimg, tab, a, p, step[i], turn[j], s_body, lane);
  if (lane == 0) choice[r] = tsd_drive_choice{i, j, (int32_t)count[r], o.end_cell, o.d_end, o.d_nose, o.cost, 0u, o.score};
}

// ---- the host's side of the rule
static const int32_t* drive_table()
{
  static int32_t table[2 * DR_H];
  static const bool made = [] {
    const double two_pi = 6.283185307179586476925286766559;
    for (int h = 0; h <= DR_H / 8; h++) {
      table[2 * h] = (int32_t)std::lrint(65536.0 * std::cos(two_pi * h / DR_H));
      table[2 * h + 1] = (int32_t)std::lrint(65536.0 * std::sin(two_pi * h / DR_H));
    }
    for (int h = DR_H / 8 + 1; h <= DR_H / 4; h++) { table[2 * h] = table[2 * (DR_H / 4 - h) + 1]; table[2 * h + 1] = table[2 * (DR_H / 4 - h)]; }
    for (int h = DR_H / 4 + 1; h <= DR_H / 2; h++) { table[2 * h] = -table[2 * (DR_H / 2 - h)]; table[2 * h + 1] = table[2 * (DR_H / 2 - h) + 1]; }
    for (int h = DR_H / 2 + 1; h < DR_H; h++) { table[2 * h] = -table[2 * (h - DR_H / 2)]; table[2 * h + 1] = -table[2 * (h - DR_H / 2) + 1]; }
    return true;
  }();
  (void)made;
  return table;
}

static bool drive_pose_wrong(const tsd_drive_pose& p)
{
  return p.fx < 0 || p.fx > 65535 || p.fy < 0 || p.fy > 65535 || p.heading < 0 || p.heading >= DR_H;
}

static const char* drive_args_wrong(const tsd_ctx::Route& r, bool layered, const tsd_drive_params* p, const tsd_drive_pose* poses, int n_robots,
                                    const tsd_drive_choice* choice)
{
  if (!p) return "params is NULL";
  if (!poses) return "poses is NULL";
  if (!choice) return "choice_host is NULL";
  if (n_robots < 1 || n_robots > TSD_DRIVE_MAX_ROBOTS) return "n_robots is outside 1 .. TSD_DRIVE_MAX_ROBOTS";
  if (p->steps < 1 || p->steps > TSD_DRIVE_MAX_STEPS) return "steps is outside 1 .. TSD_DRIVE_MAX_STEPS";
  if (p->n_speeds < 1 || p->n_speeds > TSD_DRIVE_MAX_SPEEDS) return "n_speeds is outside 1 .. TSD_DRIVE_MAX_SPEEDS";
  if (p->n_turns < 1 || p->n_turns > TSD_DRIVE_MAX_TURNS) return "n_turns is outside 1 .. TSD_DRIVE_MAX_TURNS";
  if (p->n_body < 0 || p->n_body > TSD_DRIVE_MAX_BODY) return "n_body is outside 0 .. TSD_DRIVE_MAX_BODY";
  if (!p->step_q16) return "step_q16 is NULL";
  if (!p->turn) return "turn is NULL";
  if (p->n_body > 0 && !p->body_q16) return "body_q16 is NULL";
  for (int i = 0; i < p->n_speeds; i++)
    if (p->step_q16[i] < 0 || p->step_q16[i] > 65536) return "a step length is outside 0 .. 65536";
  for (int j = 0; j < p->n_turns; j++)
    if (p->turn[j] < -DR_H / 8 || p->turn[j] > DR_H / 8) return "a turn is outside -TSD_DRIVE_HEADINGS / 8 .. TSD_DRIVE_HEADINGS / 8";
  for (int b = 0; b < 2 * p->n_body; b++)
    if (p->body_q16[b] < -64 * 65536 || p->body_q16[b] > 64 * 65536) return "a body coordinate is outside -64 .. 64 cells";
  for (const int32_t c : {p->a_end, p->a_nose, p->a_cost, p->a_turn})
    if (c < 0 || c > 255) return "a coefficient is outside 0 .. 255";
  if (p->nose_q16 < 0 || p->nose_q16 > 64 * 65536) return "nose_q16 is outside 0 .. 64 cells";
  if (p->nose_miss > TSD_ROUTE_MAX_DIST) return "nose_miss is above TSD_ROUTE_MAX_DIST";
  if (!r.valid) return layered ? "no fields result" : "no route result";
  for (int i = 0; i < n_robots; i++) {
    const tsd_drive_pose& q = poses[i];
    if (q.x < 0 || q.x >= r.W || q.y < 0 || q.y >= r.H) return "a pose's cell lies outside the map";
    if (drive_pose_wrong(q)) return "a pose's offset is outside 0 .. 65535 or its heading outside 0 .. TSD_DRIVE_HEADINGS - 1";
    if (layered && (q.layer < 0 || q.layer >= r.layers)) return "a pose's layer is outside 0 .. layers - 1";
  }
  return nullptr;
}

// The rollout on instance r of the route result (tsd_ctx::route or ::fields).
static int drive_rollout(tsd_ctx* ctx, tsd_ctx::Route& r, const char* who, const tsd_drive_params* p, const tsd_drive_pose* poses, int n_robots,
                         tsd_drive_choice* choice_host, uint64_t* scores_host, uint16_t* why_host)
{
  const bool layered = &r == &ctx->fields;
  if (const char* why = drive_args_wrong(r, layered, p, poses, n_robots, choice_host)) return map_refused(ctx, who, why);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // the block in 32-bit words: the table | the inputs: poses, steps, turns, (even) body, (even) best, count | (even) the outputs: choices,
  // scores, why.  The pinned copy holds the inputs and the outputs.
  const size_t R = (size_t)n_robots, S = (size_t)p->n_speeds * p->n_turns, B = (size_t)p->n_body;
  const size_t tab_words = 2 * DR_H;
  const size_t o_pose = 0, o_step = o_pose + 6 * R, o_turn = o_step + p->n_speeds, o_body = (o_turn + p->n_turns + 1) & ~(size_t)1;
  const size_t o_best = (o_body + 2 * B + 1) & ~(size_t)1, o_count = o_best + 2 * R, in_words = (o_count + R + 1) & ~(size_t)1;
  const size_t o_choice = in_words, o_scores = o_choice + R * (sizeof(tsd_drive_choice) / 4), o_why = o_scores + 2 * R * S;
  const size_t words = o_why + (R * S + 1) / 2;
  tsd_ctx::Drive& dr = ctx->drive;
  if (dr.words < tab_words + words) dr.table_ready = false;            // a new block has no table in it, whatever becomes of this call
  int rc = scratch_grow(ctx, who, &dr.d_buf, &dr.words, tab_words + words, "the rollout's samples");
  if (!rc) rc = scratch_grow(ctx, who, &dr.h_buf, &dr.h_words, words, "the rollout's pinned copy", true);
  if (rc) return rc;
  if (!dr.table_ready) {
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(dr.d_buf, drive_table(), tab_words * 4, hipMemcpyHostToDevice, r.stream));
    dr.table_ready = true;                                             // (enqueued on the stream every reader of it follows or waits for)
  }
  uint32_t* h = dr.h_buf;
  std::memcpy(h + o_pose, poses, R * sizeof(tsd_drive_pose));
  if (!layered)
    for (size_t i = 0; i < R; i++) reinterpret_cast<tsd_drive_pose*>(h + o_pose)[i].layer = 0;
  std::memcpy(h + o_step, p->step_q16, (size_t)p->n_speeds * 4);
  std::memcpy(h + o_turn, p->turn, (size_t)p->n_turns * 4);
  if (B) std::memcpy(h + o_body, p->body_q16, 2 * B * 4);
  std::memset(h + o_best, 0xFF, 2 * R * 4);
  std::memset(h + o_count, 0, R * 4);
  uint32_t* d = dr.d_buf + tab_words;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(d, h, in_words * 4, hipMemcpyHostToDevice, r.stream));
  const DrArgs a{r.W, r.H, (uint32_t)r.W * (uint32_t)r.H, p->steps, p->n_speeds, p->n_turns, p->n_body,
                 (uint32_t)p->a_end, (uint32_t)p->a_nose, (uint32_t)p->a_cost, (uint32_t)p->a_turn, p->nose_q16, p->nose_miss};
  const int2* d_tab = reinterpret_cast<const int2*>(dr.d_buf);
  const tsd_drive_pose* d_pose = reinterpret_cast<const tsd_drive_pose*>(d + o_pose);
  const int32_t* d_step = reinterpret_cast<const int32_t*>(d + o_step);
  const int32_t* d_turn = reinterpret_cast<const int32_t*>(d + o_turn);
  const int2* d_body = reinterpret_cast<const int2*>(d + o_body);
  unsigned long long* d_best = reinterpret_cast<unsigned long long*>(d + o_best);
  {
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? "drive_rollout" : "", true);
    hipLaunchKernelGGL(k_drive_rollout, dim3((unsigned)((S + DR_WAVES - 1) / DR_WAVES), (unsigned)n_robots), dim3(DR_THREADS), 0, r.stream, r.d_key, r.d_w,
                       d_tab, a, d_pose, d_step, d_turn, d_body, d_best, d + o_count, reinterpret_cast<unsigned long long*>(d + o_scores),
                       reinterpret_cast<uint16_t*>(d + o_why));
    hipLaunchKernelGGL(k_drive_pick, dim3((unsigned)n_robots), dim3(64), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_pose, d_step, d_turn, d_body, d_best,
                       d + o_count, reinterpret_cast<tsd_drive_choice*>(d + o_choice));
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  const size_t back = (why_host ? words : scores_host ? o_why : o_scores) - o_choice;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(h + o_choice, d + o_choice, back * 4, hipMemcpyDeviceToHost, r.stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  std::memcpy(choice_host, h + o_choice, R * sizeof(tsd_drive_choice));
  if (scores_host) std::memcpy(scores_host, h + o_scores, R * S * sizeof(uint64_t));
  if (why_host) std::memcpy(why_host, h + o_why, R * S * sizeof(uint16_t));
  return TSD_OK;
}

void drive_free(tsd_ctx* ctx)
{
  hipFree(ctx->drive.d_buf);
  if (ctx->drive.h_buf) hipHostFree(ctx->drive.h_buf);
  ctx->drive = tsd_ctx::Drive{};
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_drive_table(int32_t* table)
{
  if (!table) return TSD_E_ARG;
  std::memcpy(table, drive_table(), 2 * DR_H * sizeof(int32_t));
  return TSD_OK;
}

int tsd_drive_advance(const tsd_drive_pose* p, int step_q16, int turn, int n_steps, tsd_drive_pose* out)
{
  if (!p || !out || drive_pose_wrong(*p)) return TSD_E_ARG;
  if (p->x < -(1 << 30) || p->x > (1 << 30) || p->y < -(1 << 30) || p->y > (1 << 30)) return TSD_E_ARG;
  if (step_q16 < 0 || step_q16 > 65536 || turn < -DR_H / 8 || turn > DR_H / 8 || n_steps < 0 || n_steps > TSD_DRIVE_MAX_STEPS) return TSD_E_ARG;
  const int32_t* tab = drive_table();
  long long X = p->fx, Y = p->fy;
  for (int k = 1; k <= n_steps; k++) {
    const int h = (p->heading + k * turn) & (DR_H - 1);
    X += ((long long)step_q16 * tab[2 * h] + 32768) >> 16;
    Y += ((long long)step_q16 * tab[2 * h + 1] + 32768) >> 16;
  }
  const tsd_drive_pose q{p->x + (int32_t)(X >> 16), p->y + (int32_t)(Y >> 16), (int32_t)(X & 65535), (int32_t)(Y & 65535),
                         (p->heading + n_steps * turn) & (DR_H - 1), p->layer};
  *out = q;
  return TSD_OK;
}

int tsd_drive_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_pose* poses, int n_robots, tsd_drive_choice* choice_host,
                      uint64_t* scores_host, uint16_t* why_host)
{
  if (!ctx) return TSD_E_ARG;
  return drive_rollout(ctx, ctx->route, "tsd_drive_rollout", params, poses, n_robots, choice_host, scores_host, why_host);
}

int tsd_drive_fields_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_pose* poses, int n_robots, tsd_drive_choice* choice_host,
                             uint64_t* scores_host, uint16_t* why_host)
{
  if (!ctx) return TSD_E_ARG;
  return drive_rollout(ctx, ctx->fields, "tsd_drive_fields_rollout", params, poses, n_robots, choice_host, scores_host, why_host);
}

int tsd_drive_dev_ptrs(tsd_ctx* ctx, const void** block_dev, unsigned long long* words)
{
  if (!ctx) return TSD_E_ARG;
  if (!ctx->drive.d_buf) return map_refused(ctx, "tsd_drive_dev_ptrs", "no drive call yet");
  if (block_dev) *block_dev = ctx->drive.d_buf;
  if (words) *words = ctx->drive.words;
  return TSD_OK;
}

}  // extern "C"
