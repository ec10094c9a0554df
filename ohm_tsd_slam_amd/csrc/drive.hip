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
// Both kernels come in two instantiations: <false>, the code of a context without a live layer, and <true>, which also refuses a step
// whose centre or body point lies in the layer of tsd_drive_live_set (reason 7; k_live_stamp further down makes the layer).
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

// the live layer of a launch (tsd_drive_live_set): a bit per cell, `stride` words per row
struct DrLive { const uint32_t* words; int stride; };

// the bit of the cell (x, y), which lies inside the map
__device__ __forceinline__ bool dr_live(const DrLive& lv, int x, int y)
{
  return (lv.words[(size_t)(uint32_t)y * (uint32_t)lv.stride + ((uint32_t)x >> 5)] >> (x & 31)) & 1u;
}

// Sample (s, t) of pose p, by the whole wave.  key: the sample's key image; s_body: the body points (LDS).  LIVE: reason 7 behind
// reason 4 -- the centre's bit and, beside each body point's byte, its bit; a launch without a layer takes the instantiation without.
template <bool LIVE>
__device__ DrSample dr_sample(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, const DrArgs& a,
                              const DrLive& lv, const tsd_drive_pose& p, int s, int t, const int2* s_body, int lane)
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
      bool seven = false;
      if constexpr (LIVE) seven = dr_live(lv, x, y);           // (c_k lies inside the map: 1 has passed)
      for (int b = 0; b < a.B; b++) {
        const long long bx = s_body[b].x, by = s_body[b].y;
        const int ux = X + dr_q16(bx * d.x - by * d.y), uy = Y + dr_q16(bx * d.y + by * d.x);
        const int vx = p.x + (ux >> 16), vy = p.y + (uy >> 16);
        if constexpr (LIVE) {                                  // the byte and the bit in flight together, in front of the test
          const bool in = (unsigned)vx < (unsigned)a.W && (unsigned)vy < (unsigned)a.H;
          int wv = 0;
          uint32_t lw = 0u;
          if (in) {
            wv = wimg[(uint32_t)vy * (uint32_t)a.W + (uint32_t)vx];
            lw = lv.words[(size_t)(uint32_t)vy * (uint32_t)lv.stride + ((uint32_t)vx >> 5)];
          }
          asm volatile("" : "+v"(lw));                         // (keeps the word's load in front of the test: it would sink behind the break)
          if (wv == 0) { reason = 4; break; }
          seven |= (lw >> (vx & 31)) & 1u;
        } else {
          if (dr_w(wimg, a.W, a.H, vx, vy) == 0) { reason = 4; break; }
        }
      }
      if constexpr (LIVE)
        if (reason == 0 && seven) reason = 7;                  // 4 goes first at one step, whichever point it is
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

template <bool LIVE>
__global__ void __launch_bounds__(DR_THREADS)
k_drive_rollout(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, DrArgs a,
                const tsd_drive_pose* __restrict__ poses, const int32_t* __restrict__ step, const int32_t* __restrict__ turn,
                const int2* __restrict__ body, unsigned long long* __restrict__ best, uint32_t* __restrict__ count,
                unsigned long long* __restrict__ scores, uint16_t* __restrict__ why, DrLive lv)
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
  const DrSample o = dr_sample<LIVE>(key + (size_t)p.layer * a.cells, wimg, tab, a, lv, p, step[idx / a.Wn], t, s_body, lane);
  if (lane == 0) {
    scores[(size_t)r * S + idx] = o.score;
    why[(size_t)r * S + idx] = (uint16_t)o.why;
    if (o.why == 0) {
      atomicMin(&best[r], (o.score << 16) | (unsigned long long)idx);
      atomicAdd(&count[r], 1u);
    }
  }
}

template <bool LIVE>
__global__ void __launch_bounds__(64)
k_drive_pick(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, DrArgs a,
             const tsd_drive_pose* __restrict__ poses, const int32_t* __restrict__ step, const int32_t* __restrict__ turn,
             const int2* __restrict__ body, const unsigned long long* __restrict__ best, const uint32_t* __restrict__ count,
             tsd_drive_choice* __restrict__ choice, DrLive lv)
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
  const DrSample o = dr_sample<LIVE>(key + (size_t)p.layer * a.cells, wimg, tab, a, lv, p, step[i], turn[j], s_body, lane);
  if (lane == 0) choice[r] = tsd_drive_choice{i, j, (int32_t)count[r], o.end_cell, o.d_end, o.d_nose, o.cost, 0u, o.score};
}

// ---- the fleet form (tsd_drive_fleet_rollout): the ranks decide one after the other, ordered by kernel boundaries on one stream
// k_drive_rollout    as above for the robots that are not parked (a compact pose list), into the block's map rows: every sample's
//                    score and `why` by reasons 1 .. 5.  Its minimum and count go to words nobody reads.
// k_fleet_init       one workgroup per robot: the robot's pose into every slot of its track; a parked robot's scores, `why` and choice.
// k_fleet_sample     per rank: one wave per sample, the lanes over 64 consecutive steps as in dr_sample, but on the trajectory alone --
//                    the table read, the product and the scan; no map byte.  It runs the steps before the map's first refusal (all T
//                    for an admissible sample and for reason 5): per lane P(k) and P(k-1) (the lane below, or the carry) against
//                    the tracks of the robots decided so far, which are read from the block (at most 16 x 257 x 16 bytes, read-only
//                    in this launch and coalesced over the lanes: they stay in the caches, and a copy in LDS per workgroup of four
//                    samples would read as much and add a barrier).  One ballot gives the round's first conflict.  Lane 0 stores the
//                    final score and `why` and lowers the robot's minimum as k_drive_rollout does.
// k_fleet_pick       per rank, one wave: the winner's record and its track over the pose's -- the trajectory, w at the centre cells and
//                    the two keys; the winner is admissible, so no test is repeated and no body point walked.
// `decided` is a bit per robot and a kernel argument, so a launch reads only tracks that launches before it have finished.
constexpr long long DR_FAR = 1ll << 62;

struct DrFleet { int R, sep; unsigned decided; };

// D of the rule: far unless both differences are below sep in magnitude (so the products stay below 2^47)
__device__ __forceinline__ long long dr_dist(long long ax, long long ay, longlong2 b, long long sep)
{
  const long long dx = ax - b.x, dy = ay - b.y;
  return (dx > -sep && dx < sep && dy > -sep && dy < sep) ? dx * dx + dy * dy : DR_FAR;
}

// X_k, Y_k of the round's steps k = k0 + lane + 1 <= T (the carry cX, cY in a lane beyond T)
__device__ __forceinline__ int2 dr_round(const int2* __restrict__ tab, const tsd_drive_pose& p, int s, int t, int T, int k0, int cX, int cY, int lane)
{
  const int k = k0 + lane + 1;
  const bool act = k <= T;
  const int2 d = tab[(p.heading + k * t) & (DR_H - 1)];
  return make_int2(cX + dr_scan(act ? dr_q16((long long)s * d.x) : 0, lane), cY + dr_scan(act ? dr_q16((long long)s * d.y) : 0, lane));
}

__global__ void __launch_bounds__(DR_THREADS)
k_fleet_init(DrArgs a, const tsd_drive_pose* __restrict__ poses, longlong2* __restrict__ tracks, unsigned long long* __restrict__ scores,
             uint16_t* __restrict__ why, tsd_drive_choice* __restrict__ choice)
{
  const int r = (int)blockIdx.x, tid = (int)threadIdx.x, S = a.V * a.Wn;
  const tsd_drive_pose p = poses[r];
  const longlong2 at = make_longlong2(((long long)p.x << 16) + p.fx, ((long long)p.y << 16) + p.fy);
  for (int k = tid; k <= a.T; k += DR_THREADS) tracks[(size_t)r * (a.T + 1) + k] = at;
  if (p.layer >= 0) return;
  for (int i = tid; i < S; i += DR_THREADS) { scores[(size_t)r * S + i] = DR_NONE; why[(size_t)r * S + i] = 0; }
  if (tid == 0) choice[r] = tsd_drive_choice{-1, -1, 0, TSD_ROUTE_NONE, TSD_ROUTE_NONE, TSD_ROUTE_NONE, 0u, 0u, DR_NONE};
}

// Robot r (row c of the map pass) against the tracks of the robots in f.decided.
__global__ void __launch_bounds__(DR_THREADS)
k_fleet_sample(const int2* __restrict__ tab, DrArgs a, DrFleet f, int r, int c, const tsd_drive_pose* __restrict__ poses,
               const int32_t* __restrict__ step, const int32_t* __restrict__ turn, const longlong2* __restrict__ tracks,
               const unsigned long long* __restrict__ map_scores, const uint16_t* __restrict__ map_why, unsigned long long* __restrict__ best,
               uint32_t* __restrict__ count, unsigned long long* __restrict__ scores, uint16_t* __restrict__ why)
{
  const int tid = (int)threadIdx.x, lane = tid & 63, S = a.V * a.Wn;
  const int idx = (int)blockIdx.x * DR_WAVES + __builtin_amdgcn_readfirstlane(tid >> 6);
  if (idx >= S) return;
  uint32_t w = map_why[(size_t)c * S + idx];
  unsigned long long score = map_scores[(size_t)c * S + idx];
  const uint32_t reason = w >> 12;
  // at the map's own step the map's reason goes first: 1 .. 4, and 7 where the map pass ran with a live layer
  const int last = ((reason >= 1 && reason <= 4) || reason == 7) ? min((int)(w & 0xFFFu) - 1, a.T) : a.T;
  if (f.decided != 0 && f.sep > 0) {
    const tsd_drive_pose p = poses[r];
    const int s = step[idx / a.Wn], t = turn[idx % a.Wn];
    const long long bx = (long long)p.x << 16, by = (long long)p.y << 16, sep = f.sep, sep2 = sep * sep;
    int cX = p.fx, cY = p.fy;
    for (int k0 = 0; k0 < last; k0 += 64) {
      const int k = k0 + lane + 1;
      const int2 xy = dr_round(tab, p, s, t, last, k0, cX, cY, lane);
      int qX = __shfl_up(xy.x, 1, 64), qY = __shfl_up(xy.y, 1, 64);                   // X_{k-1}, Y_{k-1}
      if (lane == 0) { qX = cX; qY = cY; }
      bool hit = false;
      if (k <= last) {                                                                // (k <= T: slots k - 1 and k of a track exist)
        for (unsigned m = f.decided & ((1u << f.R) - 1u); m != 0; m &= m - 1) {
          const longlong2* tr = tracks + (size_t)__builtin_ctz(m) * (a.T + 1);
          const long long dk = dr_dist(bx + xy.x, by + xy.y, tr[k], sep);
          hit |= dk < sep2 && dk <= dr_dist(bx + qX, by + qY, tr[k - 1], sep);        // (far is above sep^2)
        }
      }
      const unsigned long long bad = __ballot(hit);
      if (bad) { w = (6u << 12) | (uint32_t)(k0 + __builtin_ctzll(bad) + 1); score = DR_NONE; break; }
      const int e = min(last - k0, 64) - 1;
      cX = __shfl(xy.x, e, 64); cY = __shfl(xy.y, e, 64);
    }
  }
  if (lane == 0) {
    scores[(size_t)r * S + idx] = score;
    why[(size_t)r * S + idx] = (uint16_t)w;
    if (w == 0) {
      atomicMin(&best[r], (score << 16) | (unsigned long long)idx);
      atomicAdd(&count[r], 1u);
    }
  }
}

// The winner of robot r: its record and its track.  The winner is admissible -- every step has passed every test in the map pass --
// so nothing is tested again: the trajectory, w at the centre cells for the cost, the two keys.  (k_drive_pick's re-roll with dr_sample
// walks the body points once more, a serial loop per lane; 16 of those one after the other were most of the chain's time at the limits.)
__global__ void __launch_bounds__(64)
k_fleet_pick(const uint32_t* __restrict__ key, const uint8_t* __restrict__ wimg, const int2* __restrict__ tab, DrArgs a, int r,
             const tsd_drive_pose* __restrict__ poses, const int32_t* __restrict__ step, const int32_t* __restrict__ turn,
             const unsigned long long* __restrict__ best, const uint32_t* __restrict__ count, tsd_drive_choice* __restrict__ choice,
             longlong2* __restrict__ tracks)
{
  const int lane = (int)threadIdx.x;
  const unsigned long long b = best[r];
  const int idx = (int)(b & 0xFFFFull);
  if (b == DR_NONE || idx >= a.V * a.Wn) {                     // (the same for every lane; the track stays the pose's)
    if (lane == 0) choice[r] = tsd_drive_choice{-1, -1, 0, TSD_ROUTE_NONE, TSD_ROUTE_NONE, TSD_ROUTE_NONE, 0u, 0u, DR_NONE};
    return;
  }
  const int i = idx / a.Wn, j = idx % a.Wn;
  const tsd_drive_pose p = poses[r];
  const int s = step[i], t = turn[j];
  int cX = p.fx, cY = p.fy, wsum = 0;
  for (int k0 = 0; k0 < a.T; k0 += 64) {
    const int k = k0 + lane + 1;
    const int2 xy = dr_round(tab, p, s, t, a.T, k0, cX, cY, lane);
    if (k <= a.T) {
      tracks[(size_t)r * (a.T + 1) + k] = make_longlong2(((long long)p.x << 16) + xy.x, ((long long)p.y << 16) + xy.y);
      wsum += dr_w(wimg, a.W, a.H, p.x + (xy.x >> 16), p.y + (xy.y >> 16));
    }
    const int e = min(a.T - k0, 64) - 1;
    cX = __shfl(xy.x, e, 64); cY = __shfl(xy.y, e, 64);
  }
  const uint32_t cost = (uint32_t)__shfl(wave_sum_i(wsum), 0, 64);
  if (lane != 0) return;
  // From here on this restates the end of dr_sample -- c_T's key, the nose cell, the d_nose fallback, the score -- and must change with
  // it: dr_sample itself is left as it is so that the two older entries keep their code; tests/test_gpu_drive_fleet.py holds the two
  // copies together byte for byte (sep 0 against tsd_drive_fields_rollout's choices).
  const uint32_t* lkey = key + (size_t)p.layer * a.cells;
  const int ex = p.x + (cX >> 16), ey = p.y + (cY >> 16);      // c_T: inside the map and with a key, or the sample were not admissible
  const uint32_t end = (uint32_t)ey * (uint32_t)a.W + (uint32_t)ex;
  const uint32_t ke = ((unsigned)ex < (unsigned)a.W && (unsigned)ey < (unsigned)a.H) ? lkey[end] : TSD_ROUTE_NONE;
  const uint32_t d_end = ke >> 4;
  const int2 d = tab[(p.heading + a.T * t) & (DR_H - 1)];
  const int nx = p.x + ((cX + dr_q16((long long)a.nose * d.x)) >> 16), ny = p.y + ((cY + dr_q16((long long)a.nose * d.y)) >> 16);
  uint32_t kn = TSD_ROUTE_NONE;
  if ((unsigned)nx < (unsigned)a.W && (unsigned)ny < (unsigned)a.H) kn = lkey[(uint32_t)ny * (uint32_t)a.W + (uint32_t)nx];
  const uint32_t d_nose = kn != TSD_ROUTE_NONE ? kn >> 4 : d_end + a.nose_miss;
  const unsigned long long score = (unsigned long long)a.a_end * d_end + (unsigned long long)a.a_nose * d_nose +
                                   (unsigned long long)a.a_cost * cost + (unsigned long long)a.a_turn * (uint32_t)abs(t);
  choice[r] = tsd_drive_choice{i, j, (int32_t)count[r], end, d_end, d_nose, cost, 0u, score};
}

// The key under each robot's pose on its own layer (tsd_drive_fields_togo): one thread per robot; a parked robot has none.
__global__ void __launch_bounds__(64)
k_drive_togo(const uint32_t* __restrict__ key, int W, int H, uint32_t cells, int layers, int R, const tsd_drive_pose* __restrict__ poses,
             uint32_t* __restrict__ togo)
{
  const int r = (int)threadIdx.x;
  if (r >= R) return;
  const tsd_drive_pose p = poses[r];
  const bool in = (unsigned)p.x < (unsigned)W && (unsigned)p.y < (unsigned)H && (unsigned)p.layer < (unsigned)layers;
  togo[r] = in ? key[(size_t)p.layer * cells + (uint32_t)p.y * (uint32_t)W + (uint32_t)p.x] : TSD_ROUTE_NONE;
}

// ---- the live layer (tsd_drive_live_set): the discs of a scan's end points as bits
// k_live_stamp       one thread per (point, row of its disc), 256 per workgroup, the row the fast index: a wave holds the rows of one or
//                    a few discs whatever the radius (at r = 8 a wave per point would leave 47 of 64 lanes idle, and a thread per point
//                    would walk up to 129 rows one after the other).  The skip discs and the half-width table come into LDS once per
//                    workgroup; each thread tests its point against the discs, takes the row's half-width from the table (built by
//                    the host in integers), clips the span to the map and ORs its word masks into the image -- at most five words at
//                    r = 64.  Every word address is bounded by y < H and x1 <= W - 1, so x1 >> 5 < stride.  The thread of a point's
//                    first row counts the point as kept: one atomic add per wave.
// The old layer is emptied by a memset of the bit image.  (A pass over the previous set's points that zeroes the words they wrote was
// built and measured beside it -- profiles/drive_live.txt: 3 us cheaper on a 32 MB image for one scan's points, up to 80 us dearer at
// 32 768 points -- and taken out again.)
// The points' block, in int32 words: the discs (3 * 16), the table (65), the kept count, padding up to 128, then the points.
constexpr int LV_THREADS = 256, LV_DISC = 0, LV_TABLE = 3 * TSD_DRIVE_LIVE_MAX_SKIP, LV_KEPT = LV_TABLE + TSD_DRIVE_LIVE_MAX_RADIUS + 1, LV_POINTS = 128;
constexpr size_t LV_BLOCK = LV_POINTS + 2 * (size_t)TSD_DRIVE_LIVE_MAX_POINTS;
static_assert(LV_KEPT < LV_POINTS, "the head of the block holds the discs, the table and the count");

struct LvArgs { int W, H, stride, r, n, n_skip; };

__global__ void __launch_bounds__(LV_THREADS)
k_live_stamp(int32_t* __restrict__ block, LvArgs a, uint32_t* __restrict__ words)
{
  __shared__ int s_disc[3 * TSD_DRIVE_LIVE_MAX_SKIP];
  __shared__ int s_hw[TSD_DRIVE_LIVE_MAX_RADIUS + 1];
  const int tid = (int)threadIdx.x;
  if (tid < 3 * a.n_skip) s_disc[tid] = block[LV_DISC + tid];
  if (tid <= a.r) s_hw[tid] = block[LV_TABLE + tid];
  __syncthreads();
  const int rows = 2 * a.r + 1;
  const int id = (int)blockIdx.x * LV_THREADS + tid;           // (at most 32 768 * 129 + 255)
  const int i = id / rows, row = id - i * rows;
  bool keep = i < a.n;
  int px = 0, py = 0;
  if (keep) {
    px = block[LV_POINTS + 2 * i]; py = block[LV_POINTS + 2 * i + 1];
    for (int q = 0; q < a.n_skip; q++) {
      const long long dx = (long long)px - s_disc[3 * q], dy = (long long)py - s_disc[3 * q + 1], ro = s_disc[3 * q + 2];
      if (dx >= -ro && dx <= ro && dy >= -ro && dy <= ro && dx * dx + dy * dy <= ro * ro) keep = false;
    }
  }
  const unsigned long long first_rows = __ballot(keep && row == 0);
  if ((tid & 63) == 0 && first_rows) atomicAdd(reinterpret_cast<unsigned*>(block + LV_KEPT), (unsigned)__popcll(first_rows));
  if (!keep) return;
  const int dy = row - a.r, y = py + dy;
  if ((unsigned)y >= (unsigned)a.H) return;
  const int hw = s_hw[dy < 0 ? -dy : dy];
  const int x0 = max(px - hw, 0), x1 = min(px + hw, a.W - 1);
  if (x0 > x1) return;
  uint32_t* line = words + (size_t)y * (size_t)a.stride;
  for (int w = x0 >> 5; w <= (x1 >> 5); w++) {                 // (x1 < W: w < stride)
    const int lo = max(x0, w << 5), hi = min(x1, (w << 5) + 31);
    atomicOr(&line[w], (0xFFFFFFFFu >> (31 - (hi - lo))) << (lo & 31));
  }
}

static const char* live_args_wrong(const tsd_drive_live_params* p, const int32_t* pts, int n, int width, int height)
{
  if (!p) return "params is NULL";
  if (p->radius < 0 || p->radius > TSD_DRIVE_LIVE_MAX_RADIUS) return "radius is outside 0 .. TSD_DRIVE_LIVE_MAX_RADIUS";
  if (p->n_skip < 0 || p->n_skip > TSD_DRIVE_LIVE_MAX_SKIP) return "n_skip is outside 0 .. TSD_DRIVE_LIVE_MAX_SKIP";
  if (p->n_skip > 0 && !p->skip) return "skip is NULL";
  if (n < 0 || n > TSD_DRIVE_LIVE_MAX_POINTS) return "n is outside 0 .. TSD_DRIVE_LIVE_MAX_POINTS";
  if (n > 0 && !pts) return "points_xy is NULL";
  if (width < 1 || height < 1 || width > TSD_FRONTIER_MAX_SIDE || height > TSD_FRONTIER_MAX_SIDE) return "a side outside 1 .. TSD_FRONTIER_MAX_SIDE";
  constexpr int32_t far = 1 << 30;
  for (int q = 0; q < p->n_skip; q++) {
    if (p->skip[3 * q] < -far || p->skip[3 * q] > far || p->skip[3 * q + 1] < -far || p->skip[3 * q + 1] > far) return "a skip disc's centre is beyond 1 << 30";
    if (p->skip[3 * q + 2] < 0 || p->skip[3 * q + 2] > (1 << 15)) return "a skip disc's radius is outside 0 .. 1 << 15";
  }
  for (int i = 0; i < 2 * n; i++)
    if (pts[i] < -far || pts[i] > far) return "a point's coordinate is beyond 1 << 30";
  return nullptr;
}

static int drive_live_set(tsd_ctx* ctx, const tsd_drive_live_params* p, const int32_t* pts, int n, int width, int height, int* n_kept)
{
  const char* who = "tsd_drive_live_set";
  if (const char* why = live_args_wrong(p, pts, n, width, height)) return map_refused(ctx, who, why);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  tsd_ctx::Drive::Live& l = ctx->drive.live;
  const int stride = (width + 31) / 32;
  const size_t words = (size_t)stride * (size_t)height;
  if (l.words < words) l.set = false;                                  // a new image holds nothing, whatever becomes of this call
  int rc = scratch_grow(ctx, who, &l.d_words, &l.words, words, "the live layer");
  if (!rc) rc = scratch_grow(ctx, who, &l.d_pts, &l.pts_words, LV_BLOCK, "the live layer's points");
  if (!rc) rc = scratch_grow(ctx, who, &l.h_pts, &l.h_pts_words, LV_BLOCK, "the live layer's points, pinned", true);
  if (rc) { l.set = false; return rc; }
  hipStream_t stream = ctx->stream;
  int32_t* d_new = l.d_pts;
  l.set = false;                                                       // until the new one stands
  int32_t* h = l.h_pts;
  std::memset(h, 0, LV_POINTS * sizeof(int32_t));
  if (p->n_skip) std::memcpy(h + LV_DISC, p->skip, 3 * (size_t)p->n_skip * sizeof(int32_t));
  for (int d = 0, hw = p->radius; d <= p->radius; d++) {               // floor(sqrt(r^2 - d^2)): it falls as d grows
    while (hw * hw > p->radius * p->radius - d * d) hw--;
    h[LV_TABLE + d] = hw;
  }
  if (n) std::memcpy(h + LV_POINTS, pts, 2 * (size_t)n * sizeof(int32_t));
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(d_new, h, (LV_POINTS + 2 * (size_t)n) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  {
    ScopedKernelTimer t(ctx, "drive_live", true);
    TSD_HIP_CHECK(ctx, hipMemsetAsync(l.d_words, 0, words * sizeof(uint32_t), stream));
    const long long threads = (long long)n * (2 * p->radius + 1);
    if (threads > 0)
      hipLaunchKernelGGL(k_live_stamp, dim3((unsigned)((threads + LV_THREADS - 1) / LV_THREADS)), dim3(LV_THREADS), 0, stream, d_new,
                         LvArgs{width, height, stride, p->radius, n, p->n_skip}, l.d_words);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(h + LV_KEPT, d_new + LV_KEPT, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(stream));
  l.set = true; l.W = width; l.H = height; l.stride = stride;
  if (n_kept) *n_kept = h[LV_KEPT];
  return TSD_OK;
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
                                    const tsd_drive_choice* choice, bool parked_ok = false)
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
    if (layered && (q.layer < (parked_ok ? -1 : 0) || q.layer >= r.layers))
      return parked_ok ? "a pose's layer is outside -1 .. layers - 1" : "a pose's layer is outside 0 .. layers - 1";
  }
  return nullptr;
}

// a layer that is set has the sides of the result's image
static const char* drive_live_wrong(const tsd_ctx* ctx, const tsd_ctx::Route& r)
{
  const tsd_ctx::Drive::Live& l = ctx->drive.live;
  return l.set && (l.W != r.W || l.H != r.H) ? "the live layer's width or height differ from the result's image" : nullptr;
}

// The rollout on instance r of the route result (tsd_ctx::route or ::fields).
static int drive_rollout(tsd_ctx* ctx, tsd_ctx::Route& r, const char* who, const tsd_drive_params* p, const tsd_drive_pose* poses, int n_robots,
                         tsd_drive_choice* choice_host, uint64_t* scores_host, uint16_t* why_host)
{
  const bool layered = &r == &ctx->fields;
  if (const char* why = drive_args_wrong(r, layered, p, poses, n_robots, choice_host)) return map_refused(ctx, who, why);
  if (const char* why = drive_live_wrong(ctx, r)) return map_refused(ctx, who, why);
  const DrLive lv{ctx->drive.live.d_words, ctx->drive.live.stride};
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
    const dim3 groups((unsigned)((S + DR_WAVES - 1) / DR_WAVES), (unsigned)n_robots);
    unsigned long long* d_scores = reinterpret_cast<unsigned long long*>(d + o_scores);
    uint16_t* d_why = reinterpret_cast<uint16_t*>(d + o_why);
    tsd_drive_choice* d_choice = reinterpret_cast<tsd_drive_choice*>(d + o_choice);
    if (dr.live.set) {
      hipLaunchKernelGGL(k_drive_rollout<true>, groups, dim3(DR_THREADS), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_pose, d_step, d_turn, d_body, d_best,
                         d + o_count, d_scores, d_why, lv);
      hipLaunchKernelGGL(k_drive_pick<true>, dim3((unsigned)n_robots), dim3(64), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_pose, d_step, d_turn, d_body,
                         d_best, d + o_count, d_choice, lv);
    } else {
      hipLaunchKernelGGL(k_drive_rollout<false>, groups, dim3(DR_THREADS), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_pose, d_step, d_turn, d_body, d_best,
                         d + o_count, d_scores, d_why, lv);
      hipLaunchKernelGGL(k_drive_pick<false>, dim3((unsigned)n_robots), dim3(64), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_pose, d_step, d_turn, d_body,
                         d_best, d + o_count, d_choice, lv);
    }
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

// The fleet form on the fields result: the map pass for the robots that are not parked, then a launch pair per rank.
static int drive_fleet_rollout(tsd_ctx* ctx, const tsd_drive_params* p, const tsd_drive_fleet_params* fl, const tsd_drive_pose* poses, int n_robots,
                               tsd_drive_choice* choice_host, uint64_t* scores_host, uint16_t* why_host, int64_t* tracks_host)
{
  const char* who = "tsd_drive_fleet_rollout";
  tsd_ctx::Route& r = ctx->fields;
  if (const char* why = drive_args_wrong(r, true, p, poses, n_robots, choice_host, true)) return map_refused(ctx, who, why);
  if (!fl) return map_refused(ctx, who, "fleet is NULL");
  if (!fl->order) return map_refused(ctx, who, "order is NULL");
  if (fl->sep_q16 < 0 || fl->sep_q16 > TSD_DRIVE_MAX_SEP) return map_refused(ctx, who, "sep_q16 is outside 0 .. TSD_DRIVE_MAX_SEP");
  if (const char* why = drive_live_wrong(ctx, r)) return map_refused(ctx, who, why);
  const DrLive lv{ctx->drive.live.d_words, ctx->drive.live.stride};
  unsigned seen = 0;
  for (int m = 0; m < n_robots; m++) {
    const int32_t q = fl->order[m];
    if (q < 0 || q >= n_robots || ((seen >> q) & 1u)) return map_refused(ctx, who, "order is no permutation of 0 .. n_robots - 1");
    seen |= 1u << q;
  }
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // the block as drive_rollout's, with the compact poses of the robots that are not parked among the inputs, the tracks among the
  // outputs, and behind the outputs what only the device reads: the map pass's scores and `why` per compact row, and the words its
  // minimum and count go to
  const size_t R = (size_t)n_robots, S = (size_t)p->n_speeds * p->n_turns, B = (size_t)p->n_body, T1 = (size_t)p->steps + 1;
  const size_t tab_words = 2 * DR_H;
  const size_t o_pose = 0, o_apose = o_pose + 6 * R, o_step = o_apose + 6 * R, o_turn = o_step + p->n_speeds;
  const size_t o_body = (o_turn + p->n_turns + 1) & ~(size_t)1, o_best = (o_body + 2 * B + 1) & ~(size_t)1, o_count = o_best + 2 * R;
  const size_t in_words = (o_count + R + 3) & ~(size_t)3;
  const size_t o_choice = in_words, o_tracks = (o_choice + R * (sizeof(tsd_drive_choice) / 4) + 3) & ~(size_t)3;       // (16 bytes per slot)
  const size_t o_scores = o_tracks + 4 * R * T1, o_why = o_scores + 2 * R * S, io_words = (o_why + (R * S + 1) / 2 + 1) & ~(size_t)1;
  const size_t o_mscores = io_words, o_mwhy = o_mscores + 2 * R * S, o_mbest = (o_mwhy + (R * S + 1) / 2 + 1) & ~(size_t)1;
  const size_t words = o_mbest + 2 * R + R;
  tsd_ctx::Drive& dr = ctx->drive;
  if (dr.words < tab_words + words) dr.table_ready = false;
  int rc = scratch_grow(ctx, who, &dr.d_buf, &dr.words, tab_words + words, "the fleet rollout's samples");
  if (!rc) rc = scratch_grow(ctx, who, &dr.h_buf, &dr.h_words, io_words, "the fleet rollout's pinned copy", true);
  if (rc) return rc;
  if (!dr.table_ready) {
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(dr.d_buf, drive_table(), tab_words * 4, hipMemcpyHostToDevice, r.stream));
    dr.table_ready = true;
  }
  uint32_t* h = dr.h_buf;
  std::memcpy(h + o_pose, poses, R * sizeof(tsd_drive_pose));
  int row[TSD_DRIVE_MAX_ROBOTS], A = 0;                                // a robot's row in the map pass, -1: parked
  unsigned parked = 0;
  for (size_t i = 0; i < R; i++) {
    if (poses[i].layer < 0) { row[i] = -1; parked |= 1u << i; continue; }
    std::memcpy(h + o_apose + 6 * (size_t)A, poses + i, sizeof(tsd_drive_pose));
    row[i] = A++;
  }
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
  unsigned long long* d_scores = reinterpret_cast<unsigned long long*>(d + o_scores);
  unsigned long long* d_mscores = reinterpret_cast<unsigned long long*>(d + o_mscores);
  uint16_t* d_why = reinterpret_cast<uint16_t*>(d + o_why);
  uint16_t* d_mwhy = reinterpret_cast<uint16_t*>(d + o_mwhy);
  tsd_drive_choice* d_choice = reinterpret_cast<tsd_drive_choice*>(d + o_choice);
  longlong2* d_tracks = reinterpret_cast<longlong2*>(d + o_tracks);
  const unsigned groups = (unsigned)((S + DR_WAVES - 1) / DR_WAVES);
  {
    ScopedKernelTimer t(ctx, r.stream == ctx->stream ? "drive_fleet" : "", true);
    hipLaunchKernelGGL(k_fleet_init, dim3((unsigned)n_robots), dim3(DR_THREADS), 0, r.stream, a, d_pose, d_tracks, d_scores, d_why, d_choice);
    if (A > 0) {                                                       // the map rows carry reason 7: the rank launches need nothing
      const tsd_drive_pose* d_apose = reinterpret_cast<const tsd_drive_pose*>(d + o_apose);
      unsigned long long* d_mbest = reinterpret_cast<unsigned long long*>(d + o_mbest);
      if (dr.live.set)
        hipLaunchKernelGGL(k_drive_rollout<true>, dim3(groups, (unsigned)A), dim3(DR_THREADS), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_apose, d_step,
                           d_turn, d_body, d_mbest, d + o_mbest + 2 * R, d_mscores, d_mwhy, lv);
      else
        hipLaunchKernelGGL(k_drive_rollout<false>, dim3(groups, (unsigned)A), dim3(DR_THREADS), 0, r.stream, r.d_key, r.d_w, d_tab, a, d_apose, d_step,
                           d_turn, d_body, d_mbest, d + o_mbest + 2 * R, d_mscores, d_mwhy, lv);
    }
    DrFleet f{n_robots, fl->sep_q16, parked};
    for (int m = 0; m < n_robots; m++) {
      const int q = fl->order[m];
      if (row[q] < 0) continue;
      hipLaunchKernelGGL(k_fleet_sample, dim3(groups), dim3(DR_THREADS), 0, r.stream, d_tab, a, f, q, row[q], d_pose, d_step, d_turn, d_tracks,
                         d_mscores, d_mwhy, d_best, d + o_count, d_scores, d_why);
      hipLaunchKernelGGL(k_fleet_pick, dim3(1), dim3(64), 0, r.stream, r.d_key, r.d_w, d_tab, a, q, d_pose, d_step, d_turn, d_best, d + o_count,
                         d_choice, d_tracks);
      f.decided |= 1u << q;
    }
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  const size_t back = (why_host ? io_words : scores_host ? o_why : tracks_host ? o_scores : o_tracks) - o_choice;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(h + o_choice, d + o_choice, back * 4, hipMemcpyDeviceToHost, r.stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  std::memcpy(choice_host, h + o_choice, R * sizeof(tsd_drive_choice));
  if (tracks_host) std::memcpy(tracks_host, h + o_tracks, R * T1 * 2 * sizeof(int64_t));
  if (scores_host) std::memcpy(scores_host, h + o_scores, R * S * sizeof(uint64_t));
  if (why_host) std::memcpy(why_host, h + o_why, R * S * sizeof(uint16_t));
  return TSD_OK;
}

// The keys under the poses, fetched in one round trip.
static int drive_fields_togo(tsd_ctx* ctx, const tsd_drive_pose* poses, int n_robots, uint32_t* togo_host)
{
  const char* who = "tsd_drive_fields_togo";
  tsd_ctx::Route& r = ctx->fields;
  if (!poses) return map_refused(ctx, who, "poses is NULL");
  if (!togo_host) return map_refused(ctx, who, "togo_host is NULL");
  if (n_robots < 1 || n_robots > TSD_DRIVE_MAX_ROBOTS) return map_refused(ctx, who, "n_robots is outside 1 .. TSD_DRIVE_MAX_ROBOTS");
  if (!r.valid) return map_refused(ctx, who, "no fields result");
  for (int i = 0; i < n_robots; i++) {
    if (poses[i].x < 0 || poses[i].x >= r.W || poses[i].y < 0 || poses[i].y >= r.H) return map_refused(ctx, who, "a pose's cell lies outside the map");
    if (poses[i].layer < -1 || poses[i].layer >= r.layers) return map_refused(ctx, who, "a pose's layer is outside -1 .. layers - 1");
  }
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t R = (size_t)n_robots, tab_words = 2 * DR_H, words = 7 * R;        // the poses | the keys
  tsd_ctx::Drive& dr = ctx->drive;
  if (dr.words < tab_words + words) dr.table_ready = false;
  int rc = scratch_grow(ctx, who, &dr.d_buf, &dr.words, tab_words + words, "the poses' keys");
  if (!rc) rc = scratch_grow(ctx, who, &dr.h_buf, &dr.h_words, words, "the poses' keys, pinned", true);
  if (rc) return rc;
  uint32_t* h = dr.h_buf;
  uint32_t* d = dr.d_buf + tab_words;
  std::memcpy(h, poses, R * sizeof(tsd_drive_pose));
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(d, h, 6 * R * 4, hipMemcpyHostToDevice, r.stream));
  hipLaunchKernelGGL(k_drive_togo, dim3(1), dim3(64), 0, r.stream, r.d_key, r.W, r.H, (uint32_t)r.W * (uint32_t)r.H, r.layers, n_robots,
                     reinterpret_cast<const tsd_drive_pose*>(d), d + 6 * R);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(h + 6 * R, d + 6 * R, R * 4, hipMemcpyDeviceToHost, r.stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(r.stream));
  std::memcpy(togo_host, h + 6 * R, R * 4);
  return TSD_OK;
}

void drive_free(tsd_ctx* ctx)
{
  hipFree(ctx->drive.d_buf);
  if (ctx->drive.h_buf) hipHostFree(ctx->drive.h_buf);
  hipFree(ctx->drive.live.d_words);
  hipFree(ctx->drive.live.d_pts);
  if (ctx->drive.live.h_pts) hipHostFree(ctx->drive.live.h_pts);
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

int tsd_drive_fleet_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_fleet_params* fleet, const tsd_drive_pose* poses,
                            int n_robots, tsd_drive_choice* choice_host, uint64_t* scores_host, uint16_t* why_host, int64_t* tracks_host)
{
  if (!ctx) return TSD_E_ARG;
  return drive_fleet_rollout(ctx, params, fleet, poses, n_robots, choice_host, scores_host, why_host, tracks_host);
}

int tsd_drive_fields_togo(tsd_ctx* ctx, const tsd_drive_pose* poses, int n_robots, uint32_t* togo_host)
{
  if (!ctx) return TSD_E_ARG;
  return drive_fields_togo(ctx, poses, n_robots, togo_host);
}

int tsd_drive_live_set(tsd_ctx* ctx, const tsd_drive_live_params* params, const int32_t* points_xy, int n, int width, int height, int* n_kept)
{
  if (!ctx) return TSD_E_ARG;
  return drive_live_set(ctx, params, points_xy, n, width, height, n_kept);
}

int tsd_drive_live_clear(tsd_ctx* ctx)
{
  if (!ctx) return TSD_E_ARG;
  ctx->drive.live.set = false;                                 // (the image keeps its bits: the next set empties it first)
  return TSD_OK;
}

int tsd_drive_live_fetch(tsd_ctx* ctx, uint32_t* words_host, long long cap_words, int* width, int* height, int* stride_words)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Drive::Live& l = ctx->drive.live;
  if (!l.set) return map_refused(ctx, "tsd_drive_live_fetch", "no live layer");
  const long long words = (long long)l.stride * l.H;
  if (words_host && cap_words < words) return map_refused(ctx, "tsd_drive_live_fetch", "cap_words is below stride_words * height");
  if (words_host) {
    TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    TSD_HIP_CHECK(ctx, hipMemcpy(words_host, l.d_words, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  if (width) *width = l.W;
  if (height) *height = l.H;
  if (stride_words) *stride_words = l.stride;
  return TSD_OK;
}

int tsd_drive_live_dev_ptr(tsd_ctx* ctx, const void** words_dev, int* width, int* height, int* stride_words)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Drive::Live& l = ctx->drive.live;
  if (!l.set) return map_refused(ctx, "tsd_drive_live_dev_ptr", "no live layer");
  if (words_dev) *words_dev = l.d_words;
  if (width) *width = l.W;
  if (height) *height = l.H;
  if (stride_words) *stride_words = l.stride;
  return TSD_OK;
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
