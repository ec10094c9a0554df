// view.hip -- what a scanner standing on a cell of an int8 map would see: the expected gain of exploration goals, the claims that keep
// two robots from being sent to look at the same space, and the assignment built on both (tsd_view_gains / _claim / _claims_reset /
// _claims_dev_ptr / _assign of include/tsd_hip.h, where the rule is written out).  All in integers.
//
// k_view<CLAIM>  one workgroup per candidate.  The seen set is a bit mask of the candidate's window in dynamic LDS: 2R + 1 rows of
//                ceil((2R + 1) / 32) words, sized by the call's radius.
//   rays         A ray's cell at step j is a closed form in j, so a ray is no chain of dependent loads: VIEW_L lanes (the power of
//                two at or above R, at most 64) take VIEW_L consecutive steps of one ray at once -- 64 / VIEW_L rays side by side in a
//                wave where the radius is small.  A lane loads its cell and, where its step is diagonal, the two cells the step cuts;
//                a ballot of the lanes at which the ray ends keeps the lanes in front of the first; unknown_depth is a prefix count
//                over the ballot of the unknown lanes among those, carried from one 64-step chunk of a long ray to the next.  The
//                lanes kept set their bits with atomicOr on the LDS words (after a plain look: near the candidate most bits are set
//                already).  The divisions by 2R are a multiplication by a host-made reciprocal, exact for every numerator of the rule.
//   closing      every cell of the window inside the map, consecutive lanes on consecutive cells of a row: where its bit is set the
//                map byte says unknown or clear -- the map is read again instead of a second mask, which is what lets R = 511 fit
//                (130 944 B) -- and the claims byte says claimed or not.  CLAIM = false: popcounts, one lane writes the record.  CLAIM
//                = true: a byte store of 1 on every unknown cell seen.  Stores of one value from many workgroups: no atomics, no order.
//
// No workgroup reads what another one writes in the same launch: gains read the claims and write records, claims write the claims.
#include "map_product.hpp"

#include <algorithm>
#include <cstring>

namespace tsd {

constexpr int VIEW_THREADS = 1024;                   // 16 waves: a candidate's rays are independent, and a call often brings few candidates

struct ViewArgs {
  int R, free_max, depth;
  uint32_t recip;                                    // floor(2^32 / 2R) + 1: umulhi(n, recip) == n / 2R for every n <= 2 R^2 + R (host: view_recip)
  int L, l2;                                         // lanes per ray, a power of two, and its log2
  int wpr;                                           // words per row of the window's mask
};

// ray r of the 8R in the rule's order: top row, right column, bottom row, left column
__device__ __forceinline__ void view_target(int r, int R, int& tx, int& ty)
{
  if (r <= 2 * R) { tx = r - R; ty = -R; return; }
  r -= 2 * R + 1;
  if (r < 2 * R) { tx = R; ty = r - R + 1; return; }
  r -= 2 * R;
  if (r < 2 * R) { tx = R - 1 - r; ty = R; return; }
  r -= 2 * R;
  tx = -R; ty = R - 1 - r;
}

template <bool CLAIM>
__global__ void __launch_bounds__(VIEW_THREADS)
k_view(MapView m, ViewArgs a, const uint32_t* __restrict__ cells, const uint8_t* claims_in, uint8_t* claims_out,
       tsd_view_gain* __restrict__ out)
{
  extern __shared__ uint32_t s_mask[];               // [(2R + 1) * wpr]
  __shared__ int s_sum[3][VIEW_THREADS / 64];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t cell = cells[blockIdx.x];
  const int R = a.R;
  bool empty = cell >= (uint32_t)m.W * (uint32_t)m.H;
  int cx = 0, cy = 0;
  if (!empty) {
    cx = (int)(cell % (uint32_t)m.W); cy = (int)(cell / (uint32_t)m.W);
    empty = m.map[(size_t)cy * m.stride + cx] > a.free_max;
  }
  if (empty) {                                       // (the same for every lane) outside the map or on a blocking cell: nothing is seen
    if (!CLAIM && t == 0) out[blockIdx.x] = tsd_view_gain{cell, 0u, 0u, 0u};
    return;
  }
  const int rows = 2 * R + 1, words = rows * a.wpr;
  for (int i = t; i < words; i += VIEW_THREADS) s_mask[i] = 0u;
  __syncthreads();
  if (t == 0) s_mask[R * a.wpr + (R >> 5)] = 1u << (R & 31);      // the candidate's own cell (no ray sets it: a step moves)
  __syncthreads();

  // ---- rays
  const int L = a.L, sub = lane & (L - 1), grp = lane >> a.l2, per_wave = 64 >> a.l2, n_rays = 8 * R;
  const unsigned long long grp_mask = L == 64 ? ~0ull : ((1ull << L) - 1ull);
  const int grp_shift = grp << a.l2;
  for (int base = wave * per_wave; base < n_rays; base += (VIEW_THREADS / 64) * per_wave) {
    const int r = base + grp;
    int tx = 0, ty = 0;
    bool alive = r < n_rays;
    if (alive) view_target(r, R, tx, ty);
    const int ax = abs(tx), ay = abs(ty);
    int carry = 0;                                   // the unknown cells this ray has seen in the chunks before
    for (int j0 = 0; j0 < R; j0 += L) {              // (L < 64 only where R <= L: one chunk)
      const int j = j0 + sub + 1;
      bool end = !alive || j > R;
      int v = 0, ox = 0, oy = 0;
      if (!end) {
        ox = (int)__umulhi((uint32_t)(2 * j * ax + R), a.recip);
        oy = (int)__umulhi((uint32_t)(2 * j * ay + R), a.recip);
        const int qx = (int)__umulhi((uint32_t)(2 * (j - 1) * ax + R), a.recip), qy = (int)__umulhi((uint32_t)(2 * (j - 1) * ay + R), a.recip);
        const int x = cx + (tx < 0 ? -ox : ox), y = cy + (ty < 0 ? -oy : oy);
        end = ox * ox + oy * oy > R * R || x < 0 || x >= m.W || y < 0 || y >= m.H;
        if (!end) {
          v = m.map[(size_t)y * m.stride + x];
          if (ox != qx && oy != qy) {                // a diagonal step: the two cells it cuts
            const int px = cx + (tx < 0 ? -qx : qx), py = cy + (ty < 0 ? -qy : qy);
            const bool in_p = px >= 0 && px < m.W && py >= 0 && py < m.H;       // (false only behind the ray's end)
            const bool b1 = !in_p || m.map[(size_t)py * m.stride + x] > a.free_max;
            const bool b2 = !in_p || m.map[(size_t)y * m.stride + px] > a.free_max;
            end = b1 && b2;
          }
          end = end || v > a.free_max;
        }
      }
      const unsigned long long ends = (__ballot(end) >> grp_shift) & grp_mask;
      const int first = ends ? __ffsll((long long)ends) - 1 : L;
      const bool kept = sub < first;
      const unsigned long long unk = (__ballot(kept && v < 0) >> grp_shift) & grp_mask;
      bool seen = kept;
      if (a.depth > 0) {
        const int before = carry + __popcll(unk & ((1ull << sub) - 1ull));
        seen = kept && before < a.depth;             // the ray ends behind its depth-th unknown cell
        carry += __popcll(unk);
      }
      if (seen) {
        const int bx = (tx < 0 ? -ox : ox) + R, by = (ty < 0 ? -oy : oy) + R;
        uint32_t* w = s_mask + by * a.wpr + (bx >> 5);
        const uint32_t bit = 1u << (bx & 31);
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) atomicOr(w, bit);
      }
      alive = alive && first == L && (a.depth == 0 || carry < a.depth);
      if (!__any(alive)) break;
    }
  }
  __syncthreads();

  // ---- closing pass over the window's part of the map
  const int x0 = max(cx - R, 0), x1 = min(cx + R, m.W - 1), y0 = max(cy - R, 0), y1 = min(cy + R, m.H - 1);
  int visible = 0, unknown = 0, gain = 0;
  for (int y = y0 + wave; y <= y1; y += VIEW_THREADS / 64) {                       // a wave per row, consecutive lanes on consecutive cells
    const uint32_t* row = s_mask + (y - cy + R) * a.wpr;
    for (int x = x0 + lane; x <= x1; x += 64) {
      const int bx = x - cx + R;
      if (!((row[bx >> 5] >> (bx & 31)) & 1u)) continue;
      visible++;
      if (m.map[(size_t)y * m.stride + x] >= 0) continue;
      const size_t c = (size_t)y * m.W + x;
      if (CLAIM) { claims_out[c] = 1; continue; }
      unknown++;
      if (!claims_in || claims_in[c] == 0) gain++;
    }
  }
  if (CLAIM) return;
  visible = wave_sum_i(visible); unknown = wave_sum_i(unknown); gain = wave_sum_i(gain);
  if (lane == 0) { s_sum[0][wave] = visible; s_sum[1][wave] = unknown; s_sum[2][wave] = gain; }
  __syncthreads();
  if (t == 0) {
    int s[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++)
      for (int w = 0; w < VIEW_THREADS / 64; w++) s[k] += s_sum[k][w];
    out[blockIdx.x] = tsd_view_gain{cell, (uint32_t)s[2], (uint32_t)s[1], (uint32_t)s[0]};
  }
}

// ---- host
static uint32_t view_recip(int R) { return (uint32_t)((1ull << 32) / (unsigned)(2 * R)) + 1u; }

static ViewArgs view_args(const tsd_view_params* p)
{
  ViewArgs a{};
  a.R = p->radius; a.free_max = p->free_max; a.depth = p->unknown_depth;
  a.recip = view_recip(p->radius);
  a.l2 = 0;
  while ((1 << a.l2) < p->radius && a.l2 < 6) a.l2++;
  a.L = 1 << a.l2;
  a.wpr = (2 * p->radius + 1 + 31) / 32;
  return a;
}

static const char* vw_params_wrong(const tsd_view_params* p)
{
  if (!p) return "params is NULL";
  if (p->free_max < 0 || p->free_max > 99) return "free_max is outside 0 .. 99";
  if (p->radius < 1 || p->radius > TSD_VIEW_MAX_RADIUS) return "radius is outside 1 .. TSD_VIEW_MAX_RADIUS";
  if (p->unknown_depth < 0) return "unknown_depth is negative";
  return nullptr;
}

// The views' entry points take both forms in one signature: map_dev NULL is the staged map of the last frame.
static int vw_map_source(tsd_ctx* ctx, const char* who, const void* map_dev, int width, int height, int stride, MapSource* src)
{
  return map_dev ? map_source_caller(ctx, who, map_dev, width, height, stride, src) : map_source_frame(ctx, who, false, src);
}

static bool vw_claims_fit(const tsd_ctx* ctx, const MapView& m) { return ctx->view.d_claims && ctx->view.cW == m.W && ctx->view.cH == m.H; }

// The claims image at W x H, all 0, enqueued on `stream` (not waited for).
static int vw_claims_reset(tsd_ctx* ctx, hipStream_t stream, int W, int H)
{
  tsd_ctx::View& v = ctx->view;
  const size_t cells = (size_t)W * H;
  if (v.claims_cap < cells) { v.cW = v.cH = 0; }
  if (int rc = scratch_grow(ctx, "tsd_view", &v.d_claims, &v.claims_cap, cells, "the claims image")) return rc;
  v.cW = W; v.cH = H;
  TSD_HIP_CHECK(ctx, hipMemsetAsync(v.d_claims, 0, cells, stream));
  return TSD_OK;
}

// The candidates' buffers for n cells; h_cells holds the caller's cells on return.
static int vw_stage(tsd_ctx* ctx, const uint32_t* cells, int n)
{
  tsd_ctx::View& v = ctx->view;
  if (int rc = scratch_grow_all(ctx, "tsd_view", &v.cap, std::max<size_t>((size_t)n, 64), scratch_part(&v.d_cells, "the candidates"),
                                scratch_part(&v.d_rec, "the records"), scratch_part(&v.h_cells, "the candidates' pinned copy", true),
                                scratch_part(&v.h_rec, "the records' pinned copy", true))) return rc;   // (invalidates nothing: no result is kept)
  std::memcpy(v.h_cells, cells, (size_t)n * sizeof(uint32_t));
  return TSD_OK;
}

// One launch over n candidates.  upload: they are the staged ones (h_cells), copied to d_cells first; otherwise `d_cells` points at
// candidates a launch before this one left on the device.  claim: the store pass, not waited for (what follows on the stream sees it);
// else the records arrive in h_rec and the call waits.
static int vw_run(tsd_ctx* ctx, const MapSource& src, const tsd_view_params* prm, const uint32_t* d_cells, int n, bool upload, bool claim)
{
  tsd_ctx::View& v = ctx->view;
  const ViewArgs a = view_args(prm);
  const size_t lds = (size_t)(2 * a.R + 1) * a.wpr * sizeof(uint32_t);
  const void* fn = claim ? reinterpret_cast<const void*>(&k_view<true>) : reinterpret_cast<const void*>(&k_view<false>);
  if (int rc = ensure_dynamic_lds(ctx, fn, lds)) return rc;
  if (upload) TSD_HIP_CHECK(ctx, hipMemcpyAsync(v.d_cells, v.h_cells, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, src.stream));
  {
    ScopedKernelTimer t(ctx, src.timed ? (claim ? "view_claim" : "view_gain") : "", true);
    if (claim)
      hipLaunchKernelGGL(k_view<true>, dim3((unsigned)n), dim3(VIEW_THREADS), lds, src.stream, src.m, a, d_cells, nullptr, v.d_claims, nullptr);
    else
      hipLaunchKernelGGL(k_view<false>, dim3((unsigned)n), dim3(VIEW_THREADS), lds, src.stream, src.m, a, d_cells,
                         prm->use_claims ? v.d_claims : nullptr, nullptr, v.d_rec);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  if (claim) return TSD_OK;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(v.h_rec, v.d_rec, (size_t)n * sizeof(tsd_view_gain), hipMemcpyDeviceToHost, src.stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(src.stream));
  return TSD_OK;
}

void view_free(tsd_ctx* ctx)
{
  tsd_ctx::View& v = ctx->view;
  hipFree(v.d_cells); hipFree(v.d_rec); hipFree(v.d_claims);
  if (v.h_cells) hipHostFree(v.h_cells);
  if (v.h_rec) hipHostFree(v.h_rec);
  v = tsd_ctx::View{};
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_view_gains(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                   const uint32_t* cells_host, int n, tsd_view_gain* out_host)
{
  if (!ctx) return TSD_E_ARG;
  if (const char* why = vw_params_wrong(params)) return set_error(ctx, TSD_E_ARG, (std::string("tsd_view_gains: ") + why).c_str(), hipSuccess);
  if (!cells_host || !out_host || n < 1 || n > TSD_VIEW_MAX_CELLS)
    return set_error(ctx, TSD_E_ARG, "tsd_view_gains: cells or out is NULL, or n is outside 1 .. TSD_VIEW_MAX_CELLS", hipSuccess);
  MapSource src{};
  if (int rc = vw_map_source(ctx, "tsd_view_gains", map_dev, width, height, stride, &src)) return rc;
  if (params->use_claims && !vw_claims_fit(ctx, src.m))
    return set_error(ctx, TSD_E_ARG, "tsd_view_gains: use_claims without a claims image of the map's size (tsd_view_claims_reset)", hipSuccess);
  if (int rc = map_source_enter(ctx, src)) return rc;
  if (int rc = vw_stage(ctx, cells_host, n)) return rc;
  if (int rc = vw_run(ctx, src, params, ctx->view.d_cells, n, true, false)) return rc;
  std::memcpy(out_host, ctx->view.h_rec, (size_t)n * sizeof(tsd_view_gain));
  return TSD_OK;
}

int tsd_view_claim(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                   const uint32_t* cells_host, int n)
{
  if (!ctx) return TSD_E_ARG;
  if (const char* why = vw_params_wrong(params)) return set_error(ctx, TSD_E_ARG, (std::string("tsd_view_claim: ") + why).c_str(), hipSuccess);
  if (!cells_host || n < 1 || n > TSD_VIEW_MAX_CELLS)
    return set_error(ctx, TSD_E_ARG, "tsd_view_claim: cells is NULL, or n is outside 1 .. TSD_VIEW_MAX_CELLS", hipSuccess);
  MapSource src{};
  if (int rc = vw_map_source(ctx, "tsd_view_claim", map_dev, width, height, stride, &src)) return rc;
  if (!vw_claims_fit(ctx, src.m))
    return set_error(ctx, TSD_E_ARG, "tsd_view_claim: no claims image of the map's size (tsd_view_claims_reset)", hipSuccess);
  if (int rc = map_source_enter(ctx, src)) return rc;
  if (int rc = vw_stage(ctx, cells_host, n)) return rc;
  if (int rc = vw_run(ctx, src, params, ctx->view.d_cells, n, true, true)) return rc;
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(src.stream));
  return TSD_OK;
}

int tsd_view_claims_reset(tsd_ctx* ctx, int width, int height)
{
  if (!ctx) return TSD_E_ARG;
  if (width < 1 || height < 1 || width > TSD_FRONTIER_MAX_SIDE || height > TSD_FRONTIER_MAX_SIDE)
    return set_error(ctx, TSD_E_ARG, "tsd_view_claims_reset: a side outside 1 .. TSD_FRONTIER_MAX_SIDE", hipSuccess);
  if (int rc = enter(ctx)) return rc;
  if (int rc = vw_claims_reset(ctx, ctx->stream, width, height)) return rc;
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}

int tsd_view_claims_dev_ptr(tsd_ctx* ctx, const void** claims_dev, int* width, int* height)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::View& v = ctx->view;
  if (!v.d_claims || v.cW == 0) return set_error(ctx, TSD_E_ARG, "tsd_view_claims_dev_ptr: no claims image", hipSuccess);
  if (claims_dev) *claims_dev = v.d_claims;
  if (width) *width = v.cW;
  if (height) *height = v.cH;
  return TSD_OK;
}

int tsd_view_assign(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                    const tsd_route_goal* goals, int n_goals, int n_robots, uint32_t gain_weight, int32_t* goal_of_robot,
                    tsd_view_gain* picked, int* rounds)
{
  if (!ctx) return TSD_E_ARG;
  if (const char* why = vw_params_wrong(params)) return set_error(ctx, TSD_E_ARG, (std::string("tsd_view_assign: ") + why).c_str(), hipSuccess);
  if (n_goals < 0 || n_goals > TSD_VIEW_MAX_CELLS || (n_goals > 0 && !goals) || n_robots < 1 || n_robots > TSD_FRONTIER_MAX_SEEDS || !goal_of_robot || !rounds)
    return set_error(ctx, TSD_E_ARG, "tsd_view_assign: n_goals outside 0 .. TSD_VIEW_MAX_CELLS, goals NULL, n_robots outside 1 .. TSD_FRONTIER_MAX_SEEDS, or a NULL output",
                     hipSuccess);
  MapSource src{};
  if (int rc = vw_map_source(ctx, "tsd_view_assign", map_dev, width, height, stride, &src)) return rc;
  if (int rc = map_source_enter(ctx, src)) return rc;
  if (int rc = vw_claims_reset(ctx, src.stream, src.m.W, src.m.H)) return rc;        // (the round's first launch runs behind it)
  tsd_view_params prm = *params;
  prm.use_claims = 1;
  for (int r = 0; r < n_robots; r++) {
    goal_of_robot[r] = -1;
    if (picked) picked[r] = tsd_view_gain{TSD_ROUTE_NONE, 0u, 0u, 0u};
  }
  std::vector<int> remaining;
  for (int k = 0; k < n_goals; k++)
    if (goals[k].cell != TSD_ROUTE_NONE && goals[k].seed >= 0 && goals[k].seed < n_robots) remaining.push_back(k);
  std::vector<uint32_t> cells;
  int n_rounds = 0;
  while (!remaining.empty()) {
    n_rounds++;
    cells.clear();
    for (int k : remaining) cells.push_back(goals[k].cell);
    if (int rc = vw_stage(ctx, cells.data(), (int)cells.size())) return rc;
    if (int rc = vw_run(ctx, src, &prm, ctx->view.d_cells, (int)cells.size(), true, false)) return rc;
    const tsd_view_gain* rec = ctx->view.h_rec;
    size_t best = 0;
    long long best_score = 0;
    for (size_t i = 0; i < remaining.size(); i++) {                                // (ascending goal index: the first of a tie stays)
      const long long score = (long long)rec[i].gain * (long long)gain_weight - (long long)goals[remaining[i]].dist;
      if (i == 0 || score > best_score) { best = i; best_score = score; }
    }
    if (rec[best].gain == 0) break;
    const int k = remaining[best], seed = goals[k].seed;
    goal_of_robot[seed] = k;
    if (picked) picked[seed] = rec[best];
    // the claim reads its cell where the round's gains left it; the next round's upload runs behind it on the stream
    if (int rc = vw_run(ctx, src, &prm, ctx->view.d_cells + best, 1, false, true)) return rc;
    remaining.erase(std::remove_if(remaining.begin(), remaining.end(), [&](int q) { return goals[q].seed == seed; }), remaining.end());
  }
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(src.stream));                            // (the last claim; the reset, where no round ran)
  *rounds = n_rounds;
  return TSD_OK;
}

int tsd_view_assign_fields(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                           const tsd_route_goal* goals, int n_frontiers, int n_robots, uint32_t gain_weight, int32_t* goal_of_robot,
                           tsd_view_gain* picked, int* rounds)
{
  if (!ctx) return TSD_E_ARG;
  if (const char* why = vw_params_wrong(params)) return set_error(ctx, TSD_E_ARG, (std::string("tsd_view_assign_fields: ") + why).c_str(), hipSuccess);
  if (n_frontiers < 0 || n_frontiers > TSD_VIEW_MAX_CELLS || (n_frontiers > 0 && !goals) || n_robots < 1 || n_robots > TSD_FRONTIER_MAX_SEEDS ||
      !goal_of_robot || !rounds)
    return set_error(ctx, TSD_E_ARG, "tsd_view_assign_fields: n_frontiers outside 0 .. TSD_VIEW_MAX_CELLS, goals NULL, n_robots outside 1 .. "
                                     "TSD_FRONTIER_MAX_SEEDS, or a NULL output", hipSuccess);
  MapSource src{};
  if (int rc = vw_map_source(ctx, "tsd_view_assign_fields", map_dev, width, height, stride, &src)) return rc;
  if (int rc = map_source_enter(ctx, src)) return rc;
  if (int rc = vw_claims_reset(ctx, src.stream, src.m.W, src.m.H)) return rc;        // (the round's first launch runs behind it)
  tsd_view_params prm = *params;
  prm.use_claims = 1;
  for (int r = 0; r < n_robots; r++) {
    goal_of_robot[r] = -1;
    if (picked) picked[r] = tsd_view_gain{TSD_ROUTE_NONE, 0u, 0u, 0u};
  }
  struct Pair { int f, r; };
  std::vector<Pair> remaining;                                                     // in ascending (f, r): the order of the tie
  for (int f = 0; f < n_frontiers; f++)
    for (int r = 0; r < n_robots; r++)
      if (goals[(size_t)r * n_frontiers + f].cell != TSD_ROUTE_NONE) remaining.push_back(Pair{f, r});
  std::vector<uint32_t> cells;
  std::vector<tsd_view_gain> rec;
  int n_rounds = 0;
  while (!remaining.empty()) {
    n_rounds++;
    // every distinct cell of the remaining pairs once, in launches of at most TSD_VIEW_MAX_CELLS candidates
    cells.clear();
    for (const Pair& p : remaining) cells.push_back(goals[(size_t)p.r * n_frontiers + p.f].cell);
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    rec.resize(cells.size());
    for (size_t at = 0; at < cells.size(); at += TSD_VIEW_MAX_CELLS) {
      const int n = (int)std::min<size_t>(cells.size() - at, TSD_VIEW_MAX_CELLS);
      if (int rc = vw_stage(ctx, cells.data() + at, n)) return rc;
      if (int rc = vw_run(ctx, src, &prm, ctx->view.d_cells, n, true, false)) return rc;
      std::memcpy(rec.data() + at, ctx->view.h_rec, (size_t)n * sizeof(tsd_view_gain));
    }
    const Pair* best = nullptr;
    long long best_score = 0;
    tsd_view_gain best_rec{};
    for (const Pair& p : remaining) {                                              // (ascending (f, r): the first of a tie stays)
      const tsd_route_goal& g = goals[(size_t)p.r * n_frontiers + p.f];
      const tsd_view_gain& v = rec[(size_t)(std::lower_bound(cells.begin(), cells.end(), g.cell) - cells.begin())];
      if (v.gain == 0) continue;                                                   // only pairs with a gain compete
      const long long score = (long long)v.gain * (long long)gain_weight - (long long)g.dist;
      if (!best || score > best_score) { best = &p; best_score = score; best_rec = v; }
    }
    if (!best) break;
    const int f = best->f, r = best->r;
    goal_of_robot[r] = f;
    if (picked) picked[r] = best_rec;
    // the claim uploads its one cell; it is waited for, so that the next round's staging does not write under the copy
    if (int rc = vw_stage(ctx, &best_rec.cell, 1)) return rc;
    if (int rc = vw_run(ctx, src, &prm, ctx->view.d_cells, 1, true, true)) return rc;
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(src.stream));
    remaining.erase(std::remove_if(remaining.begin(), remaining.end(), [&](const Pair& q) { return q.r == r || q.f == f; }), remaining.end());
  }
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(src.stream));                            // (the reset, where no round ran)
  *rounds = n_rounds;
  return TSD_OK;
}

}  // extern "C"
