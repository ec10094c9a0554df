// fuse.hip -- TSD-level fusion of several grids on ONE GPU into one grid (tsd_fuse_* of include/tsd_hip.h).  Not in the reference, whose
// robots share one TsdGrid; here every robot of the multi-robot mode may own a grid, and this is how they get a common one.
//
// A cell is a running weighted mean (TsdGridPartition::addTsd), an untouched "empty" tile is shorthand for tsd = 1, W = _initWeight
// (TsdGridPartition::init), so the weight-weighted mean of the members' cells is the cell of the grid that saw all their scans.  The
// rule, contributor by contributor, is spelled out at tsd_fuse_begin in the header; tests/tsd_fuse_ref.py restates it in numpy and the
// kernel equals that bit for bit with fp64 cells.
//
// Ordering (events only; the host waits for nothing before tsd_fuse_wait, nothing spins on the device, the NULL stream stays unused):
//   member i's streams   :  record ev_fuse_src (grid stream) / ev_fuse_src_push (push stream of the asynchronous mapping)
//   destination's stream :  [its own waits: readers on the sensors' streams, an asynchronous push]  wait ev_fuse_src*[*]
//                           clear the push bookkeeping  k_tsd_fuse  record ev_fuse_read[*]  copy the counters to the host
//   member i's streams   :  wait ev_fuse_read[i]   -- whatever the member enqueues next, its grid writes included, runs behind the fusion
// The events belong to the member, so either side may be destroyed with a fusion in flight: tsd_destroy drains the context's own
// streams, and those have waited for every event the other side recorded.
#include "capi_internal.hpp"

#include <memory>

namespace tsd {

constexpr int FUSE_MAX = 64;
// the counters are one atomic per workgroup and kind, spread over 32 lines of their own like group.hip's GROUP_COUNT_SHARDS (16 384
// workgroups adding to one address are handed through one after the other); tsd_fuse_wait sums the lines
constexpr int FUSE_SHARDS = 32, FUSE_STRIDE = 16;
constexpr size_t kFuseStatBytes = (size_t)FUSE_SHARDS * FUSE_STRIDE * sizeof(unsigned long long);
enum : int { FS_MATERIALISED = 0, FS_EMPTY = 1, FS_ONE = 2, FS_MANY = 3 };

struct FuseMember {
  const uint8_t* flags; const double* init_weight; const tsd_cell_t* tsd; const w_cell_t* weight;
  int ox, oy, PX, pad;       // the member's cell (x, y) is the destination's cell (x + ox, y + oy); tiles per side
};
struct FuseArgs {            // by value: the member table is read from the kernel-argument segment, uniformly
  uint8_t* flags; double* init_weight; tsd_cell_t* tsd; w_cell_t* weight; unsigned long long* negmask;
  unsigned long long* stats;
  int N, PX, n, pad;
  FuseMember m[FUSE_MAX];
};
static_assert(sizeof(FuseArgs) <= 4096, "FuseArgs travels as a kernel argument");

// the contributors of one fused cell, in member order
struct FuseAcc {
  int cnt; double t0, num, den;
  __device__ __forceinline__ void init() { cnt = 0; t0 = 0.0; num = 0.0; den = 0.0; }
  __device__ __forceinline__ void take(double t, double w)
  {
    if (cnt == 0) t0 = t;
    cnt++;
    num += t * w;            // (-ffp-contract=off: a product, then a sum)
    den += w;
  }
  __device__ __forceinline__ void result(double& t, double& w) const
  {
    if (cnt == 0) { t = __builtin_nan(""); w = 0.0; }
    else if (cnt == 1) { t = t0; w = fmin(den, MAX_WEIGHT); }           // verbatim (den = 0 + w): fusing one grid is an identity
    else if (den > 0.0) { t = num / den; w = fmin(den, MAX_WEIGHT); }
    else { t = t0; w = 0.0; }                                            // cells freed by freeFootprint: weight 0 on every side
  }
};

__device__ __forceinline__ unsigned long long fuse_key(double t)         // equal for equal cells, NaN payloads aside
{
  return isnan(t) ? ~0ull : (unsigned long long)__double_as_longlong(t);
}

// One 256-lane workgroup per destination tile.  Lane `tid` owns the interior cells (tid & 31, k * 8 + (tid >> 5)), k = 0 .. 3 -- a wave's
// load or store covers two whole 256-byte rows -- and lanes 0 .. 64 one of the tile's 65 halo cells each: a halo cell is the fused state
// of the grid cell it duplicates, a function of the members alone, so no workgroup waits for another and there is no second pass.
// Per member the 33 x 33 cells of the tile fall into at most 2 x 2 source tiles whose flags and _initWeight are the same for the whole
// workgroup: a member that does not reach the tile costs those reads and a uniform branch.  Source cells are read from the source
// tiles' INTERIORS only (their halos may be stale, TsdGridPartition.cpp:97); a destination row is two aligned segments of source rows.
__global__ void __launch_bounds__(256) k_tsd_fuse(const FuseArgs a)
{
  __shared__ unsigned long long s_neg, s_ref_t, s_ref_w;
  __shared__ int s_cnt[8], s_differs;
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  const int tile = (int)blockIdx.x, tx = tile % a.PX, ty = tile / a.PX;
  const int gx0 = tx * TILE_DIM, gy0 = ty * TILE_DIM;
  const int ix = tid & 31, iy0 = tid >> 5;
  const int hx = tid < TILE_DIM ? TILE_DIM : tid - TILE_DIM, hy = tid < TILE_DIM ? tid : TILE_DIM;     // this lane's halo cell (tid < 65)
  const bool halo = tid < 2 * TILE_DIM + 1 && gx0 + hx < a.N && gy0 + hy < a.N;      // beyond the grid's edge: (NaN, 0)
  if (tid == 0) { s_neg = 0ull; s_differs = 0; }

  FuseAcc acc[5];
#pragma unroll
  for (int k = 0; k < 5; k++) acc[k].init();
  bool materialise = false;        // a member's initialised tile intersects this tile's interior
  double mat_iw = 0.0;             // ... the first one's _initWeight (dead state of a materialised tile; kept so that one grid fuses to itself)

  for (int i = 0; i < a.n; i++) {
    const FuseMember& m = a.m[i];
    const int bx = gx0 - m.ox, by = gy0 - m.oy;         // the member's cell under this tile's cell (0, 0)
    const int sx0 = bx >> 5, sy0 = by >> 5, rx = bx & 31, ry = by & 31;
    int st[4]; double iw[4]; int sp[4];                 // per source tile: 0 nothing, 1 initialised, 2 empty (_initWeight > 0); its index
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int sx = sx0 + (q & 1), sy = sy0 + (q >> 1);
      st[q] = 0; iw[q] = 0.0; sp[q] = 0;
      if ((unsigned)sx < (unsigned)m.PX && (unsigned)sy < (unsigned)m.PX) {
        sp[q] = sy * m.PX + sx;
        iw[q] = m.init_weight[sp[q]];
        st[q] = m.flags[sp[q]] ? 1 : (iw[q] > 0.0 ? 2 : 0);
      }
      any |= st[q] != 0;
      // (source tile column sx0 + 1 reaches the interior only when the offset is not a multiple of 32; likewise the rows)
      if (st[q] == 1 && ((q & 1) == 0 || rx > 0) && ((q >> 1) == 0 || ry > 0) && !materialise) { materialise = true; mat_iw = iw[q]; }
    }
    if (!any) continue;
    // (as values: selected between by lane, the arrays themselves would be kept in memory -- and so would the member table, were
    // its entry referred to from inside a closure)
    const int st0 = st[0], st1 = st[1], st2 = st[2], st3 = st[3], sp0 = sp[0], sp1 = sp[1], sp2 = sp[2], sp3 = sp[3];
    const double iw0 = iw[0], iw1 = iw[1], iw2 = iw[2], iw3 = iw[3];
    const tsd_cell_t* const mt = m.tsd;
    const w_cell_t* const mw = m.weight;
#define TSD_FUSE_TAKE(c, cx, cy)                                                                         \
    do {                                                                                                 \
      const int mx = bx + (cx), my = by + (cy);          /* the member's cell under the tile's cell (cx, cy), 0 .. 32 each */ \
      const bool hi_x = (mx >> 5) != sx0, hi_y = (my >> 5) != sy0;                                       \
      const int s = hi_y ? (hi_x ? st3 : st2) : (hi_x ? st1 : st0);                                      \
      if (s == 1) {                                                                                      \
        const int p = hi_y ? (hi_x ? sp3 : sp2) : (hi_x ? sp1 : sp0);                                    \
        const size_t off = (size_t)p * TILE_STRIDE + (size_t)((my & 31) * TILE_DIM + (mx & 31));         \
        const double tv = ld_tsd(mt + off), wv = ld_w(mw + off);                                         \
        if (!isnan(tv)) (c).take(tv, wv);                                                                \
      } else if (s == 2) {                                                                               \
        (c).take(1.0, hi_y ? (hi_x ? iw3 : iw2) : (hi_x ? iw1 : iw0));                                   \
      }                                                                                                  \
    } while (0)
#pragma unroll
    for (int k = 0; k < 4; k++) TSD_FUSE_TAKE(acc[k], ix, k * 8 + iy0);
    if (halo) TSD_FUSE_TAKE(acc[4], hx, hy);
#undef TSD_FUSE_TAKE
  }

  double t[5], w[5];
#pragma unroll
  for (int k = 0; k < 5; k++) acc[k].result(t[k], w[k]);
  if (tid == 0) { s_ref_t = fuse_key(t[0]); s_ref_w = (unsigned long long)__double_as_longlong(w[0]); }
  __syncthreads();
  int differs = 0, one = 0, many = 0;
  unsigned long long neg = 0ull;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    differs |= fuse_key(t[k]) != s_ref_t || (unsigned long long)__double_as_longlong(w[k]) != s_ref_w;
    one += acc[k].cnt == 1; many += acc[k].cnt > 1;
    // rows k * 8 + wave * 2 + {0, 1}: both in group row k * 2 + (wave >> 1); lane l and lane l + 32 share a column
    const unsigned long long b = __ballot(t[k] < 0.0);
    const unsigned cols = (unsigned)b | (unsigned)(b >> 32);
    unsigned g8 = 0;
#pragma unroll
    for (int gx = 0; gx < 8; gx++) g8 |= ((cols >> (4 * gx)) & 0xFu) ? 1u << gx : 0u;
    neg |= (unsigned long long)g8 << (8 * (k * 2 + (wave >> 1)));
  }
  // a tile none of whose 1024 cells differ stays unmaterialised (the fusion of whole empty / unknown tiles); the empty tiles of members
  // shifted by less than a tile give cells that differ, and those are materialised like data
  one = wave_sum_i(one); many = wave_sum_i(many);
  if (__any(differs) && (tid & 63) == 0) s_differs = 1;        // (every writer stores the same value)
  if ((tid & 63) == 0) {
    s_cnt[wave * 2] = one; s_cnt[wave * 2 + 1] = many;
    if (neg) atomicOr(&s_neg, neg);
  }
  __syncthreads();
  const bool mat = s_differs != 0 || materialise;
  if (mat) {
    tsd_cell_t* T = a.tsd + (size_t)tile * TILE_STRIDE;
    w_cell_t* W = a.weight + (size_t)tile * TILE_STRIDE;
#pragma unroll
    for (int k = 0; k < 4; k++) st_cell(T, W, k * 256 + tid, t[k], w[k]);
    if (tid < 2 * TILE_DIM + 1) st_cell(T, W, cell_off(hx, hy), t[4], w[4]);
  }
  if (tid == 0) {
    const double ref_w = __longlong_as_double((long long)s_ref_w);
    const double iw_out = materialise ? mat_iw : (mat || s_ref_t == ~0ull) ? 0.0 : ref_w;
    a.flags[tile] = mat ? 1 : 0;
    a.init_weight[tile] = iw_out;
    a.negmask[tile] = s_neg;
    unsigned long long* sh = a.stats + (size_t)(blockIdx.x & (FUSE_SHARDS - 1)) * FUSE_STRIDE;
    const int n_one = s_cnt[0] + s_cnt[2] + s_cnt[4] + s_cnt[6], n_many = s_cnt[1] + s_cnt[3] + s_cnt[5] + s_cnt[7];
    if (mat) atomicAdd(sh + FS_MATERIALISED, 1ull);
    else if (iw_out > 0.0) atomicAdd(sh + FS_EMPTY, 1ull);
    if (n_one) atomicAdd(sh + FS_ONE, (unsigned long long)n_one);
    if (n_many) atomicAdd(sh + FS_MANY, (unsigned long long)n_many);
  }
}

static int launch_fuse(tsd_ctx* dst, const FuseArgs& a)
{
  ScopedKernelTimer t(dst, "fuse");
  hipExtLaunchKernelGGL(k_tsd_fuse, dim3((unsigned)dst->grid.tiles), dim3(256), 0, dst->stream, t.a, t.b, 0, a);
  TSD_HIP_CHECK(dst, hipGetLastError());
  return TSD_OK;
}

static int fuse_event(tsd_ctx* err_to, hipEvent_t* e)
{
  if (!*e) TSD_HIP_CHECK(err_to, hipEventCreateWithFlags(e, hipEventDisableTiming));
  return TSD_OK;
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_fuse_begin(tsd_ctx* dst, int n, tsd_ctx* const* src, const int32_t* cell_off_xy)
{
  if (!dst) return TSD_E_ARG;
  // ---- argument checks: nothing here touches the HIP runtime or a grid
  auto refuse = [&](const char* what) { return set_error(dst, TSD_E_ARG, what, hipSuccess); };
  if (n < 1 || n > FUSE_MAX) return refuse("tsd_fuse: the number of members must be 1 .. 64");
  if (!src) return refuse("tsd_fuse: no members");
  for (int i = 0; i < n; i++) if (!src[i]) return refuse("tsd_fuse: a member is NULL");
  for (int i = 0; i < n; i++) {
    if (src[i] == dst) return refuse("tsd_fuse: the destination is among the members");
    for (int j = 0; j < i; j++) if (src[j] == src[i]) return refuse("tsd_fuse: a member is listed twice");
  }
  for (int i = 0; i < n; i++) if (src[i]->device != dst->device) return refuse("tsd_fuse: the members and the destination must be on one device");
  for (int i = 0; i < n; i++) {
    if (std::memcmp(&src[i]->grid.cs, &dst->grid.cs, sizeof(double)) != 0) return refuse("tsd_fuse: a member's cell size differs from the destination's");
    if (std::memcmp(&src[i]->grid.max_trunc, &dst->grid.max_trunc, sizeof(double)) != 0)
      return refuse("tsd_fuse: a member's max_truncation differs from the destination's");
  }
  for (int i = 0; cell_off_xy && i < 2 * n; i++)
    if (cell_off_xy[i] < -(1 << 24) || cell_off_xy[i] > (1 << 24)) return refuse("tsd_fuse: an offset is outside +-2^24 cells");

  auto args = std::make_unique<FuseArgs>();
  FuseArgs& a = *args;
  std::memset(&a, 0, sizeof(a));
  const GridDev& g = dst->grid;
  a.flags = g.flags; a.init_weight = g.init_weight; a.tsd = g.tsd; a.weight = g.weight; a.negmask = g.negmask;
  a.N = g.N; a.PX = g.PX; a.n = n;
  for (int i = 0; i < n; i++) {
    const GridDev& s = src[i]->grid;
    a.m[i] = FuseMember{s.flags, s.init_weight, s.tsd, s.weight, cell_off_xy ? cell_off_xy[2 * i] : 0, cell_off_xy ? cell_off_xy[2 * i + 1] : 0, s.PX, 0};
  }

  // Every context involved is held while the fusion is enqueued, and only then (address order: two fusions cannot deadlock): a grid
  // write of a member that slipped in between "written so far" and "the fusion has read" would run beside the kernel.
  std::vector<tsd_ctx*> all(src, src + n);
  all.push_back(dst);
  std::sort(all.begin(), all.end());
  std::vector<std::unique_lock<std::mutex>> held;
  held.reserve(all.size());
  for (tsd_ctx* c : all) held.emplace_back(c->order_mutex);

  if (int rc = enter(dst)) return rc;
  if (!dst->d_fuse_stats) {
    TSD_HIP_CHECK(dst, hipMalloc(&dst->d_fuse_stats, kFuseStatBytes));
    TSD_HIP_CHECK(dst, hipHostMalloc(&dst->h_fuse_stats, kFuseStatBytes, hipHostMallocDefault));
  }
  a.stats = dst->d_fuse_stats;
  WriterScope w(dst, /*held=*/true); if (w.rc) return w.rc;
  for (int i = 0; i < n; i++) {
    tsd_ctx* m = src[i];
    if (int rc = fuse_event(dst, &m->ev_fuse_src)) return rc;
    if (int rc = fuse_event(dst, &m->ev_fuse_read)) return rc;
    TSD_HIP_CHECK(dst, hipEventRecord(m->ev_fuse_src, m->stream));
    TSD_HIP_CHECK(dst, hipStreamWaitEvent(dst->stream, m->ev_fuse_src, 0));
    if (m->stream_push) {                   // asynchronous mapping: the member's pushes run on a stream of their own
      if (int rc = fuse_event(dst, &m->ev_fuse_src_push)) return rc;
      TSD_HIP_CHECK(dst, hipEventRecord(m->ev_fuse_src_push, m->stream_push));
      TSD_HIP_CHECK(dst, hipStreamWaitEvent(dst->stream, m->ev_fuse_src_push, 0));
    }
  }
  // the push bookkeeping as tsd_reset leaves it: the fused halos agree with their neighbours, nothing is dirty
  if (int rc = reset_push_bookkeeping(dst)) return rc;
  TSD_HIP_CHECK(dst, hipMemsetAsync(dst->d_fuse_stats, 0, kFuseStatBytes, dst->stream));
  if (int rc = launch_fuse(dst, a)) return rc;
  for (int i = 0; i < n; i++) {
    tsd_ctx* m = src[i];
    TSD_HIP_CHECK(dst, hipEventRecord(m->ev_fuse_read, dst->stream));
    TSD_HIP_CHECK(dst, hipStreamWaitEvent(m->stream, m->ev_fuse_read, 0));
    if (m->stream_push) TSD_HIP_CHECK(dst, hipStreamWaitEvent(m->stream_push, m->ev_fuse_read, 0));
  }
  TSD_HIP_CHECK(dst, hipMemcpyAsync(dst->h_fuse_stats, dst->d_fuse_stats, kFuseStatBytes, hipMemcpyDeviceToHost, dst->stream));
  dst->fuse_begun = true;
  return TSD_OK;
}

int tsd_fuse_wait(tsd_ctx* dst, tsd_fuse_stats* stats)
{
  if (!dst) return TSD_E_ARG;
  if (!dst->fuse_begun) return set_error(dst, TSD_E_ARG, "tsd_fuse_wait without tsd_fuse_begin", hipSuccess);
  TSD_HIP_CHECK(dst, hipSetDevice(dst->device));
  TSD_HIP_CHECK(dst, hipStreamSynchronize(dst->stream));
  dst->fuse_begun = false;
  if (stats) {
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int k = 0; k < FUSE_SHARDS; k++)
      for (int j = 0; j < 4; j++) s[j] += dst->h_fuse_stats[k * FUSE_STRIDE + j];
    stats->tiles_materialised = (int64_t)s[FS_MATERIALISED]; stats->tiles_empty = (int64_t)s[FS_EMPTY];
    stats->cells_one_source = (int64_t)s[FS_ONE]; stats->cells_many_sources = (int64_t)s[FS_MANY];
    stats->cells_valid = (int64_t)(s[FS_ONE] + s[FS_MANY]);      // every contributor holds a value, and so does their mean
  }
  return TSD_OK;
}

int tsd_fuse(tsd_ctx* dst, int n, tsd_ctx* const* src, const int32_t* cell_off_xy, tsd_fuse_stats* stats)
{
  const int rc = tsd_fuse_begin(dst, n, src, cell_off_xy);
  if (rc != TSD_OK) return rc;
  return tsd_fuse_wait(dst, stats);
}

}  // extern "C"
