// reloc.hip -- relocalisation: where in the grid was this scan taken?  (tsd_relocalize, include/tsd_hip.h)
//
// Every other localisation path starts from a known pose.  This one searches a pose lattice (nx x ny positions, ntheta rotations) on the
// TSD grid itself -- a scan end point lies on a surface, where |tsd| is small -- and hands the best local maxima to the existing
// registration; the selection among the refined poses is the reference's IcpMultiInitIterator rule (IcpMultiInitIterator.cpp:26-38).
//
//   k_reloc_score        one uint32 per candidate: sum over the scan points of 2^20 - rint(|tsd| * 2^20) at the point carried to the
//                        candidate pose, over the look-ups that succeed; 0 for every candidate whose position is not in seen free space.
//                        Integer terms: the sum does not depend on its order, so the wave reduction is exact.
//   k_reloc_peaks        strict local maxima over the 26 lattice neighbours (ties to the lower index), the 64 best of every workgroup
//   k_reloc_peaks_merge  the K best of those, score descending, index ascending
//
// Shape of the score kernels (reloc_shared.hpp's lattice_score; DESIGN.md 3.8, measured there).  A divergent gather like k_pdf_score: a
// workgroup = one position and a run of its rotations, the points staged in LDS once, a wave per rotation, lanes over points,
// RELOC_BATCH look-ups per lane in flight, the tile flag and the four cells of each issued together (tsd_device.hpp's lookup_issue).  The
// rotations of one position sweep the same discs of cells, so neighbouring waves hit the same lines.  The device computes no sine: the
// rotation table comes from the host.
//
// This file also holds the search's host side for both of its users (the map alignment, align.hip, is the other): the lattice's
// refusals and rotation table, the score volume's operations, the one launch of score and peak kernels.
#include "reloc_shared.hpp"

namespace tsd {

constexpr int RELOC_MIN_BLOCKS = 2048;     // a lattice of few positions is cut along its rotations until the launch has about this many workgroups
constexpr size_t RELOC_KEEP_CANDIDATES = (size_t)1 << 23;   // a score volume up to this (32 MiB) stays with the context for the next search

// the points as they are: every one, no pivot (x - 0.0 is x for every x)
__global__ void __launch_bounds__(64 * RELOC_WAVES)
k_reloc_score(GridDev g, RelocLattice L, const double* __restrict__ pts, int P, const double* __restrict__ cos_sin,
              uint32_t* __restrict__ scores, int rot_per_block)
{
  lattice_score<true>(g, L, pts, P, 1, 0.0, 0.0, cos_sin, scores, rot_per_block);
}

// ---- peaks: a stream of 64-bit keys (reloc_shared.hpp's peak_key), the best PK_KEEP kept in LDS -------------------------------------------
constexpr int PK_THREADS = 256;
constexpr int PK_CAP = 1024;               // keys the LDS buffer holds (a power of two: bitonic sort); a round adds at most PK_THREADS
constexpr int RELOC_PEAK_GRID = 512;       // workgroups of k_reloc_peaks at most; they stride over the volume

// all PK_THREADS threads; descending
__device__ void pk_sort(unsigned long long* s_keys)
{
  for (int k = 2; k <= PK_CAP; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < PK_CAP; i += PK_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = s_keys[i], b = s_keys[l];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) { s_keys[i] = b; s_keys[l] = a; }
        }
      }
    }
  __syncthreads();
}
// One round: every thread brings at most one key (0 = none).  Slots at and beyond *s_n hold 0 at all times, so the buffer sorts as a whole.
__device__ void pk_round(unsigned long long* s_keys, int* s_n, unsigned long long key)
{
  if (key) s_keys[atomicAdd(s_n, 1)] = key;
  __syncthreads();
  const int filled = *s_n;
  __syncthreads();                         // (every thread has read the count before the next round moves it)
  if (filled > PK_CAP - PK_THREADS) {      // (the same for every thread) the next round might not fit: keep the best PK_KEEP
    pk_sort(s_keys);
    for (int i = PK_KEEP + (int)threadIdx.x; i < PK_CAP; i += PK_THREADS) s_keys[i] = 0ull;
    if (threadIdx.x == 0) *s_n = PK_KEEP;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_THREADS)
k_reloc_peaks(const uint32_t* __restrict__ scores, int nx, int ny, int nt, int wraps, unsigned long long* __restrict__ wg_keys)
{
  __shared__ unsigned long long s_keys[PK_CAP];
  __shared__ int s_n;
  for (int i = threadIdx.x; i < PK_CAP; i += PK_THREADS) s_keys[i] = 0ull;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const long long n = (long long)nx * ny * nt;
  for (long long base = (long long)blockIdx.x * PK_THREADS; base < n; base += (long long)gridDim.x * PK_THREADS) {   // (per workgroup: barriers inside)
    const long long idx = base + threadIdx.x;
    unsigned long long key = 0ull;
    if (idx < n) {
      const unsigned int sc = scores[idx];
      if (sc > 0u) {
        const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), k = (int)(idx / ((long long)nx * ny));
        bool peak = true;
        for (int dk = -1; dk <= 1 && peak; dk++) {
          int kk = k + dk;
          if (kk < 0 || kk >= nt) { if (!wraps) continue; kk = kk < 0 ? nt - 1 : 0; }
          for (int dy = -1; dy <= 1 && peak; dy++) {
            const int yy = iy + dy;
            if (yy < 0 || yy >= ny) continue;
            for (int dx = -1; dx <= 1; dx++) {
              const int xx = ix + dx;
              if (xx < 0 || xx >= nx) continue;
              const long long nidx = ((long long)kk * ny + yy) * nx + xx;
              if (nidx == idx) continue;                      // (itself, directly or through the wrap of a one-rotation lattice)
              const unsigned int sn = scores[nidx];
              if (!(sc > sn || (sc == sn && idx < nidx))) { peak = false; break; }
            }
          }
        }
        if (peak) key = peak_key(sc, (unsigned int)idx);
      }
    }
    pk_round(s_keys, &s_n, key);
  }
  pk_sort(s_keys);
  for (int i = threadIdx.x; i < PK_KEEP; i += PK_THREADS) wg_keys[(size_t)blockIdx.x * PK_KEEP + i] = s_keys[i];
}

// one workgroup: the K best of the n_keys keys the workgroups left (0 = no key), and how many there are (<= K)
__global__ void __launch_bounds__(PK_THREADS)
k_reloc_peaks_merge(const unsigned long long* __restrict__ wg_keys, int n_keys, int K, unsigned long long* __restrict__ out /* [PK_KEEP + 1] */)
{
  __shared__ unsigned long long s_keys[PK_CAP];
  __shared__ int s_n;
  for (int i = threadIdx.x; i < PK_CAP; i += PK_THREADS) s_keys[i] = 0ull;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  for (int base = 0; base < n_keys; base += PK_THREADS) {
    const int i = base + (int)threadIdx.x;
    pk_round(s_keys, &s_n, i < n_keys ? wg_keys[i] : 0ull);
  }
  pk_sort(s_keys);
  if ((int)threadIdx.x < PK_KEEP) out[threadIdx.x] = (int)threadIdx.x < K ? s_keys[threadIdx.x] : 0ull;
  if (threadIdx.x == 0) {
    int cnt = 0;
    for (int i = 0; i < K; i++) cnt += s_keys[i] != 0ull;
    out[PK_KEEP] = (unsigned long long)cnt;
  }
}

void reloc_free(tsd_ctx* ctx)
{
  tsd_ctx::Reloc& r = ctx->reloc;
  hipFree(r.d_points); hipFree(r.d_cos_sin); hipFree(r.volume.d); hipFree(r.d_keys);
  if (r.h_keys) hipHostFree(r.h_keys);
  r = tsd_ctx::Reloc{};
}

void ScoreVolume::drop() { hipFree(d); *this = ScoreVolume{}; }
ScoreVolume::GiveBack::~GiveBack() { if (v.cap > RELOC_KEEP_CANDIDATES) v.drop(); }

int ScoreVolume::ensure(tsd_ctx* ctx, size_t candidates)
{
  if (candidates > cap) {
    drop();
    TSD_HIP_CHECK(ctx, hipMalloc(&d, sizeof(uint32_t) * candidates));
    cap = candidates;
  }
  return TSD_OK;
}

int ScoreVolume::copy_out(tsd_ctx* ctx, uint32_t* scores, int room) const
{
  const long long n = (long long)nx * ny * ntheta;
  const long long m = std::min<long long>(n, room > 0 ? room : 0);
  if (m > 0 && scores) {
    TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    TSD_HIP_CHECK(ctx, hipMemcpyAsync(scores, d, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return (int)n;
}

int reloc_ensure(tsd_ctx* ctx, size_t rotations)
{
  tsd_ctx::Reloc& r = ctx->reloc;
  if (!r.d_points) TSD_HIP_CHECK(ctx, hipMalloc(&r.d_points, sizeof(double) * 2 * TSD_MAX_ICP_POINTS));
  if (!r.d_keys) TSD_HIP_CHECK(ctx, hipMalloc(&r.d_keys, sizeof(unsigned long long) * ((size_t)(RELOC_PEAK_GRID + 1) * PK_KEEP + 1)));
  if (!r.h_keys) TSD_HIP_CHECK(ctx, hipHostMalloc(&r.h_keys, sizeof(unsigned long long) * (PK_KEEP + 1), hipHostMallocDefault));
  if (rotations > r.rot_cap) {
    hipFree(r.d_cos_sin); r.d_cos_sin = nullptr; r.rot_cap = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&r.d_cos_sin, sizeof(double) * 2 * rotations));
    r.rot_cap = rotations;
  }
  return TSD_OK;
}

// the two peak kernels on the context's stream over a volume on the device; the merged keys and their count arrive in r.h_keys
static int launch_reloc_peaks(tsd_ctx* ctx, const uint32_t* d_scores, int nx, int ny, int nt, int wraps, int K)
{
  tsd_ctx::Reloc& r = ctx->reloc;
  const long long n = (long long)nx * ny * nt;
  const int blocks = (int)std::min<long long>((n + PK_THREADS - 1) / PK_THREADS, RELOC_PEAK_GRID);
  unsigned long long* merged = r.d_keys + (size_t)RELOC_PEAK_GRID * PK_KEEP;
  hipLaunchKernelGGL(k_reloc_peaks, dim3(blocks), dim3(PK_THREADS), 0, ctx->stream, d_scores, nx, ny, nt, wraps, r.d_keys);
  hipLaunchKernelGGL(k_reloc_peaks_merge, dim3(1), dim3(PK_THREADS), 0, ctx->stream, (const unsigned long long*)r.d_keys, blocks * PK_KEEP, K, merged);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(r.h_keys, merged, sizeof(unsigned long long) * (PK_KEEP + 1), hipMemcpyDeviceToHost, ctx->stream));
  return TSD_OK;
}

const unsigned long long* reloc_merged_keys(const tsd_ctx* ctx) { return ctx->reloc.d_keys + (size_t)RELOC_PEAK_GRID * PK_KEEP; }

// how a lattice of nx * ny positions and nt rotations is cut into workgroups of RELOC_WAVES waves: (rotations per workgroup, grid.y)
static void reloc_cut(int nx, int ny, int nt, int& rot_per_block, int& blocks_y)
{
  const long long positions = (long long)nx * ny;
  long long cuts = (RELOC_MIN_BLOCKS + positions - 1) / positions;                 // along the rotations, whole rounds of RELOC_WAVES at least
  cuts = std::max<long long>(1, std::min<long long>(cuts, (nt + RELOC_WAVES - 1) / RELOC_WAVES));
  cuts = std::min<long long>(cuts, 65535);
  rot_per_block = (int)((nt + cuts - 1) / cuts);
  blocks_y = (nt + rot_per_block - 1) / rot_per_block;
}

int launch_lattice_search(tsd_ctx* ctx, ScoreVolume& vol, const LatticeSpec& lat, bool gate, const double* d_pts, int P, int stride,
                          double pvx, double pvy)
{
  const RelocLattice& L = lat.L;
  int rot_per_block = 0, blocks_y = 0;
  reloc_cut(L.nx, L.ny, L.ntheta, rot_per_block, blocks_y);
  const dim3 grid((unsigned)((long long)L.nx * L.ny), (unsigned)blocks_y), block(64 * RELOC_WAVES);
  const size_t lds = sizeof(double) * 2 * (size_t)P;                    // the staged points
  const double* table = ctx->reloc.d_cos_sin;
  if (gate) hipLaunchKernelGGL(k_reloc_score, grid, block, lds, ctx->stream, ctx->grid, L, d_pts, P, table, vol.d, rot_per_block);
  else hipLaunchKernelGGL(k_align_score, grid, block, lds, ctx->stream, ctx->grid, L, d_pts, P, stride, pvx, pvy, table, vol.d, rot_per_block);
  vol.nx = L.nx; vol.ny = L.ny; vol.ntheta = L.ntheta;
  return launch_reloc_peaks(ctx, vol.d, L.nx, L.ny, L.ntheta, lat.theta_wraps, lat.K);
}

static bool reloc_lattice_ok(int nx, int ny, int nt) { return nx >= 1 && ny >= 1 && nt >= 1; }
static bool reloc_lattice_fits(int nx, int ny, int nt) { return (long long)nx * ny <= TSD_RELOC_MAX_CANDIDATES && (long long)nx * ny * nt <= TSD_RELOC_MAX_CANDIDATES; }

double reloc_reach(const GridDev& g) { return (double)TSD_RELOC_MAX_REACH * ((double)g.N * g.cs); }
static bool reloc_lattice_near(const GridDev& g, double a0, int n, double step)
{
  const double a1 = a0 + (double)(n - 1) * step;
  return a0 >= -reloc_reach(g) && a1 <= (double)g.N * g.cs + reloc_reach(g);
}

int lattice_check(tsd_ctx* ctx, const LatticeSpec& lat, const char* who)
{
  const RelocLattice& L = lat.L;
  if (!reloc_lattice_ok(L.nx, L.ny, L.ntheta)) return refuse(ctx, who, TSD_E_ARG, "nx, ny, ntheta must be >= 1");
  if (!std::isfinite(L.x0) || !std::isfinite(L.y0) || !std::isfinite(L.step) || !(L.step > 0.0))
    return refuse(ctx, who, TSD_E_ARG, "x0, y0 finite and step_xy > 0");
  if (!reloc_lattice_fits(L.nx, L.ny, L.ntheta)) return refuse(ctx, who, TSD_E_CAPACITY, "nx * ny * ntheta > TSD_RELOC_MAX_CANDIDATES");
  if (!reloc_lattice_near(ctx->grid, L.x0, L.nx, L.step) || !reloc_lattice_near(ctx->grid, L.y0, L.ny, L.step))
    return refuse(ctx, who, TSD_E_ARG, "the lattice reaches further than TSD_RELOC_MAX_REACH grid widths from the grid");
  if (!lat.cos_sin && (!std::isfinite(lat.theta0) || !std::isfinite(lat.dtheta) || lat.dtheta == 0.0))
    return refuse(ctx, who, TSD_E_ARG, "without a cos_sin table, theta0 and a non-zero dtheta are needed");
  return TSD_OK;
}

bool lattice_table(const LatticeSpec& lat, std::vector<double>& table)
{
  table.resize((size_t)2 * lat.L.ntheta);
  for (int k = 0; k < lat.L.ntheta; k++) {
    if (lat.cos_sin) { table[2 * k] = lat.cos_sin[2 * k]; table[2 * k + 1] = lat.cos_sin[2 * k + 1]; }
    else { const double th = lat.theta0 + (double)k * lat.dtheta; table[2 * k] = std::cos(th); table[2 * k + 1] = std::sin(th); }
    if (!std::isfinite(table[2 * k]) || !std::isfinite(table[2 * k + 1])) return false;
  }
  return true;
}

bool points_in_reach(const GridDev& g, const double* points_xy, int n)
{
  for (int i = 0; i < 2 * n; i++)
    if (!(std::fabs(points_xy[i]) <= reloc_reach(g))) return false;      // (NaN fails too)
  return true;
}

bool reloc_scan_in_flight(const tsd_ctx* ctx)
{
  for (const tsd_sensor* s : ctx->sensors) if (s->ledger.in_flight()) return true;
  for (const tsd_batch* b : ctx->batches) if (b->n > 0) return true;
  return false;
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_relocalize(tsd_ctx* ctx, const tsd_reloc_params* prm, const double* points_xy, int P, const double* rays_local_2xB,
                   const double* ranges, const uint8_t* mask, int beams, double min_range, double max_range,
                   const tsd_icp_params* icp_params, tsd_reloc_result* result)
{
  if (!ctx || !prm || !points_xy || !rays_local_2xB || !ranges || !mask || !icp_params || !result) return TSD_E_ARG;
  if (P < 1) return set_error(ctx, TSD_E_ARG, "tsd_relocalize: no scan point", hipSuccess);
  if (P > TSD_MAX_ICP_POINTS) return set_error(ctx, TSD_E_CAPACITY, "tsd_relocalize: points > TSD_MAX_ICP_POINTS", hipSuccess);
  if (beams < 1 || beams > TSD_MAX_BEAMS || beams > TSD_MAX_ICP_POINTS)
    return set_error(ctx, TSD_E_CAPACITY, "tsd_relocalize: beams out of range for the registration", hipSuccess);
  if (prm->K < 1 || prm->K > TSD_RELOC_MAX_PEAKS) return set_error(ctx, TSD_E_ARG, "tsd_relocalize: K outside 1 .. TSD_RELOC_MAX_PEAKS", hipSuccess);
  if (prm->min_pairs < 0) return set_error(ctx, TSD_E_ARG, "tsd_relocalize: min_pairs < 0", hipSuccess);
  const LatticeSpec lat = lattice_spec(*prm);
  if (int rc = lattice_check(ctx, lat, "tsd_relocalize")) return rc;
  if (!points_in_reach(ctx->grid, points_xy, P))
    return set_error(ctx, TSD_E_ARG, "tsd_relocalize: a scan point is not finite or further than TSD_RELOC_MAX_REACH grid widths from the sensor", hipSuccess);
  std::vector<double> table;
  if (!lattice_table(lat, table)) return set_error(ctx, TSD_E_ARG, "tsd_relocalize: cos_sin is not finite", hipSuccess);
  if (reloc_scan_in_flight(ctx)) return set_error(ctx, TSD_E_ARG, "tsd_relocalize: a scan of this context is in flight (collect it first)", hipSuccess);
  // ---- the arguments stand: from here on the context changes ----
  if (int rc = enter(ctx)) return rc;
  ctx->ledger.outputs_overwritten();      // (the refinement rewrites the context's ray-cast outputs, like tsd_localize)
  tsd_ctx::Reloc& r = ctx->reloc;
  ScoreVolume::GiveBack give_back{r.volume};
  if (int rc = reloc_ensure(ctx, (size_t)lat.L.ntheta)) return rc;
  if (int rc = r.volume.ensure(ctx, (size_t)lat.L.nx * (size_t)lat.L.ny * (size_t)lat.L.ntheta)) return rc;
  std::memset(result, 0, sizeof(*result));
  StageEvents stages;                     // 0 .. 1 the search, 2 .. 3 the refinement
  if (int rc = stages.open(ctx, 4, "tsd_relocalize")) return rc;

  // ---- search ----
  // (the sources stay valid until the wait behind the search)
  hipError_t e = hipMemcpyAsync(r.d_points, points_xy, sizeof(double) * 2 * (size_t)P, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(r.d_cos_sin, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, "tsd_relocalize: copy of the points", e);
  stages.record(0);
  int rc = launch_lattice_search(ctx, r.volume, lat, true, r.d_points, P, 1, 0.0, 0.0);
  stages.record(1);
  if (rc == TSD_OK && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = set_error(ctx, TSD_E_HIP, "tsd_relocalize: search", e);
  if (rc != TSD_OK) return rc;
  const int n_peaks = (int)r.h_keys[PK_KEEP];
  Peak pk[TSD_RELOC_MAX_PEAKS];
  for (int j = 0; j < n_peaks; j++) pk[j] = peak_of(r.h_keys[j]);

  // ---- refinement: the unfused localisation from every peak, in the peaks' order; strictly more pairs win (IcpMultiInitIterator.cpp:26-38) ----
  const double nan = std::nan("");
  result->n_peaks = n_peaks; result->winner_idx = -1;
  for (double& v : result->pose33) v = nan;
  result->coarse_x = result->coarse_y = result->coarse_cos = result->coarse_sin = nan;
  const size_t nb = (size_t)beams;
  const double cs = ctx->grid.cs;
  std::vector<double> rays_world(2 * nb);
  int best = -1; tsd_icp_result best_icp{}; double best_pose[9] = {0};
  stages.record(2);
  for (int j = 0; j < n_peaks; j++) {
    const LatticePose at = lattice_pose(lat.L, table.data(), pk[j].idx);
    const double c = at.c, s = at.s, ms = -s;
    const double pose[9] = {c, ms, at.x, s, c, at.y, 0.0, 0.0, 1.0};
    for (size_t i = 0; i < nb; i++) {
      const double x = rays_local_2xB[i], y = rays_local_2xB[nb + i];
      double wx = 0.0, wy = 0.0;                               // Sensor::transform (Sensor.cpp:50-55)
      wx += c * x; wx += ms * y;
      wy += s * x; wy += c * y;
      if (cs != 1.0) { wx *= (cs / 1.0); wy *= (cs / 1.0); }   // Sensor::getNormalizedRayMap (Sensor.cpp:36-48), _rayNorm = 1
      rays_world[i] = wx; rays_world[nb + i] = wy;
    }
    tsd_icp_result ir;
    rc = tsd_localize(ctx, pose, rays_world.data(), rays_local_2xB, ranges, mask, beams, min_range, max_range, icp_params, &ir);
    if (rc != TSD_OK) break;
    result->n_refined++;
    if (best < 0 || ir.pairs > best_icp.pairs) { best = j; best_icp = ir; std::memcpy(best_pose, pose, sizeof(pose)); }
  }
  stages.record(3);
  stages.measure(0, 1, result->search_ms);
  stages.measure(2, 3, result->refine_ms);
  if (rc != TSD_OK) return rc;
  if (best >= 0) {
    result->winner_idx = (int32_t)pk[best].idx; result->winner_score = pk[best].score;
    result->coarse_x = best_pose[2]; result->coarse_y = best_pose[5]; result->coarse_cos = best_pose[0]; result->coarse_sin = best_pose[3];
    result->icp = best_icp;
    result->found = best_icp.pairs >= prm->min_pairs ? 1 : 0;
    if (result->found)
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {                           // pose = coarse * T (3 x 3 product, k ascending from 0.0)
          double t = 0.0;
          for (int q = 0; q < 3; q++) t += best_pose[3 * i + q] * best_icp.T[3 * q + j];
          result->pose33[3 * i + j] = t;
        }
  }
  return TSD_OK;
}

int tsd_debug_reloc_scores(tsd_ctx* ctx, uint32_t* scores, int cap)
{
  return ctx ? ctx->reloc.volume.copy_out(ctx, scores, cap) : TSD_E_ARG;
}

int tsd_debug_reloc_peaks(tsd_ctx* ctx, const uint32_t* scores, int nx, int ny, int ntheta, int theta_wraps, int K,
                          int32_t* idx_out, uint32_t* score_out, int* n_out)
{
  if (!ctx || !scores || !idx_out || !score_out || !n_out) return TSD_E_ARG;
  if (!reloc_lattice_ok(nx, ny, ntheta) || K < 1 || K > TSD_RELOC_MAX_PEAKS) return set_error(ctx, TSD_E_ARG, "tsd_debug_reloc_peaks: shape or K", hipSuccess);
  if (!reloc_lattice_fits(nx, ny, ntheta)) return set_error(ctx, TSD_E_CAPACITY, "tsd_debug_reloc_peaks: volume > TSD_RELOC_MAX_CANDIDATES", hipSuccess);
  if (reloc_scan_in_flight(ctx)) return set_error(ctx, TSD_E_ARG, "tsd_debug_reloc_peaks: a scan of this context is in flight (collect it first)", hipSuccess);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (int rc = reloc_ensure(ctx, 0)) return rc;
  const size_t n = (size_t)nx * (size_t)ny * (size_t)ntheta;
  uint32_t* d_vol = nullptr;
  TSD_HIP_CHECK(ctx, hipMalloc(&d_vol, sizeof(uint32_t) * n));
  int rc = TSD_OK;
  hipError_t e = hipMemcpyAsync(d_vol, scores, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) rc = launch_reloc_peaks(ctx, d_vol, nx, ny, ntheta, theta_wraps ? 1 : 0, K);
  if (e == hipSuccess && rc == TSD_OK) e = hipStreamSynchronize(ctx->stream);
  hipFree(d_vol);
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, "tsd_debug_reloc_peaks", e);
  if (rc != TSD_OK) return rc;
  const tsd_ctx::Reloc& r = ctx->reloc;
  *n_out = (int)r.h_keys[PK_KEEP];
  for (int j = 0; j < *n_out; j++) {
    const Peak pk = peak_of(r.h_keys[j]);
    score_out[j] = pk.score; idx_out[j] = (int32_t)pk.idx;
  }
  return TSD_OK;
}

}  // extern "C"
