// align.hip -- map-to-map alignment: which rigid transform carries a list of surface points (another robot's map, tsd_surface_*) into
// this grid?  (tsd_align_points / tsd_map_align, include/tsd_hip.h)  The first reader of the surface list.
//
//   k_align_stage    the list's way into the context: p + add (the half-cell offset between calcCoords' list and the field the look-ups
//                    read, for tsd_map_align), and the count of coordinates that are not finite or out of reach
//   k_align_score    k_reloc_score's sum over the coarse points (every stride-th, minus the pivot, read from the device list), without the
//                    free-space gate: reloc_shared.hpp's lattice_score<false>, the body both score kernels run
//   (peaks)          reloc.hip's k_reloc_peaks / k_reloc_peaks_merge, launched with the score kernel by launch_lattice_search
//   k_align_refine   point-to-TSD Gauss-Newton: ONE persistent workgroup per peak, all K peaks in one launch; its threads stride over all
//                    n points every iteration, the 11 sums are reduced inside the workgroup in a fixed order (per thread in index order,
//                    shuffle tree per wave, waves in order: no floating-point atomics), one lane solves the 3 x 3 system and steps the
//                    state -- no kernel boundary and no exchange between workgroups, k_icp's reasoning.  It decodes its
//                    start pose from the merged peak keys on the device: the host waits once per call.
//
// Shape of k_align_refine: a divergent gather of 25 reads per point (five look-ups: the value and interpolate_normal's four, a tile flag
// and four cells each).  All 25 are requested before the first is used (tsd_device.hpp's lookup_issue: not behind the flag tests).
//
// The lattice's refusals, the rotation table, the score volume, the launch of the search and the decoding of a peak key are the
// relocalisation's, through reloc_shared.hpp; this file keeps what is the alignment's own.
#include "reloc_shared.hpp"

namespace tsd {

constexpr int ALIGN_THREADS = 512;         // k_align_refine's workgroup: 8 waves
constexpr int ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr int ALIGN_SUMS = 11;             // A00 A01 A02 A11 A12 A22 | b0 b1 b2 | sum w | sum w r^2
constexpr int ALIGN_DEBUG_SLOT = TSD_RELOC_MAX_PEAKS;   // the record tsd_debug_align_sums uses

__global__ void __launch_bounds__(256)
k_align_stage(const double* __restrict__ in, double* __restrict__ out, int n, double add, double reach, unsigned int* __restrict__ bad)
{
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const double x = in[2 * (size_t)i], y = in[2 * (size_t)i + 1];
  if (!(fabs(x) <= reach) || !(fabs(y) <= reach)) atomicAdd(bad, 1u);     // (NaN fails too)
  if (out) { out[2 * (size_t)i] = x + add; out[2 * (size_t)i + 1] = y + add; }
}

__global__ void __launch_bounds__(64 * RELOC_WAVES)
k_align_score(GridDev g, RelocLattice L, const double* __restrict__ pts, int P, int stride, double pvx, double pvy,
              const double* __restrict__ cos_sin, uint32_t* __restrict__ scores, int rot_per_block)
{
  lattice_score<false>(g, L, pts, P, stride, pvx, pvy, cos_sin, scores, rot_per_block);
}

struct AlignRefineArgs {
  const double* pts; int n; int iterations;
  double pvx, pvy, v_cut, eps, lever;
  const unsigned long long* keys;          // merged peak keys (workgroup j refines key j), or nullptr: `start`
  RelocLattice L; const double* cos_sin;   // to decode a key
  double start[4];                         // m.x m.y c s
  tsd_align_peak* rec;                     // [gridDim.x]
};

// this thread's share of one accumulation at the state (mx, my, c, s): points tid, tid + ALIGN_THREADS, .. in that order
__device__ __forceinline__ void align_accumulate(const GridDev& g, const AlignRefineArgs& a, double mx, double my, double c, double s,
                                                 double acc[ALIGN_SUMS], int& n_ok)
{
#pragma unroll
  for (int t = 0; t < ALIGN_SUMS; t++) acc[t] = 0.0;
  n_ok = 0;
  for (int i = (int)threadIdx.x; i < a.n; i += ALIGN_THREADS) {
    const double px = a.pts[2 * (size_t)i] - a.pvx, py = a.pts[2 * (size_t)i + 1] - a.pvy;
    const double qx = (c * px - s * py) + mx;
    const double qy = (s * px + c * py) + my;
    // the value's look-up and the normal's four: 5 flag reads and 20 cell reads requested together
    const Lookup at = lookup_issue(g, qx, qy);
    double nx, ny, v;
    const bool okn = interpolate_normal(g, qx, qy, nx, ny);
    const bool okv = lookup_value(at, v);
    // (interpolate_normal normalises exactly when the length is > 10e-6: a normalised normal has length 1, any other at most 10e-6)
    const bool ok = okv && okn && (nx * nx + ny * ny > 0.25);
    if (ok) {
      n_ok++;
      const double u = v / a.v_cut;
      if (fabs(u) < 1.0) {
        const double h = 1.0 - u * u, w = h * h;
        const double r = v * g.max_trunc;
        const double jt = nx * (-(qy - my)) + ny * (qx - mx);
        const double wjx = w * nx, wjy = w * ny, wjt = w * jt;
        acc[0] += wjx * nx; acc[1] += wjx * ny; acc[2] += wjx * jt;
        acc[3] += wjy * ny; acc[4] += wjy * jt; acc[5] += wjt * jt;
        acc[6] += -(wjx * r); acc[7] += -(wjy * r); acc[8] += -(wjt * r);
        acc[9] += w; acc[10] += (w * r) * r;
      }
    }
  }
}

__global__ void __launch_bounds__(ALIGN_THREADS)
k_align_refine(GridDev g, const AlignRefineArgs a)
{
  __shared__ double s_part[ALIGN_WAVES][ALIGN_SUMS];
  __shared__ int s_nok[ALIGN_WAVES];
  __shared__ double s_state[4];            // m.x m.y c s
  __shared__ int s_stop;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  tsd_align_peak* rec = a.rec + blockIdx.x;
  int idx = -1; unsigned int score = 0u;
  double mx = a.start[0], my = a.start[1], c = a.start[2], s = a.start[3];
  if (a.keys) {                            // (uniform)
    const unsigned long long key = a.keys[blockIdx.x];
    if (key == 0ull) return;               // fewer peaks than workgroups
    const Peak pk = peak_of(key);
    const LatticePose at = lattice_pose(a.L, a.cos_sin, pk.idx);
    score = pk.score; idx = (int)pk.idx;
    mx = at.x; my = at.y; c = at.c; s = at.s;
  }
  // thread 0's: the step control
  double gain = 1.0, pdx = 0.0, pdy = 0.0, pdt = 0.0;
  bool converged = false;
  for (int it = 0; ; it++) {
    double acc[ALIGN_SUMS]; int n_ok;
    align_accumulate(g, a, mx, my, c, s, acc, n_ok);
#pragma unroll
    for (int t = 0; t < ALIGN_SUMS; t++) acc[t] = wave_sum(acc[t]);
    n_ok = wave_sum_i(n_ok);
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < ALIGN_SUMS; t++) s_part[wave][t] = acc[t];
      s_nok[wave] = n_ok;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double S[ALIGN_SUMS]; int nok = 0;
#pragma unroll
      for (int t = 0; t < ALIGN_SUMS; t++) S[t] = 0.0;
      for (int w = 0; w < ALIGN_WAVES; w++) {                   // waves in order
#pragma unroll
        for (int t = 0; t < ALIGN_SUMS; t++) S[t] += s_part[w][t];
        nok += s_nok[w];
      }
      int status = -1;                                          // -1: step on
      if (nok < 3) status = TSD_ALIGN_DEGENERATE;
      else if (converged) status = TSD_ALIGN_CONVERGED;
      else if (it >= a.iterations) status = TSD_ALIGN_MAXITER;
      double ddx = 0.0, ddy = 0.0, ddt = 0.0;
      if (status < 0) {
        // LDL^T of the symmetric A without pivoting, fp64 in the written order
        const double d0 = S[0];
        const double l10 = S[1] / d0, l20 = S[2] / d0;
        const double d1 = S[3] - l10 * S[1];
        const double t21 = S[4] - l20 * S[1];
        const double l21 = t21 / d1;
        const double d2 = (S[5] - l20 * S[2]) - l21 * t21;
        if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) status = TSD_ALIGN_DEGENERATE;
        else {
          const double y0 = S[6], y1 = S[7] - l10 * y0, y2 = (S[8] - l20 * y0) - l21 * y1;
          ddt = y2 / d2;
          ddy = y1 / d1 - l21 * ddt;
          ddx = (y0 / d0 - l10 * ddy) - l20 * ddt;
        }
      }
      if (status < 0) {
        const double dot = (ddx * pdx + ddy * pdy) + (a.lever * a.lever) * (ddt * pdt);
        if (dot < 0.0) gain = fmax(gain * 0.5, 0.0625);
        ddx *= gain; ddy *= gain; ddt *= gain;
        pdx = ddx; pdy = ddy; pdt = ddt;
        const double h = hypot(1.0, ddt), rc = 1.0 / h, rs = ddt / h;
        const double c2 = c * rc - s * rs, s2 = s * rc + c * rs, hh = hypot(c2, s2);
        s_state[0] = mx + ddx; s_state[1] = my + ddy; s_state[2] = c2 / hh; s_state[3] = s2 / hh;
        converged = hypot(ddx, ddy) < a.eps && a.lever * fabs(ddt) < a.eps;
      } else {
        rec->idx = idx; rec->score = score; rec->status = status; rec->iterations = it; rec->n_ok = nok; rec->reserved = 0;
        rec->m[0] = mx; rec->m[1] = my; rec->c = c; rec->s = s; rec->gain = gain;
        for (int t = 0; t < ALIGN_SUMS; t++) rec->sums[t] = S[t];
      }
      s_stop = status >= 0 ? 1 : 0;
    }
    __syncthreads();
    if (s_stop) break;                                           // (uniform)
    mx = s_state[0]; my = s_state[1]; c = s_state[2]; s = s_state[3];
    // (the next round's barrier after the sums stands between these reads and thread 0's next write)
  }
}

void align_free(tsd_ctx* ctx)
{
  tsd_ctx::Align& al = ctx->align;
  hipFree(al.d_pts); hipFree(al.volume.d); hipFree(al.d_rec); hipFree(al.d_bad);
  if (al.h_rec) hipHostFree(al.h_rec);
  if (al.h_bad) hipHostFree(al.h_bad);
  al = tsd_ctx::Align{};
}

static int align_ensure(tsd_ctx* ctx, size_t points)
{
  tsd_ctx::Align& al = ctx->align;
  if (!al.d_rec) TSD_HIP_CHECK(ctx, hipMalloc(&al.d_rec, sizeof(tsd_align_peak) * (TSD_RELOC_MAX_PEAKS + 1)));
  if (!al.h_rec) TSD_HIP_CHECK(ctx, hipHostMalloc(reinterpret_cast<void**>(&al.h_rec), sizeof(tsd_align_peak) * (TSD_RELOC_MAX_PEAKS + 1), hipHostMallocDefault));
  if (!al.d_bad) TSD_HIP_CHECK(ctx, hipMalloc(&al.d_bad, sizeof(unsigned int)));
  if (!al.h_bad) TSD_HIP_CHECK(ctx, hipHostMalloc(reinterpret_cast<void**>(&al.h_bad), sizeof(unsigned int), hipHostMallocDefault));
  if (points > al.pts_cap) {
    const size_t cap = std::max<size_t>({points, 2 * al.pts_cap, 1024});
    hipFree(al.d_pts); al.d_pts = nullptr; al.pts_cap = 0;
    TSD_HIP_CHECK(ctx, hipMalloc(&al.d_pts, sizeof(double) * 2 * cap));
    al.pts_cap = cap;
  }
  return TSD_OK;
}

static double align_v_cut(const tsd_align_params* p) { return p->v_cut == 0.0 ? 0.75 : p->v_cut; }
static double align_eps(const tsd_align_params* p) { return p->eps == 0.0 ? 1e-6 : p->eps; }

// everything of the parameters that can be checked without the points, and the call's rotation table; `who` names the entry point in
// the message
static int align_check_params(tsd_ctx* ctx, const tsd_align_params* prm, bool pivot_may_be_nan, const char* who, std::vector<double>& table)
{
  auto refuse = [&](int code, const char* what) { return tsd::refuse(ctx, who, code, what); };
  if (prm->K < 1 || prm->K > TSD_RELOC_MAX_PEAKS) return refuse(TSD_E_ARG, "K outside 1 .. TSD_RELOC_MAX_PEAKS");
  if (prm->iterations < 0 || prm->iterations > 64) return refuse(TSD_E_ARG, "iterations outside 0 .. 64");
  const LatticeSpec lat = lattice_spec(*prm);
  if (int rc = lattice_check(ctx, lat, who)) return rc;
  if (!lattice_table(lat, table)) return refuse(TSD_E_ARG, "cos_sin is not finite");
  const bool pivot_nan = std::isnan(prm->pivot_x) && std::isnan(prm->pivot_y);
  if (!(pivot_may_be_nan && pivot_nan) && (!(std::fabs(prm->pivot_x) <= reloc_reach(ctx->grid)) || !(std::fabs(prm->pivot_y) <= reloc_reach(ctx->grid))))
    return refuse(TSD_E_ARG, "the pivot is not finite or further than TSD_RELOC_MAX_REACH grid widths away");
  if (!(align_v_cut(prm) > 0.0 && align_v_cut(prm) <= 1.0)) return refuse(TSD_E_ARG, "v_cut outside (0, 1]");
  if (!(align_eps(prm) > 0.0) || !std::isfinite(prm->eps)) return refuse(TSD_E_ARG, "eps must be > 0");
  if (!std::isfinite(prm->lever)) return refuse(TSD_E_ARG, "lever is not finite");
  if (std::isnan(prm->min_overlap) || std::isnan(prm->max_rms)) return refuse(TSD_E_ARG, "min_overlap / max_rms is NaN");
  return TSD_OK;
}

static void align_clear_result(tsd_align_result* out)
{
  std::memset(out, 0, sizeof(*out));
  const double nan = std::nan("");
  out->winner_idx = -1;
  for (double& v : out->T33) v = nan;
  out->coarse_x = out->coarse_y = out->coarse_cos = out->coarse_sin = nan;
  out->cell_error = nan;
}

// the whole alignment; the arguments have been checked and `table` is theirs.  src_cells: the side of the grid the points come from,
// for cell_error
static int align_run(tsd_ctx* ctx, const tsd_align_params* prm, const std::vector<double>& table, const double* points_xy, int n,
                     bool on_device, int src_cells, tsd_align_result* out)
{
  const LatticeSpec lat = lattice_spec(*prm);
  const RelocLattice& L = lat.L;
  if (int rc = enter(ctx)) return rc;
  tsd_ctx::Align& al = ctx->align;
  al.n_rec = 0;
  ScoreVolume::GiveBack give_back{al.volume};
  if (int rc = reloc_ensure(ctx, (size_t)L.ntheta)) return rc;
  if (int rc = align_ensure(ctx, on_device ? 0 : (size_t)n)) return rc;
  if (int rc = al.volume.ensure(ctx, (size_t)L.nx * (size_t)L.ny * (size_t)L.ntheta)) return rc;
  tsd_ctx::Reloc& r = ctx->reloc;
  align_clear_result(out);
  StageEvents stages;                      // 0 .. 1 the search, 1 .. 2 the refinement
  if (int rc = stages.open(ctx, 3, "tsd_align_points")) return rc;
  const double* d_pts = points_xy;
  hipError_t e = hipMemsetAsync(al.d_bad, 0, sizeof(unsigned int), ctx->stream);
  if (!on_device) {                        // (checked on the host already; the source stays valid until the wait)
    if (e == hipSuccess) e = hipMemcpyAsync(al.d_pts, points_xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    d_pts = al.d_pts;
  } else
    hipLaunchKernelGGL(k_align_stage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, points_xy, (double*)nullptr, n, 0.0,
                       reloc_reach(ctx->grid), al.d_bad);
  if (e == hipSuccess) e = hipMemcpyAsync(r.d_cos_sin, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, "tsd_align_points: copy of the points", e);
  // ---- search ----
  const int stride = (n + TSD_MAX_ICP_POINTS - 1) / TSD_MAX_ICP_POINTS;
  const int P = (n + stride - 1) / stride;
  stages.record(0);
  int rc = launch_lattice_search(ctx, al.volume, lat, false, d_pts, P, stride, prm->pivot_x, prm->pivot_y);
  stages.record(1);
  // ---- refinement: every peak in one launch, the start poses decoded from the merged keys on the device ----
  const double lever = prm->lever > 0.0 ? prm->lever : 0.5 * ((double)ctx->grid.N * ctx->grid.cs);
  if (rc == TSD_OK) {
    AlignRefineArgs a{};
    a.pts = d_pts; a.n = n; a.iterations = prm->iterations;
    a.pvx = prm->pivot_x; a.pvy = prm->pivot_y; a.v_cut = align_v_cut(prm); a.eps = align_eps(prm); a.lever = lever;
    a.keys = reloc_merged_keys(ctx); a.L = L; a.cos_sin = r.d_cos_sin; a.rec = al.d_rec;
    hipLaunchKernelGGL(k_align_refine, dim3((unsigned)prm->K), dim3(ALIGN_THREADS), 0, ctx->stream, ctx->grid, a);
    e = hipGetLastError();
    stages.record(2);
    if (e == hipSuccess) e = hipMemcpyAsync(al.h_rec, al.d_rec, sizeof(tsd_align_peak) * (size_t)prm->K, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(al.h_bad, al.d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // the one wait of the call
    if (e != hipSuccess) rc = set_error(ctx, TSD_E_HIP, "tsd_align_points: search and refinement", e);
  }
  if (rc != TSD_OK) return rc;
  stages.measure(0, 1, out->search_ms);
  stages.measure(1, 2, out->refine_ms);
  if (*al.h_bad != 0u)
    return set_error(ctx, TSD_E_ARG, "tsd_align_points: a point is not finite or further than TSD_RELOC_MAX_REACH grid widths away", hipSuccess);
  const int n_peaks = (int)r.h_keys[PK_KEEP];
  al.n_rec = n_peaks;
  out->n_peaks = n_peaks; out->n_refined = n_peaks; out->n = n; out->stride = stride;
  // ---- the winner: the largest sum w among the peaks that are not degenerate, the earlier peak keeps a tie ----
  int best = -1;
  for (int j = 0; j < n_peaks; j++) {
    const tsd_align_peak& p = al.h_rec[j];
    if (p.status == TSD_ALIGN_DEGENERATE) continue;
    if (best < 0 || p.sums[9] > al.h_rec[best].sums[9]) best = j;
  }
  if (best < 0) return TSD_OK;
  const tsd_align_peak& w = al.h_rec[best];
  const LatticePose coarse = lattice_pose(L, table.data(), (unsigned int)w.idx);
  out->winner_idx = w.idx; out->winner_score = w.score;
  out->coarse_x = coarse.x; out->coarse_y = coarse.y; out->coarse_cos = coarse.c; out->coarse_sin = coarse.s;
  out->iterations = w.iterations; out->converged = w.status == TSD_ALIGN_CONVERGED ? 1 : 0;
  out->n_ok = w.n_ok; out->weight_sum = w.sums[9];
  out->rms = w.sums[9] > 0.0 ? std::sqrt(w.sums[10] / w.sums[9]) : std::nan("");
  out->overlap = w.sums[9] / (double)n;
  for (int t = 0; t < 6; t++) out->info[t] = w.sums[t];
  const double tx = w.m[0] - (w.c * prm->pivot_x - w.s * prm->pivot_y), ty = w.m[1] - (w.s * prm->pivot_x + w.c * prm->pivot_y);
  const double T[9] = {w.c, -w.s, tx, w.s, w.c, ty, 0.0, 0.0, 1.0};
  std::memcpy(out->T33, T, sizeof(T));
  // the nearest whole-cell shift (tsd_fuse: src's cell (x, y) is dst's cell (x + ox, y + oy)) and how far T is from it over src's corners
  const double cs = ctx->grid.cs, ox = std::rint(tx / cs), oy = std::rint(ty / cs);
  if (std::fabs(ox) < 2147483647.0 && std::fabs(oy) < 2147483647.0) {
    out->cell_off[0] = (int32_t)ox; out->cell_off[1] = (int32_t)oy;
    const double side = (double)src_cells * cs;
    double worst = 0.0;
    for (int q = 0; q < 4; q++) {
      const double px = (q & 1) ? side : 0.0, py = (q & 2) ? side : 0.0;
      const double ex = (w.c * px - w.s * py + tx) - (px + ox * cs), ey = (w.s * px + w.c * py + ty) - (py + oy * cs);
      worst = std::max(worst, std::hypot(ex, ey) / cs);
    }
    out->cell_error = worst;
  }
  const bool rms_ok = !(prm->max_rms > 0.0) || out->rms <= prm->max_rms;
  out->found = out->converged && out->overlap >= prm->min_overlap && rms_ok ? 1 : 0;
  return TSD_OK;
}

static int align_check_count(tsd_ctx* ctx, int n, const char* who)
{
  if (n < 1) return set_error(ctx, TSD_E_ARG, (std::string(who) + ": no point").c_str(), hipSuccess);
  if (n > TSD_ALIGN_MAX_POINTS) return set_error(ctx, TSD_E_CAPACITY, (std::string(who) + ": points > TSD_ALIGN_MAX_POINTS").c_str(), hipSuccess);
  return TSD_OK;
}

}  // namespace tsd

using namespace tsd;

extern "C" {

int tsd_align_points(tsd_ctx* ctx, const tsd_align_params* prm, const double* points_xy, int n, int on_device, tsd_align_result* out)
{
  if (!ctx || !prm || !points_xy || !out) return TSD_E_ARG;
  if (int rc = align_check_count(ctx, n, "tsd_align_points")) return rc;
  std::vector<double> table;
  if (int rc = align_check_params(ctx, prm, false, "tsd_align_points", table)) return rc;
  if (!on_device && !points_in_reach(ctx->grid, points_xy, n))
    return set_error(ctx, TSD_E_ARG, "tsd_align_points: a point is not finite or further than TSD_RELOC_MAX_REACH grid widths away", hipSuccess);
  if (reloc_scan_in_flight(ctx)) return set_error(ctx, TSD_E_ARG, "tsd_align_points: a scan of this context is in flight (collect it first)", hipSuccess);
  return align_run(ctx, prm, table, points_xy, n, on_device != 0, ctx->grid.N, out);
}

int tsd_map_align(tsd_ctx* dst, tsd_ctx* src, const tsd_align_params* prm, tsd_align_result* out)
{
  if (!dst || !src || !prm || !out) return TSD_E_ARG;
  if (dst == src) return set_error(dst, TSD_E_ARG, "tsd_map_align: dst and src are the same context", hipSuccess);
  if (dst->device != src->device) return set_error(dst, TSD_E_ARG, "tsd_map_align: dst and src are on different devices", hipSuccess);
  std::vector<double> table;
  if (int rc = align_check_params(dst, prm, true, "tsd_map_align", table)) return rc;
  if (reloc_scan_in_flight(dst) || reloc_scan_in_flight(src))
    return set_error(dst, TSD_E_ARG, "tsd_map_align: a scan of dst or src is in flight (collect it first)", hipSuccess);
  // ---- the arguments stand ----
  int n = 0;
  if (int rc = tsd_surface_extract(src, nullptr, &n)) return set_error(dst, rc, "tsd_map_align: tsd_surface_extract(src) failed", hipSuccess);
  if (n == 0) { align_clear_result(out); dst->align.n_rec = 0; return TSD_OK; }
  if (int rc = align_check_count(dst, n, "tsd_map_align")) return rc;
  tsd_align_params p = *prm;
  if (std::isnan(p.pivot_x) && std::isnan(p.pivot_y)) p.pivot_x = p.pivot_y = 0.5 * ((double)src->grid.N * src->grid.cs);
  if (int rc = enter(dst)) return rc;
  if (int rc = align_ensure(dst, (size_t)n)) return rc;
  // (the list is complete: tsd_surface_extract waited for it.  The half-cell offset: see the header.)
  hipLaunchKernelGGL(k_align_stage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dst->stream, (const double*)src->surface.d_xy,
                     dst->align.d_pts, n, 0.5 * src->grid.cs, reloc_reach(dst->grid) + (double)src->grid.N * src->grid.cs, dst->align.d_bad);
  TSD_HIP_CHECK(dst, hipGetLastError());
  return align_run(dst, &p, table, dst->align.d_pts, n, true, src->grid.N, out);
}

int tsd_debug_align_scores(tsd_ctx* ctx, uint32_t* scores, int cap)
{
  return ctx ? ctx->align.volume.copy_out(ctx, scores, cap) : TSD_E_ARG;
}

int tsd_debug_align_peaks(tsd_ctx* ctx, tsd_align_peak* records, int cap)
{
  if (!ctx) return TSD_E_ARG;
  const tsd_ctx::Align& al = ctx->align;
  const int m = std::min(al.n_rec, cap > 0 ? cap : 0);
  if (m > 0 && records) std::memcpy(records, al.h_rec, sizeof(tsd_align_peak) * (size_t)m);
  return al.n_rec;
}

int tsd_debug_align_sums(tsd_ctx* ctx, const double* points_xy, int n, const double pivot[2], const double m[2], double c, double s,
                         double v_cut, double sums[11], int* n_ok)
{
  if (!ctx || !points_xy || !pivot || !m || !sums || !n_ok) return TSD_E_ARG;
  if (int rc = align_check_count(ctx, n, "tsd_debug_align_sums")) return rc;
  if (!(v_cut > 0.0 && v_cut <= 1.0)) return set_error(ctx, TSD_E_ARG, "tsd_debug_align_sums: v_cut outside (0, 1]", hipSuccess);
  if (reloc_scan_in_flight(ctx)) return set_error(ctx, TSD_E_ARG, "tsd_debug_align_sums: a scan of this context is in flight", hipSuccess);
  if (int rc = enter(ctx)) return rc;
  if (int rc = align_ensure(ctx, (size_t)n)) return rc;
  tsd_ctx::Align& al = ctx->align;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(al.d_pts, points_xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  AlignRefineArgs a{};
  a.pts = al.d_pts; a.n = n; a.iterations = 0;
  a.pvx = pivot[0]; a.pvy = pivot[1]; a.v_cut = v_cut; a.eps = 1e-6; a.lever = 1.0;
  a.keys = nullptr; a.cos_sin = nullptr; a.rec = al.d_rec + ALIGN_DEBUG_SLOT;
  a.start[0] = m[0]; a.start[1] = m[1]; a.start[2] = c; a.start[3] = s;
  hipLaunchKernelGGL(k_align_refine, dim3(1), dim3(ALIGN_THREADS), 0, ctx->stream, ctx->grid, a);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  tsd_align_peak* h = al.h_rec + ALIGN_DEBUG_SLOT;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(h, al.d_rec + ALIGN_DEBUG_SLOT, sizeof(tsd_align_peak), hipMemcpyDeviceToHost, ctx->stream));
  TSD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(sums, h->sums, sizeof(double) * ALIGN_SUMS);
  *n_ok = h->n_ok;
  return TSD_OK;
}

}  // extern "C"
