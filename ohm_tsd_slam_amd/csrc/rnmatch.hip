// rnmatch.hip -- the RandomNormalMatching pre-registration ThreadLocalize runs before the ICP in registration_mode 1
// (ThreadLocalize.cpp:183, :537-545): obvious::RandomNormalMatching::match (registration/ransacMatching/RandomNormalMatching.cpp:67-395)
// on top of obvious::RandomMatching.
//
// What it computes.  The front end is registration_modes 2 and 3's (pdf_front.hpp; RandomNormalMatching.cpp:79-262 restates
// PDFMatching.cpp statement for statement): for `trials` randomly picked model points and every scene point within +-span beams whose
// normal angle differs by less than phiMax, the rigid motion T(idx, i).  Each candidate carries the control set through T and rates it
// (:266-331): a control point is in view unless its polar angle lies outside the polar angles of the first and last valid model point
// (:159-160, :273-282); for each one in view, the exact nearest valid model point under L2 (FLANN's kd-tree with eps = 0, :296-306),
// err = d^2 / epsThresh^2 + 0.33 (1 - cos(phiM[q] - phiControl[s] - phi)) / 2 (:322-324), errSum over the in-view points in ascending
// control order and cntMatch = #(err < 1).  Candidates with cntMatch > pointsInC / 3 compete by Kuehn's rating (:338-359), an
// order-dependent fold, defined here in the reference's serial (trial, i) order.
//
// Where the work goes.  About 1 050 candidates x 140 control points x an exact search over ~1 050 model points: 150 M squared
// distances per scan.  k_rnm_score: one WORKGROUP per candidate (grid-strided), one thread per control point, the valid model points
// and their normal angles in LDS and scanned in ascending order by every lane at once (broadcast reads, no data-dependent memory
// traffic); the errors meet in LDS and one thread sums them in the reference's order.  k_rnm_select: one wave folds the candidates 64
// at a time -- each lane tests the rule against the current best, a ballot finds the first that accepts, the state moves to it and
// only the lanes after it are tested again -- and writes TBest.
//
// Exactness.  The nearest neighbour: d^2 = (qx - mx)^2 + (qy - my)^2 (x term first, no FMA: -ffp-contract=off), the smallest wins,
// a strict `<` in ascending idxMValid order keeps the lowest position among equal distances -- the repo's tie rule.
// As in mode 2, the normals and each candidate's cos / sin come from the host's libm, so T and the control points under T are the
// reference's IEEE operations in its order; the field-of-view bounds are taken with the same device atan2 as the control points' angles,
// so a control point that T carries exactly onto the first or last model point sits on the bound on both sides.  What remains device
// arithmetic (atan2 of the control points, cos of the consensus term) moves err by an ulp or so: errSum agrees to ~1e-15 relative,
// cntMatch exactly unless an err lies within an ulp of 1.0.
//
// Randomness: as in modes 2 and 3, the rand() streams are inputs (csrc/host/obvision draws them where the reference does).
#include "tsd_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsdpdf_device.hpp"
#include "pdf_front.hpp"

namespace tsd {

constexpr int RNM_GRID = 2048;            // workgroups at most; they stride over the candidates (the model is staged once per workgroup)
constexpr double RNM_SCALE_ORIENTATION = 0.33;     // _scaleOrientation (RandomNormalMatching.cpp:22)

// what k_rnm_select leaves for the host
struct RnmResult { double T[9]; double ratio, err; int cnt, max_cnt, idx, i, winner, pad; };

// One WORKGROUP per candidate, thread s on control point s (blockDim = 64 * ceil(nC / 64)).  Writes, per candidate, cntMatch (before the
// cntMatchThresh test), maxCntMatch and errSum.
__global__ void __launch_bounds__(PDF_MAX_CONTROL)
k_rnm_score(const double2* __restrict__ mv_g, const double* __restrict__ phim_g, int nM, const double2* __restrict__ ctrl_g,
            const double* __restrict__ phic_g, int nC, const PdfCandidate* __restrict__ cand, const double2* __restrict__ cos_sin,
            int n_cand, const double* __restrict__ M, const double* __restrict__ S, double scale_d,
            int* __restrict__ cnt_out, int* __restrict__ max_out, double* __restrict__ err_out)
{
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  double2* s_m = reinterpret_cast<double2*>(s_dyn);           // [nM] valid model points, idxMValid order
  double2* s_c = s_m + nM;                                    // [nC] control set
  double* s_phm = reinterpret_cast<double*>(s_c + nC);        // [nM] phiM[idxMValid[k]]
  double* s_phc = s_phm + nM;                                 // [nC] phiControl
  double* s_err = s_phc + nC;                                 // [nC] this candidate's err (0.0 out of view)
  __shared__ int s_cnt[PDF_MAX_CONTROL / 64], s_max[PDF_MAX_CONTROL / 64];
  for (int k = threadIdx.x; k < nM; k += blockDim.x) { s_m[k] = mv_g[k]; s_phm[k] = phim_g[k]; }
  for (int k = threadIdx.x; k < nC; k += blockDim.x) { s_c[k] = ctrl_g[k]; s_phc[k] = phic_g[k]; }
  __syncthreads();
  // the frustum: polar angles of the first and last valid model point (:159-160)
  const double2 mf = s_m[0], ml = s_m[nM - 1];
  const double thetaBoundMin = atan2(mf.y, mf.x), thetaBoundMax = atan2(ml.y, ml.x);
  const int s = threadIdx.x, lane = s & 63, wave = s >> 6, W = (int)blockDim.x >> 6;
  for (int c = blockIdx.x; c < n_cand; c += (int)gridDim.x) {
    const PdfCandidate cd = cand[c];
    // T = TransformationMatrix33(phi, 0, 0) + translation (:257-263), with libm's cos(phi) / sin(phi) from the host
    const double2 cs = cos_sin[c];
    const double co = cs.x, si = cs.y;
    int ci; double T02, T12;
    pdf_candidate_T(M, S, cd.idx, cd.ti, co, si, ci, T02, T12);
    double cx = 0.0, cy = 0.0;
    bool in_view = false;
    if (s < nC) {
      // STemp = T * Control (:266; dgemm: k ascending from 0.0)
      const double2 cp = s_c[s];
      pdf_transform_point(co, -si, T02, si, co, T12, cp.x, cp.y, cx, cy);
      const double thetaControl = atan2(cy, cx);
      in_view = !(thetaControl > thetaBoundMax || thetaControl < thetaBoundMin);     // (:274)
    }
    const unsigned long long vb = __ballot(in_view);
    bool match = false;
    if (vb) {                                                  // (wave-uniform: a wave with no control point in view skips the search)
      // exact nearest valid model point, lowest position among equal distances
      double bd = INFINITY; int bk = 0;
#pragma unroll 4
      for (int k = 0; k < nM; k++) {
        const double2 m = s_m[k];
        const double dx = cx - m.x, dy = cy - m.y;
        const double d = dx * dx + dy * dy;
        if (d < bd) { bd = d; bk = k; }
      }
      if (in_view) {
        const double normalConsensus = (1.0 - cos(s_phm[bk] - s_phc[s] - cd.phi)) / 2.0;   // (:322)
        const double err = bd * scale_d + normalConsensus * RNM_SCALE_ORIENTATION;        // (:324)
        s_err[s] = err;
        match = err < 1.0;                                                                // (:330)
      }
    }
    if (s < nC && !in_view) s_err[s] = 0.0;
    const unsigned long long mb = __ballot(match);
    if (lane == 0) { s_cnt[wave] = __popcll(mb); s_max[wave] = __popcll(vb); }
    __syncthreads();
    if (s == 0) {
      // errSum += err over the in-view points, s ascending (:329).  Every err is >= +0 (d^2 and 1 - cos are), so the sum stays >= +0 and
      // adding the +0.0 written for a point out of view changes no bit
      double errSum = 0.0;
      for (int j = 0; j < nC; j++) errSum += s_err[j];
      int cnt = 0, mx = 0;
      for (int w = 0; w < W; w++) { cnt += s_cnt[w]; mx += s_max[w]; }
      cnt_out[c] = cnt; max_out[c] = mx; err_out[c] = errSum;
    }
    __syncthreads();                                           // (s_err / s_cnt are rewritten for the next candidate)
  }
}

// Kuehn's rating (RandomNormalMatching.cpp:338-359) folded over the candidates in their serial order by one wave.  A candidate takes
// part if cntMatch > cntMatchThresh (unsigned, :338); it replaces the best if
//   rateCondition       = (ratio - bestRatio) > 1e-5 && cntMatch > bestCnt, or
//   similarityCondition = fabs((ratio - bestRatio) < 1e-5) && cntMatch == bestCnt && errSum < bestErr
// where the reference's fabs() is applied to the bool: any smaller ratio passes its first term.  64 candidates at a time: every lane
// tests the rule against the current best, the first lane that accepts (ballot) becomes the best, and only the lanes after it are
// tested again -- exactly the serial fold, with one pass per 64 candidates plus one per acceptance.  `cand` == nullptr (test hook):
// no T.
__global__ void __launch_bounds__(64)
k_rnm_select(const int* __restrict__ cnt_g, const int* __restrict__ max_g, const double* __restrict__ err_g, int n, unsigned thresh,
             const PdfCandidate* __restrict__ cand, const double2* __restrict__ cos_sin, const double* __restrict__ M,
             const double* __restrict__ S, RnmResult* __restrict__ out)
{
  const int lane = threadIdx.x;
  const double equalThres = 1e-5;
  double bestRatio = 0.0, bestErr = 1e12;
  unsigned bestCnt = 0, bestMax = 0;
  int win = -1;
  for (int base = 0; base < n; base += 64) {
    const int c = base + lane;
    unsigned cnt = 0, mx = 0; double err = 0.0, ratio = 0.0;
    bool part = false;
    if (c < n) {
      cnt = (unsigned)cnt_g[c]; mx = (unsigned)max_g[c]; err = err_g[c];
      part = cnt > thresh;
      ratio = (double)cnt / (double)mx;                       // (:342)
    }
    const int rlo = __double2loint(ratio), rhi = __double2hiint(ratio), elo = __double2loint(err), ehi = __double2hiint(err);
    int start = 0;
    for (;;) {
      const bool rateCondition = ((ratio - bestRatio) > equalThres) && (cnt > bestCnt);
      const bool similarityCondition = fabs((double)((ratio - bestRatio) < equalThres)) != 0.0 && (cnt == bestCnt) && err < bestErr;
      const unsigned long long b = __ballot(part && lane >= start && (rateCondition || similarityCondition));
      if (!b) break;
      const int j = __ffsll((long long)b) - 1;
      bestRatio = __hiloint2double(__builtin_amdgcn_readlane(rhi, j), __builtin_amdgcn_readlane(rlo, j));
      bestErr = __hiloint2double(__builtin_amdgcn_readlane(ehi, j), __builtin_amdgcn_readlane(elo, j));
      bestCnt = (unsigned)__builtin_amdgcn_readlane((int)cnt, j);
      bestMax = (unsigned)__builtin_amdgcn_readlane((int)mx, j);
      win = base + j;
      start = j + 1;
    }
  }
  if (lane == 0) {
    RnmResult r;
    for (int i = 0; i < 9; i++) r.T[i] = (i % 4 == 0) ? 1.0 : 0.0;
    r.ratio = bestRatio; r.err = bestErr; r.cnt = (int)bestCnt; r.max_cnt = (int)bestMax; r.idx = -1; r.i = -1; r.winner = win; r.pad = 0;
    if (win >= 0 && cand) {
      // TBest = T of the winner (:257-263, :357), with the host's cos / sin as in k_rnm_score
      const PdfCandidate cd = cand[win];
      const double2 cs = cos_sin[win];
      const double co = cs.x, si = cs.y;
      r.T[0] = co; r.T[1] = -si; r.T[3] = si; r.T[4] = co;
      pdf_candidate_T(M, S, cd.idx, cd.ti, co, si, r.i, r.T[2], r.T[5]);
      r.idx = cd.idx;
    }
    *out = r;
  }
}

}  // namespace tsd

using namespace tsd;

namespace {
constexpr int RNM_DBG_MODE = 1;
// behind the shared layout: [model points | phiM | phiControl | (cos, sin) | cntMatch | maxCntMatch | errSum | result], per match
struct RnmLayout { size_t off_mv, off_phm, off_phc, off_cs, off_cnt, off_max, off_err, off_res, bytes; };
RnmLayout rnm_layout(int n, size_t max_cand)
{
  PdfCarve carve;
  RnmLayout L;
  L.off_mv = carve((size_t)n * 16); L.off_phm = carve((size_t)n * 8); L.off_phc = carve((size_t)n * 8); L.off_cs = carve(max_cand * 16);
  L.off_cnt = carve(max_cand * 4); L.off_max = carve(max_cand * 4); L.off_err = carve(max_cand * 8); L.off_res = carve(sizeof(RnmResult));
  L.bytes = carve.off;
  return L;
}
size_t rnm_extra(int n, size_t max_cand) { return rnm_layout(n, max_cand).bytes; }
}

extern "C" int tsd_rn_match(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B,
                            const uint8_t* mask_s, int beams, const tsd_rnmatch_params* prm, const int* draws_subsample,
                            const int* draws_control, const int* draws_trials, tsd_rnmatch_result* result)
{
  if (int rc = pdf_check_match(ctx, {model_xy_2B, mask_m, scene_xy_2B, mask_s, draws_subsample, draws_control, draws_trials, result},
                               beams, prm, "tsd_rn_match: beams / control set out of range"))
    return rc;
  static PdfPhaseTimer tm("TSD_MODE1_TIMING");           // the phases of this call
  std::memset(result, 0, sizeof(*result));
  tsd_tsdpdf_result fr;
  PdfFrontEnd fe;
  const int rc = pdf_front_end(ctx, model_xy_2B, mask_m, scene_xy_2B, mask_s, beams, prm->trials, prm->size_control_set, prm->phi_max,
                               prm->ang_res, draws_subsample, draws_control, draws_trials, rnm_extra, tm, &fr, fe,
                               true /* the host's normals, as mode 2 */);
  // the reference's early returns: TBest = identity (:82-92, :165-175, :192-201), counts as far as it gets
  std::memcpy(result->T, fr.T, sizeof(fr.T));
  result->ratio = 0.0; result->err_sum = 1e12; result->cnt_match = 0; result->max_cnt_match = 0;
  result->idx_model = -1; result->idx_scene = -1; result->candidates = fr.candidates;
  result->valid_model = fr.valid_model; result->valid_scene = fr.valid_scene; result->control_points = fr.control_points;
  if (rc) return rc;
  if (fe.stage != PdfFrontEnd::SCORE) return TSD_OK;
  const int nC = fe.nC, nM = (int)fe.idxM.size(), nc = fe.n_cand();
  const RnmLayout L = rnm_layout(fe.n, fe.max_cand);
  char* hx = fe.h + fe.off_extra; char* dx = fe.d + fe.off_extra;

  // ---- host staging: the valid model points and their normal angles (idxMValid order), the control set's angles
  // (calcPhi(NControl, NULL, .) = phiS at the control points, :145-154), the candidates with libm's cos / sin
  double2* h_mv = reinterpret_cast<double2*>(hx + L.off_mv);
  double* h_phm = reinterpret_cast<double*>(hx + L.off_phm);
  double* h_phc = reinterpret_cast<double*>(hx + L.off_phc);
  for (int k = 0; k < nM; k++) {
    const int i = fe.idxM[k];
    h_mv[k] = make_double2(model_xy_2B[2 * i], model_xy_2B[2 * i + 1]);
    h_phm[k] = fe.phiM[i];
  }
  for (int s = 0; s < nC; s++) h_phc[s] = fe.phiS[fe.idxControl[s]];
  if (int e = pdf_stage_candidates(ctx, fe, reinterpret_cast<double2*>(hx + L.off_cs))) return e;
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(dx, hx, L.off_cs + (size_t)nc * 16, hipMemcpyHostToDevice, ctx->stream));
  tm.lap(3);
  const size_t lds = (size_t)nM * 24 + (size_t)nC * 32;       // <= 4 096 x 24 + 1 024 x 32 = 128 KB (160 KB per CU)
  if (int e = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(k_rnm_score), lds)) return e;
  // ---- device: score, select
  const double2* d_cs = reinterpret_cast<const double2*>(dx + L.off_cs);
  int* d_cnt = reinterpret_cast<int*>(dx + L.off_cnt);
  int* d_max = reinterpret_cast<int*>(dx + L.off_max);
  double* d_err = reinterpret_cast<double*>(dx + L.off_err);
  const unsigned cntMatchThresh = (unsigned)nC / 3;          // (:152)
  {
    ScopedKernelTimer t(ctx, "tsdpdf", true);
    tm.mark(ctx->stream);
    const int threads = 64 * std::max((nC + 63) / 64, 1);
    hipLaunchKernelGGL(k_rnm_score, dim3(std::min(nc, RNM_GRID)), dim3(threads), lds, ctx->stream,
                       reinterpret_cast<const double2*>(dx + L.off_mv), reinterpret_cast<const double*>(dx + L.off_phm), nM,
                       fe.dC(), reinterpret_cast<const double*>(dx + L.off_phc), nC, fe.dK(), d_cs, nc,
                       fe.dM(), fe.dS(), 1.0 / (prm->eps_thresh * prm->eps_thresh) /* _scaleDistance (:21) */, d_cnt, d_max, d_err);
    tm.mark(ctx->stream);
    hipLaunchKernelGGL(k_rnm_select, dim3(1), dim3(64), 0, ctx->stream, d_cnt, d_max, d_err, nc, cntMatchThresh, fe.dK(), d_cs, fe.dM(), fe.dS(),
                       reinterpret_cast<RnmResult*>(dx + L.off_res));
    tm.mark(ctx->stream);
  }
  if (int e = pdf_fetch(ctx, hx + L.off_res, dx + L.off_res, sizeof(RnmResult))) return e;
  tm.lap(4);
  if (tm.due())
    std::fprintf(stderr, "tsd_rn_match, us per call: normals of both sets (host) %.1f | lists + control set %.1f | candidates (%d) %.1f | "
                 "cos / sin + staging + H2D issue %.1f | kernels + D2H %.1f (scoring %.1f | selection %.1f)\n",
                 tm.us(0), tm.us(1), nc, tm.us(2), tm.us(3), tm.us(4), tm.us(5), tm.us(6));
  const RnmResult* r = reinterpret_cast<const RnmResult*>(hx + L.off_res);
  std::memcpy(result->T, r->T, sizeof(r->T));
  result->ratio = r->ratio; result->err_sum = r->err; result->cnt_match = r->cnt; result->max_cnt_match = r->max_cnt;
  result->idx_model = r->idx; result->idx_scene = r->i;
  ctx->match_dbg.n = nc; ctx->match_dbg.mode = RNM_DBG_MODE;
  ctx->match_dbg.off[0] = fe.off_extra + L.off_cnt; ctx->match_dbg.off[1] = fe.off_extra + L.off_max; ctx->match_dbg.off[2] = fe.off_extra + L.off_err;
  return TSD_OK;
}

extern "C" int tsd_debug_rn_match_scores(tsd_ctx* ctx, int* cnt, int* max_cnt, double* err_sum, int cap)
{
  if (!ctx || cap < 0 || (cap > 0 && (!cnt || !max_cnt || !err_sum))) return TSD_E_ARG;
  void* const out[3] = {cnt, max_cnt, err_sum};
  const int elem[3] = {4, 4, 8};
  return pdf_debug_scores(ctx, RNM_DBG_MODE, cap, out, elem);
}

extern "C" int tsd_debug_rn_select(tsd_ctx* ctx, const int* cnt, const int* max_cnt, const double* err_sum, int n, int thresh, int* winner)
{
  if (!ctx || !winner || n < 0 || (n > 0 && (!cnt || !max_cnt || !err_sum))) return TSD_E_ARG;
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bi = ((size_t)std::max(n, 1) * 4 + 15) & ~(size_t)15, bytes = 2 * bi + (size_t)std::max(n, 1) * 8 + sizeof(RnmResult);
  char* d = nullptr;
  TSD_HIP_CHECK(ctx, hipMalloc(&d, bytes));
  RnmResult r;
  hipError_t e = hipSuccess;
  if (n > 0) {
    if (e == hipSuccess) e = hipMemcpyAsync(d, cnt, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + bi, max_cnt, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + 2 * bi, err_sum, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream);
  }
  RnmResult* d_res = reinterpret_cast<RnmResult*>(d + 2 * bi + (size_t)std::max(n, 1) * 8);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_rnm_select, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const int*>(d), reinterpret_cast<const int*>(d + bi),
                       reinterpret_cast<const double*>(d + 2 * bi), n, (unsigned)thresh, nullptr, nullptr, nullptr, nullptr, d_res);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&r, d_res, sizeof(RnmResult), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  hipFree(d);
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, "tsd_debug_rn_select", e);
  *winner = r.winner;
  return TSD_OK;
}
