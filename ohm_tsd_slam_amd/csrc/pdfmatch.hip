// pdfmatch.hip -- the PDFMatching pre-registration ThreadLocalize runs before the ICP in registration_mode 2
// (ThreadLocalize.cpp:185-187, :545-553): obvious::PDFMatching::match (registration/ransacMatching/PDFMatching.cpp:47-432)
// on top of obvious::RandomMatching.
//
// What it computes.  The front end is registration_mode 3's (pdf_front.hpp): for `trials` randomly picked model points and every
// scene point within +-span beams whose normal angle differs by less than phiMax, the rigid motion T(idx, i).  Each candidate carries
// the control set through T (in the SENSOR frame: mode 2 has no TSensor) and scores it with a beam model: for each control point the
// model point with the nearest polar angle (a search over all valid model points), then probabilityOfTwoSingleScans of the two
// ranges (:435-487), multiplied over the control set in the reference's order.  A candidate wins on the largest product among those
// that see more than percentagePointsInC of the control set within maxAngleDiff of a model beam (:373).
//
// Where the work goes.  About 1 300 candidates x 140 control points x a search over ~1 000 model angles: a serial O(C x M) loop per
// candidate in the reference.  Here one WAVE per candidate (like k_pdf_score), one lane per control point, the model angles in LDS
// and searched by bisection when they are sorted (a scan's ray cast yields them in beam order), by the reference's linear scan
// otherwise; the factors are multiplied in the reference's order through scalar reads of the lanes.
//
// Exactness.  Unlike mode 3's bilinear look-ups, this score has a step exactly where a candidate is most often evaluated: the scene
// point i of candidate (idx, i) is a control point in about one candidate of two, T carries it onto model point idx up to rounding,
// so s == m within an ulp -- and p_short switches on at s < m (:455), a jump of a few per cent in that factor.  Which side of the
// step such a point lands on is decided by the last bit of cos(phi) / sin(phi) and of phi itself (a difference of two PCA normal
// angles).  So mode 2 takes both from the host's libm, as the reference does: the normals by the front end's host restatement
// (k_pdf_normals' double-double means and device atan2 differ in the last bits), cos / sin of every candidate's angle on the host,
// handed to the scoring kernel beside the candidate.  The rest -- T, the control points, their ranges -- is then the same IEEE
// arithmetic in the same order on both sides.
//
// Randomness: as in mode 3, the rand() streams are inputs (csrc/host/obvision draws them where the reference does).
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

constexpr int PDFM_WAVES = 4;              // candidates per workgroup and round
constexpr int PDFM_GRID = 512;             // workgroups at most; their waves stride over the candidates (the model angles are staged once per workgroup)

// the per-match constants of probabilityOfTwoSingleScans and of the field-of-view test
struct PdfmParams {
  double zhit, zphi, zshort, zmax, zrand, rangemax, sigphi, sighit, lamshort;
  double sigphit;        // 1 / (sqrt(2 pi) sighit) (PDFMatching.cpp:33)
  double angle_thresh;   // (M_PI / 180.0) * maxAngleDiff (:227)
  double pct;            // percentagePointsInC
  int skip_phi;          // zphi == 0 and pphi finite for every s: the zphi * pphi term adds +-0 (see pdfm_factor)
};

// Per valid model point k (idxMValid order, :200-204): its polar angle, its range and the normaliser of p_short,
// 1 / (1 - e^(-lamshort m_k)) (:457), which depends on m_k alone; and, once per match, whether the angles are non-decreasing
// (flag[0] != 0: they are not).
__global__ void __launch_bounds__(256)
k_pdfm_model(const double* __restrict__ M, const int* __restrict__ idxM, int nM, double lamshort,
             double* __restrict__ ang, double2* __restrict__ dist_norm, int* __restrict__ flag)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nM) return;
  const int i = idxM[k];
  const double x = M[2 * i], y = M[2 * i + 1];
  const double a = atan2(y, x);
  const double m = sqrt(x * x + y * y);          // sqrt(pow(x, 2) + pow(y, 2)) (:203): pow(x, 2) is x * x rounded, as gcc folds it
  ang[k] = a;
  dist_norm[k] = make_double2(m, 1.0 / (1.0 - pow(M_E, (-lamshort * m))));
  if (k + 1 < nM) {
    const int j = idxM[k + 1];
    const double b = atan2(M[2 * j + 1], M[2 * j]);
    if (!(a <= b)) atomicOr(flag, 1);            // (a NaN angle counts as out of order: the linear scan then decides)
  }
}

// PDFMatching::probabilityOfTwoSingleScans(m, s, .) (:435-487), literally: pow(M_E, .) and the reference's term order
__device__ __forceinline__ double pdfm_factor(const PdfmParams& p, double m, double norm, double s)
{
  double phit = 0.0, pphi = 0.0, pshort = 0.0, pmax = 0.0, prand = 0.0;
  if (s < p.rangemax) phit = p.sigphit * pow(M_E, ((-0.5 * ((m - s) * (m - s))) / (p.sighit * p.sighit)));     // (pow(m - s, 2))
  if (s < m) pshort = norm * p.lamshort * pow(M_E, (-p.lamshort * s));
  if (s >= p.rangemax) pmax = 1.0;
  if (s < p.rangemax) prand = 1.0 / p.rangemax;
  double ptemp = p.zhit * phit + p.zshort * pshort + p.zmax * pmax + p.zrand * prand;
  // p_phi = sigphi e^(-s^2 / (2 sigphi^2)) (:452; the reference scales by _sigphi, not _sigpphi).  With zphi == 0 the last term is
  // 0 * pphi = +-0 as long as pphi is finite -- the host sets skip_phi only then (sigphi finite, sigphi^2 a positive normal number:
  // the exponent is finite or -inf and pow(e, .) lies in [0, 1]) -- and x + (+-0) == x: skipping it changes no bit of the sum.
  if (!p.skip_phi) {
    pphi = p.sigphi * pow(M_E, ((-0.5 * s * s) / (p.sigphi * p.sigphi)));
    ptemp = ptemp + p.zphi * pphi;
  }
  return ptemp;
}

// The first k minimising |angle - A[k]| with a strict `<` from minAngleDiff = 2 pi, idx 0 (PDFMatching.cpp:324-337).
__device__ __forceinline__ int pdfm_nearest_linear(const double* A, int nM, double q, double& best)
{
  double mn = 2 * M_PI; int idx = 0;
  for (int k = 0; k < nM; k++) {
    const double diff = fabs(q - A[k]);
    if (diff < mn) { mn = diff; idx = k; }
  }
  best = mn;
  return idx;
}
// The same for non-decreasing A, by bisection.  For x <= y <= q, fl(q - x) >= fl(q - y) (rounding is monotone), and for q < x <= y,
// fl(x - q) <= fl(y - q): the differences fall up to the last element <= q and rise after it, so the minimum sits at that element or
// at the next one.  Equal differences go to the lower index (the linear scan keeps its first): from the last element <= q step left
// while the difference stays the same (equal angles, or distinct angles whose differences round alike), and take the element after
// it only if its difference is strictly smaller.  No difference below 2 pi: idx 0, 2 pi, as in the scan.
__device__ __forceinline__ int pdfm_nearest_sorted(const double* A, int nM, double q, double& best)
{
  int lo = 0, hi = nM;                          // first index with A[k] > q, in [0, nM]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] <= q) lo = mid + 1; else hi = mid;
  }
  double mn = 2 * M_PI; int idx = 0;
  if (lo > 0) {
    int k = lo - 1;
    const double d = fabs(q - A[k]);
    while (k > 0 && fabs(q - A[k - 1]) == d) k--;
    if (d < mn) { mn = d; idx = k; }
  }
  if (lo < nM) {
    const double d = fabs(q - A[lo]);
    if (d < mn) { mn = d; idx = lo; }
  }
  best = mn;
  return idx;
}

// One WAVE per candidate: lane l takes the control points l, l + 64, ...; the factors are multiplied in the reference's order
// s = 0 .. C-1 through scalar reads of the lanes (a lane past the control set contributes 1.0, which changes no bit), the
// field-of-view count is a ballot.  Writes the gated product (0 unless fov > C * percentagePointsInC) for the arg-max and, for the
// test hook, the ungated product and the count.
__global__ void __launch_bounds__(64 * PDFM_WAVES)
k_pdfm_score(const double* __restrict__ M, const double* __restrict__ S, const double* __restrict__ ang_g,
             const double2* __restrict__ dist_norm, const int* __restrict__ flag, int nM,
             const double2* __restrict__ control_g, int n_control, const PdfCandidate* __restrict__ cand,
             const double2* __restrict__ cos_sin, int n_cand,
             PdfmParams p, double* __restrict__ prob_out, double* __restrict__ prob_ungated, int* __restrict__ fov_out)
{
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  double* s_ang = s_dyn;                                                  // [nM]
  double2* s_ctrl = reinterpret_cast<double2*>(s_dyn + ((nM + 1) & ~1));  // [n_control]
  for (int k = threadIdx.x; k < nM; k += blockDim.x) s_ang[k] = ang_g[k];
  for (int k = threadIdx.x; k < n_control; k += blockDim.x) s_ctrl[k] = control_g[k];
  const bool sorted = ld_pinned(flag) == 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.x * PDFM_WAVES + wave; c < n_cand; c += (int)gridDim.x * PDFM_WAVES) {     // (whole waves: no barrier below)
    const PdfCandidate cd = cand[c];
    // T = TransformationMatrix33(phi, 0, 0) + translation (PDFMatching.cpp:244-250), as k_pdf_score builds it, with libm's
    // cos(phi) / sin(phi) from the host (see the head of this file)
    const double2 cs = cos_sin[c];
    const double co = cs.x, si = cs.y;
    int ci; double T02, T12;
    pdf_candidate_T(M, S, cd.idx, cd.ti, co, si, ci, T02, T12);
    double prob = 1.0;
    int fov = 0;
    for (int s0 = 0; s0 < n_control; s0 += 64) {
      const int s = s0 + lane;
      double f = 1.0;
      bool in_view = false;
      if (s < n_control) {
        // STemp = T * Control (:253; dgemm: k ascending from 0.0)
        const double2 cp = s_ctrl[s];
        double cx, cy;
        pdf_transform_point(co, -si, T02, si, co, T12, cp.x, cp.y, cx, cy);
        const double angle = atan2(cy, cx);
        const double distance = sqrt(cx * cx + cy * cy);                // (:311; pow(., 2) as above)
        double minAngleDiff;
        const int k = sorted ? pdfm_nearest_sorted(s_ang, nM, angle, minAngleDiff) : pdfm_nearest_linear(s_ang, nM, angle, minAngleDiff);
        in_view = minAngleDiff < p.angle_thresh;
        const double2 dn = dist_norm[k];
        f = pdfm_factor(p, dn.x, dn.y, distance);
      }
      fov += __popcll(__ballot(in_view));
      const int flo = __double2loint(f), fhi = __double2hiint(f);
#pragma unroll
      for (int j = 0; j < 64; j++)                                       // the reference's order
        prob *= __hiloint2double(__builtin_amdgcn_readlane(fhi, j), __builtin_amdgcn_readlane(flo, j));
    }
    if (n_control == 0) prob = 0.0;                                      // probOfAllScans.size() == 0 (:359-363)
    // (:373) the product wins only if more than percentagePointsInC of the control set is in view.  k_pdf_argmax starts from
    // bestProb = 0 and replaces on a strict `>` in the reference's serial order, so a gated-out candidate written as 0 can never be
    // chosen -- exactly what the reference's two-part test does -- and the arg-max serves both modes unchanged.
    const bool gate = (double)fov > (double)n_control * p.pct;
    if (lane == 0) { prob_out[c] = gate ? prob : 0.0; prob_ungated[c] = prob; fov_out[c] = fov; }
  }
}

}  // namespace tsd

using namespace tsd;

namespace {
constexpr int PDFM_DBG_MODE = 2;
// behind the shared layout: [idxM | angles | (range, normaliser) | flag | ungated products | fov counts | (cos, sin) per candidate]
struct PdfmLayout { size_t off_idx, off_ang, off_dn, off_flag, off_u, off_fov, off_cs, bytes; };
PdfmLayout pdfm_layout(int n, size_t max_cand)
{
  PdfCarve carve;
  PdfmLayout L;
  L.off_idx = carve((size_t)n * 4); L.off_ang = carve((size_t)n * 8); L.off_dn = carve((size_t)n * 16); L.off_flag = carve(16);
  L.off_u = carve(max_cand * 8); L.off_fov = carve(max_cand * 4); L.off_cs = carve(max_cand * 16);
  L.bytes = carve.off;
  return L;
}
size_t pdfm_extra(int n, size_t max_cand) { return pdfm_layout(n, max_cand).bytes; }
}

extern "C" int tsd_pdf_match(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B,
                             const uint8_t* mask_s, int beams, const tsd_pdfmatch_params* prm, const int* draws_subsample,
                             const int* draws_control, const int* draws_trials, tsd_tsdpdf_result* result)
{
  if (int rc = pdf_check_match(ctx, {model_xy_2B, mask_m, scene_xy_2B, mask_s, draws_subsample, draws_control, draws_trials, result},
                               beams, prm, "tsd_pdf_match: beams / control set out of range"))
    return rc;
  static PdfPhaseTimer tm("TSD_MODE2_TIMING");           // the phases of this call
  PdfFrontEnd fe;
  if (int rc = pdf_front_end(ctx, model_xy_2B, mask_m, scene_xy_2B, mask_s, beams, prm->trials, prm->size_control_set, prm->phi_max,
                             prm->ang_res, draws_subsample, draws_control, draws_trials, pdfm_extra, tm, result, fe,
                             true /* the host's normals: see the head of this file */))
    return rc;
  if (fe.stage != PdfFrontEnd::SCORE) return TSD_OK;     // the reference's early returns: TBest = identity (:53-65, :134-144, :167-171)
  const int nC = fe.nC, nM = (int)fe.idxM.size(), nc = fe.n_cand();
  const PdfmLayout L = pdfm_layout(fe.n, fe.max_cand);
  char* hx = fe.h + fe.off_extra; char* dx = fe.d + fe.off_extra;

  PdfmParams p;
  p.zhit = prm->zhit; p.zphi = prm->zphi; p.zshort = prm->zshort; p.zmax = prm->zmax; p.zrand = prm->zrand;
  p.rangemax = prm->rangemax; p.sigphi = prm->sigphi; p.sighit = prm->sighit; p.lamshort = prm->lamshort;
  p.sigphit = 1.0 / (sqrt(2.0 * M_PI) * prm->sighit);
  p.angle_thresh = (M_PI / 180.0) * prm->max_angle_diff;
  p.pct = prm->percentage_points_in_c;
  const double sp2 = prm->sigphi * prm->sigphi;
  p.skip_phi = prm->zphi == 0.0 && std::isfinite(prm->sigphi) && std::isnormal(sp2) ? 1 : 0;

  // ---- staging: the candidates with libm's cos / sin, the valid model indices, the cleared order flag
  if (int rc = pdf_stage_candidates(ctx, fe, reinterpret_cast<double2*>(hx + L.off_cs))) return rc;
  std::memcpy(hx + L.off_idx, fe.idxM.data(), (size_t)nM * 4);
  std::memset(hx + L.off_flag, 0, 16);
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(dx + L.off_idx, hx + L.off_idx, (size_t)nM * 4, hipMemcpyHostToDevice, ctx->stream));
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(dx + L.off_flag, hx + L.off_flag, 16, hipMemcpyHostToDevice, ctx->stream));
  TSD_HIP_CHECK(ctx, hipMemcpyAsync(dx + L.off_cs, hx + L.off_cs, (size_t)nc * 16, hipMemcpyHostToDevice, ctx->stream));
  tm.lap(3);
  // ---- device: per-model-point arrays, score, arg-max
  double* d_ang = reinterpret_cast<double*>(dx + L.off_ang);
  double2* d_dn = reinterpret_cast<double2*>(dx + L.off_dn);
  int* d_flag = reinterpret_cast<int*>(dx + L.off_flag);
  {
    ScopedKernelTimer t(ctx, "tsdpdf", true);
    tm.mark(ctx->stream);
    hipLaunchKernelGGL(k_pdfm_model, dim3((nM + 255) / 256), dim3(256), 0, ctx->stream, fe.dM(), reinterpret_cast<const int*>(dx + L.off_idx), nM,
                       prm->lamshort, d_ang, d_dn, d_flag);
    tm.mark(ctx->stream);
    const size_t lds = (size_t)((nM + 1) & ~1) * 8 + (size_t)nC * 16;      // <= 32 KB + 16 KB
    const int blocks = std::min((nc + PDFM_WAVES - 1) / PDFM_WAVES, PDFM_GRID);
    hipLaunchKernelGGL(k_pdfm_score, dim3(blocks), dim3(64 * PDFM_WAVES), lds, ctx->stream, fe.dM(), fe.dS(), d_ang, d_dn, d_flag, nM,
                       fe.dC(), nC, fe.dK(), reinterpret_cast<const double2*>(dx + L.off_cs), nc, p,
                       fe.d_prob(), reinterpret_cast<double*>(dx + L.off_u), reinterpret_cast<int*>(dx + L.off_fov));
    tm.mark(ctx->stream);
    launch_pdf_argmax(ctx, fe);
    tm.mark(ctx->stream);
  }
  if (int rc = pdf_fetch_result(ctx, fe, result)) return rc;
  tm.lap(4);
  if (tm.due())
    std::fprintf(stderr, "tsd_pdf_match, us per call: normals of both sets (host) %.1f | lists + control set %.1f | candidates (%d) %.1f | "
                 "cos / sin + staging + H2D issue %.1f | kernels + D2H %.1f (model arrays %.1f | scoring %.1f | arg-max %.1f)\n",
                 tm.us(0), tm.us(1), nc, tm.us(2), tm.us(3), tm.us(4), tm.us(5), tm.us(6), tm.us(7));
  ctx->match_dbg.n = nc; ctx->match_dbg.mode = PDFM_DBG_MODE;
  ctx->match_dbg.off[0] = fe.off_extra + L.off_u; ctx->match_dbg.off[1] = fe.off_extra + L.off_fov;
  return TSD_OK;
}

extern "C" int tsd_debug_pdf_match_scores(tsd_ctx* ctx, double* prob_ungated, int* fov, int cap)
{
  if (!ctx || cap < 0 || (cap > 0 && (!prob_ungated || !fov))) return TSD_E_ARG;
  void* const out[3] = {prob_ungated, fov, nullptr};
  const int elem[3] = {8, 4, 0};
  return pdf_debug_scores(ctx, PDFM_DBG_MODE, cap, out, elem);
}
