// pdf_front.hpp -- the host side the three pre-registrations share: registration_mode 1 (RandomNormalMatching, rnmatch.hip), 2
// (PDFMatching, pdfmatch.hip) and 3 (TSD_PDFMatching, tsdpdf.hip) are one algorithm with three scoring rules
// (RandomNormalMatching.cpp:79-262 = PDFMatching.cpp:45-220 = TSD_PDFMatching.cpp:31-205).  Shared here: the front end -- subsampleMask
// of the scene, the PCA normals of both sets (k_pdf_normals), extractSamples, pickControlSet, the trial picks and the candidate list in
// the reference's serial (trial, i) order -- and the scaffold of a match call around it: argument check, buffer carving, candidate
// staging, phase timer, result fetch, the score read-back of the test hooks.  Only the scoring differs (the kernels' shared device
// code: tsdpdf_device.hpp).  Implemented in tsdpdf.hip.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <initializer_list>
#include <vector>
#include "tsdpdf_device.hpp"

namespace tsd {

// offsets into a buffer, handed out front to back: carve(bytes) rounds the piece up to 16 bytes, exact(bytes) does not
struct PdfCarve {
  size_t off = 0;
  static size_t al(size_t x) { return (x + 15) & ~(size_t)15; }
  size_t operator()(size_t bytes) { const size_t at = off; off += al(bytes); return at; }
  size_t exact(size_t bytes) { const size_t at = off; off += bytes; return at; }
};

// The phases of a match call, switched on by an environment variable (read once: one static timer per call site): host laps
// [0, 5), up to three kernel intervals between marks on the stream [5, 8), a line every 100 calls (the caller's own text).
struct PdfPhaseTimer {
  explicit PdfPhaseTimer(const char* env) : on(std::getenv(env) != nullptr) {}
  const bool on;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int t_calls = 0;
  std::chrono::steady_clock::time_point t;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; int marks = 0;
  void start() { if (on) t = std::chrono::steady_clock::now(); }
  void lap(int i) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    acc[i] += std::chrono::duration<double, std::micro>(now - t).count(); t = now;
  }
  void mark(hipStream_t stream) { if (on && marks < 4 && hipEventCreate(&ev[marks]) == hipSuccess) hipEventRecord(ev[marks++], stream); }
  // after the call's stream sync: folds the marks in; true when the line is due
  bool due() {
    if (!on) return false;
    for (int i = 0; i + 1 < marks; i++) { float ms = 0.f; hipEventElapsedTime(&ms, ev[i], ev[i + 1]); acc[5 + i] += 1000.0 * ms; }
    for (int i = 0; i < marks; i++) hipEventDestroy(ev[i]);
    marks = 0;
    return ++t_calls % 100 == 0;
  }
  double us(int i) const { return acc[i] / t_calls; }
};

struct PdfFrontEnd {
  // where the reference's match() stands after the front end
  enum Stage { FEW_POINTS,       // n < 3 (:53-57): identity, nothing else set
               FEW_VALID,        // idxSValid / idxMValid < 3 (:129-139): identity, counts set
               NO_RESOLUTION,    // resolution <= 1e-6 (:161-171)
               NO_CANDIDATES,    // no (trial, i) pair passes the angle test
               SCORE } stage = FEW_POINTS;
  int n = 0, nC = 0, trials = 0, span = 0;
  double phi_max = 0.0;                    // min(phiMax, pi/2)
  std::vector<int> idxM, idxS;             // extractSamples of both sets (ascending beam indices)
  std::vector<double> control;             // the control set, nC x 2
  std::vector<int> idxControl;             // the control set's scene indices (pickControlSet's idxControl)
  std::vector<double> phiM, phiS;          // calcPhi of both sets' normals, beam-indexed (-1e6 where masked)
  std::vector<PdfCandidate> cand;          // in the reference's serial order
  size_t max_cand = 0;                     // the candidate list's allocation (entries)
  // ctx->h_pdf / ctx->d_pdf: [M | S | masks | angles | control | candidates | pose | prob | result | extra]
  char* h = nullptr; char* d = nullptr;
  size_t off_S = 0, off_C = 0, off_K = 0, off_P = 0, off_prob = 0, off_res = 0, off_extra = 0, bC = 0;
  int n_cand() const { return (int)cand.size(); }
  // the device's copies
  const double* dM() const { return reinterpret_cast<const double*>(d); }
  const double* dS() const { return reinterpret_cast<const double*>(d + off_S); }
  const double2* dC() const { return reinterpret_cast<const double2*>(d + off_C); }
  const PdfCandidate* dK() const { return reinterpret_cast<const PdfCandidate*>(d + off_K); }
  double* d_prob() const { return reinterpret_cast<double*>(d + off_prob); }
  PdfResult* d_res() const { return reinterpret_cast<PdfResult*>(d + off_res); }
};

// the caller's own part of the buffer behind the shared layout, sized from the beams and the candidate bound
typedef size_t (*PdfExtraBytes)(int n, size_t max_cand);

// The pointer / range check at the top of a match call (`ptrs`: everything but ctx and prm) and hipSetDevice; `text`: the caller's own
// words for a range error.
template <class Params>
int pdf_check_match(tsd_ctx* ctx, std::initializer_list<const void*> ptrs, int beams, const Params* prm, const char* text)
{
  if (!ctx || !prm) return TSD_E_ARG;
  for (const void* p : ptrs) if (!p) return TSD_E_ARG;
  if (beams < 1 || beams > TSD_MAX_BEAMS || prm->size_control_set < 0 || prm->size_control_set > PDF_MAX_CONTROL || prm->trials < 0)
    return set_error(ctx, TSD_E_CAPACITY, text, hipSuccess);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return TSD_OK;
}

// the front end: fills `fe` (and result's counts where the reference has them) and leaves M and S on the device at
// fe.d / fe.d + fe.off_S.  host_normals: the normals by the host restatement (libm's atan2, long double means) instead of
// k_pdf_normals, as TSD_PDF_HOST_NORMALS=1 selects for every call.  Returns TSD_OK or an error code (set_error); fe.stage says how far the reference's match() gets.
int pdf_front_end(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B, const uint8_t* mask_s,
                  int beams, int trials_cfg, int size_control_set, double phi_max_in, double ang_res, const int* draws_subsample,
                  const int* draws_control, const int* draws_trials, PdfExtraBytes extra, PdfPhaseTimer& tm, tsd_tsdpdf_result* result,
                  PdfFrontEnd& fe, bool host_normals = false);

// control set + candidate list into the pinned buffer and to the device (one copy on ctx->stream: they are neighbours);
// h_cos_sin != nullptr: also libm's (cos, sin) of every candidate's angle, written there (the caller copies it with its own arrays)
int pdf_stage_candidates(tsd_ctx* ctx, const PdfFrontEnd& fe, double2* h_cos_sin);

// k_pdf_argmax (tsdpdf.hip) on ctx->stream: the first candidate in the reference's serial order that reaches the largest probability
// (> 0) among fe's candidates scored at fe.d_prob(), its T and counts written to fe.d_res(); modes 2 and 3 feed it
void launch_pdf_argmax(tsd_ctx* ctx, const PdfFrontEnd& fe);

// behind a match's launches: their launch error, one result record back to the pinned buffer, the stream's end
int pdf_fetch(tsd_ctx* ctx, void* h_rec, const void* d_rec, size_t bytes);
// ... and that of modes 2 and 3 (fe.off_res) into the caller's result
int pdf_fetch_result(tsd_ctx* ctx, const PdfFrontEnd& fe, tsd_tsdpdf_result* result);

// tsd_debug_pdf_match_scores / tsd_debug_rn_match_scores: up to `cap` entries of the last match's per-candidate arrays
// (ctx->match_dbg, left by a match of `mode`; elem: bytes per entry, 0 ends the list); returns their number
int pdf_debug_scores(tsd_ctx* ctx, int mode, int cap, void* const out[3], const int elem[3]);

}  // namespace tsd
