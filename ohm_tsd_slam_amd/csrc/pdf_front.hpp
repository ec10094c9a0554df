// pdf_front.hpp -- the front end registration_mode 2 (PDFMatching, pdfmatch.hip) and registration_mode 3 (TSD_PDFMatching,
// tsdpdf.hip) share statement for statement (PDFMatching.cpp:45-220 vs TSD_PDFMatching.cpp:31-205): subsampleMask of the scene,
// the PCA normals of both sets (k_pdf_normals), extractSamples, pickControlSet, the trial picks and the candidate list in the
// reference's serial (trial, i) order.  Only the scoring differs.
#pragma once
#include <chrono>
#include <cstddef>
#include <vector>
#include "tsdpdf_device.hpp"

namespace tsd {

// host phases of a match (TSD_MODE3_TIMING=1): the caller owns the accumulators
struct PdfLap {
  bool on = false; double* acc = nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(int i) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    acc[i] += std::chrono::duration<double, std::micro>(now - t).count(); t = now;
  }
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
};

// the caller's own part of the buffer behind the shared layout, sized from the beams and the candidate bound
typedef size_t (*PdfExtraBytes)(int n, size_t max_cand);

// the front end: fills `fe` (and result's counts where the reference has them) and leaves M and S on the device at
// fe.d / fe.d + fe.off_S.  host_normals: the normals by the host restatement (libm's atan2, long double means) instead of
// k_pdf_normals, as TSD_PDF_HOST_NORMALS=1 selects for every call.  Returns TSD_OK or an error code (set_error); fe.stage says how far the reference's match() gets.
int pdf_front_end(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B, const uint8_t* mask_s,
                  int beams, int trials_cfg, int size_control_set, double phi_max_in, double ang_res, const int* draws_subsample,
                  const int* draws_control, const int* draws_trials, PdfExtraBytes extra, PdfLap& lap, tsd_tsdpdf_result* result,
                  PdfFrontEnd& fe, bool host_normals = false);

// k_pdf_argmax (tsdpdf.hip) on `stream`: the first candidate in the reference's serial order that reaches the largest probability
// (> 0), its T and counts written to *out; both modes' scoring kernels feed it
void launch_pdf_argmax(hipStream_t stream, const double* prob, const PdfCandidate* cand, int n_cand, const double* M, const double* S,
                       PdfResult* out);

}  // namespace tsd
