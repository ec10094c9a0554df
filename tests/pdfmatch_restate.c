/* pdfmatch_restate.c -- an independent plain-C restatement of obvious::PDFMatching::match (registration_mode 2;
 * registration/ransacMatching/PDFMatching.cpp:47-432) with the three rand() streams as inputs, serial, in the reference's
 * statement order.  Test infrastructure: built by the tests (gcc -O2 -ffp-contract=off) into a temporary directory.
 * RandomMatching::calcNormals and Matrix::pcaAnalysis are the oracle's (rm_calc_normals / pca2_axes), not restated a third time. */
#include "../oracle/tsd_oracle.c"

/* the layout of tsd_pdfmatch_params (include/tsd_hip.h) */
typedef struct {
  int trials, size_control_set;
  double eps_thresh, zhit, zphi, zshort, zmax, zrand, percentage_points_in_c, rangemax, sigphi, sighit, lamshort;
  double max_angle_diff, max_angle_penalty, phi_max, ang_res;
} pdfr_params;

/* PDFMatching::probabilityOfTwoSingleScans (:435-487) with the members the constructor derives (:33-35) */
double pdfr_prob(const pdfr_params* p, double m, double s)
{
  const double sigphit = 1.0 / (sqrt(2.0 * M_PI) * p->sighit);
  double phit = 0, pphi = 0, pshort = 0, pmax = 0, prand = 0;
  if (s < p->rangemax) phit = sigphit * pow(M_E, ((-0.5 * pow((m - s), 2)) / (p->sighit * p->sighit)));
  pphi = p->sigphi * pow(M_E, ((-0.5 * s * s) / (p->sigphi * p->sigphi)));
  if (s < m) {
    double n = 1.0 / (1.0 - pow(M_E, (-p->lamshort * m)));
    pshort = n * p->lamshort * pow(M_E, (-p->lamshort * s));
  }
  if (s >= p->rangemax) pmax = 1.0;
  if (s < p->rangemax) prand = 1.0 / p->rangemax;
  return p->zhit * phit + p->zshort * pshort + p->zmax * pmax + p->zrand * prand + p->zphi * pphi;
}

/* the model point nearest in angle (:324-337): first k with the smallest |angle - A[k]|, from 2 pi / 0 */
int pdfr_nearest(const double* A, int n, double angle, double* min_out)
{
  double minAngleDiff = 2 * M_PI;
  int idx = 0;
  for (int k = 0; k < n; k++) {
    const double diff = fabs(angle - A[k]);
    if (diff < minAngleDiff) { minAngleDiff = diff; idx = k; }
  }
  *min_out = minAngleDiff;
  return idx;
}

/* Returns 0, 1 (an early return: identity) or 2 (resolution not set: identity).  out_counts = {candidates, valid model,
 * valid scene, control points, idx, i}; per candidate (serial order, up to cap) the ungated product and the field-of-view
 * count. */
int pdfr_match(const double* M, const uint8_t* maskM, const double* S, const uint8_t* maskS, int n, const pdfr_params* p,
               const int* draws_subsample, const int* draws_control, const int* draws_trials, double T_out[9], double* prob_out,
               int out_counts[6], double* ungated, int* fov_out, int cap)
{
  const int SR = 10 / 2;
  for (int i = 0; i < 9; i++) T_out[i] = (i % 4 == 0) ? 1.0 : 0.0;
  *prob_out = 0.0;
  for (int i = 0; i < 6; i++) out_counts[i] = 0;
  out_counts[4] = out_counts[5] = -1;
  if (n < 3) return 1;
  double* NM = (double*)calloc(2 * (size_t)n, sizeof(double));
  double* NS = (double*)calloc(2 * (size_t)n, sizeof(double));
  double* phiM = (double*)malloc(sizeof(double) * (size_t)n);
  double* phiS = (double*)malloc(sizeof(double) * (size_t)n);
  uint8_t* maskMpca = (uint8_t*)malloc((size_t)n);
  uint8_t* maskSpca = (uint8_t*)malloc((size_t)n);
  int* idxMValid = (int*)malloc(sizeof(int) * (size_t)n);
  int* idxSValid = (int*)malloc(sizeof(int) * (size_t)n);
  int* rest = (int*)malloc(sizeof(int) * (size_t)n);
  double* anglesArray = (double*)malloc(sizeof(double) * (size_t)n);
  double* distArray = (double*)malloc(sizeof(double) * (size_t)n);
  int nM = 0, nS = 0, rc = 0;
  /* model (:67-83) */
  memcpy(maskMpca, maskM, (size_t)n);
  rm_calc_normals(M, n, NM, maskM, maskMpca, SR);
  for (int i = 0; i < n; i++) phiM[i] = maskMpca[i] ? atan2(NM[2 * i + 1], NM[2 * i]) : -1e6;
  for (int i = SR; i < n - SR; i++) if (maskMpca[i]) idxMValid[nM++] = i;
  /* scene (:87-108) */
  memcpy(maskSpca, maskS, (size_t)n);
  unsigned validPoints = 0;
  for (int i = 0; i < n; i++) if (maskSpca[i]) validPoints++;
  double probability = 180.0 / (double)validPoints;
  if (probability < 0.99) {
    if (probability > 1.0) probability = 1.0;
    if (probability < 0.0) probability = 0.0;
    const int threshold = (int)(1000.0 - probability * 1000.0 + 0.5);
    for (int i = 0; i < n; i++) if ((draws_subsample[i] % 1000) < threshold) maskSpca[i] = 0;
  }
  rm_calc_normals(S, n, NS, maskS, maskSpca, SR);
  for (int i = 0; i < n; i++) phiS[i] = maskSpca[i] ? atan2(NS[2 * i + 1], NS[2 * i]) : -1e6;
  for (int i = SR; i < n - SR; i++) if (maskSpca[i]) idxSValid[nS++] = i;
  /* control set (:111-120) */
  int pointsInC = p->size_control_set < nS ? p->size_control_set : nS;
  double* Control = (double*)malloc(sizeof(double) * 2 * (size_t)(pointsInC > 0 ? pointsInC : 1));
  {
    int left = nS;
    memcpy(rest, idxSValid, sizeof(int) * (size_t)nS);
    for (int k = 0; k < pointsInC; k++) {
      const unsigned r = (unsigned)draws_control[k] % (unsigned)left;
      const int idx = rest[r];
      memmove(rest + r, rest + r + 1, sizeof(int) * (size_t)(left - (int)r - 1)); left--;
      Control[2 * k] = S[2 * idx]; Control[2 * k + 1] = S[2 * idx + 1];
    }
  }
  out_counts[1] = nM; out_counts[2] = nS; out_counts[3] = pointsInC;
  if (nS < 3 || nM < 3) { rc = 1; goto done; }                      /* :134-144 */
  {
    int trials = p->trials;
    if (nM < trials) trials = nM;
    double phiMax = p->phi_max < M_PI * 0.5 ? p->phi_max : M_PI * 0.5;
    int span;
    if (p->ang_res > 1e-6) { span = (int)floor(phiMax / p->ang_res); if (span > n) span = n; }
    else { rc = 2; goto done; }
    double bestProb = 0.0;
    for (int k = 0; k < nM; k++) {                                    /* :200-204 */
      const double x = M[2 * idxMValid[k]], y = M[2 * idxMValid[k] + 1];
      anglesArray[k] = atan2(y, x);
      distArray[k] = sqrt(pow(x, 2) + pow(y, 2));
    }
    int left = nM, cand = 0;
    memcpy(rest, idxMValid, sizeof(int) * (size_t)nM);
    for (int trial = 0; trial < trials; trial++) {
      const int r = (int)((unsigned)draws_trials[trial] % (unsigned)left);
      const int idx = rest[r];
      memmove(rest + r, rest + r + 1, sizeof(int) * (size_t)(left - r - 1)); left--;
      const int iMin = (idx - span > SR) ? idx - span : SR;
      const int iMax = (idx + span < n - SR) ? idx + span : n - SR;
      const double angleThresh = (M_PI / 180.0) * p->max_angle_diff;
      for (int i = iMin; i < iMax; i++) {
        if (!maskSpca[i]) continue;
        double phi = phiM[idx] - phiS[i];
        if (phi > M_PI) phi -= 2.0 * M_PI;
        else if (phi < -M_PI) phi += 2.0 * M_PI;
        if (!(fabs(phi) < phiMax)) continue;
        double T[9] = {cos(phi), -sin(phi), 0, sin(phi), cos(phi), 0, 0, 0, 1};
        const double sx = S[2 * i], sy = S[2 * i + 1];
        T[2] = M[2 * idx] - (T[0] * sx + T[1] * sy);
        T[5] = M[2 * idx + 1] - (T[3] * sx + T[4] * sy);
        int fieldOfViewCount = 0;
        double prod = 1.0;
        for (int s = 0; s < pointsInC; s++) {
          /* STemp = T * Control (dgemm: k ascending from 0.0) */
          double cx = 0.0, cy = 0.0;
          cx += T[0] * Control[2 * s]; cx += T[1] * Control[2 * s + 1]; cx += T[2] * 1.0;
          cy += T[3] * Control[2 * s]; cy += T[4] * Control[2 * s + 1]; cy += T[5] * 1.0;
          const double angle = atan2(cy, cx);
          const double distance = sqrt(pow(cx, 2) + pow(cy, 2));
          double minAngleDiff;
          const int k = pdfr_nearest(anglesArray, nM, angle, &minAngleDiff);
          if (minAngleDiff < angleThresh) fieldOfViewCount++;
          prod *= pdfr_prob(p, distArray[k], distance);
        }
        if (pointsInC == 0) prod = 0.0;                               /* probOfAllScans.size() == 0 */
        if (cand < cap) { ungated[cand] = prod; fov_out[cand] = fieldOfViewCount; }
        cand++;
        if ((prod > bestProb) && ((double)fieldOfViewCount > (double)(unsigned)pointsInC * p->percentage_points_in_c)) {
          memcpy(T_out, T, sizeof(T));
          bestProb = prod;
          out_counts[4] = idx; out_counts[5] = i;
        }
      }
    }
    *prob_out = bestProb;
    out_counts[0] = cand;
  }
done:
  free(NM); free(NS); free(phiM); free(phiS); free(maskMpca); free(maskSpca); free(idxMValid); free(idxSValid); free(rest);
  free(anglesArray); free(distArray); free(Control);
  return rc;
}
