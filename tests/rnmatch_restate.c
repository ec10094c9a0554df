/* rnmatch_restate.c -- an independent plain-C restatement of obvious::RandomNormalMatching::match (registration_mode 1;
 * registration/ransacMatching/RandomNormalMatching.cpp:67-395) with the three rand() streams as inputs, serial, in the reference's
 * statement order.  Test infrastructure: built by the tests (gcc -O2 -ffp-contract=off) into a temporary directory.
 * RandomMatching::calcNormals and the exact nearest-neighbour search (FLANN's kd-tree with eps = 0) are the oracle's (rm_calc_normals,
 * kd_build_rec / kd_search_rec: the lowest index among equal squared distances), not restated a third time.  The device scans the
 * model points by brute force; a kd-tree here cross-checks that both find the same neighbour. */
#include "../oracle/tsd_oracle.c"

/* the layout of tsd_rnmatch_params (include/tsd_hip.h) */
typedef struct {
  int trials, size_control_set;
  double eps_thresh, phi_max, ang_res;
} rnr_params;

/* Kuehn's rating (:344-359), one step against the running best; 1 if the candidate replaces it.  fabs() of the bool, as written. */
int rnr_rate(double ratio, unsigned int cntMatch, double errSum, double* bestRatio, unsigned int* bestCnt, double* bestErr)
{
  double equalThres = 1e-5;
  int rateCondition = ((ratio - *bestRatio) > equalThres) && (cntMatch > *bestCnt);
  int similarityCondition = fabs((ratio - *bestRatio) < equalThres) && (cntMatch == *bestCnt) && errSum < *bestErr;
  int goodMatch = rateCondition || similarityCondition;
  if (goodMatch) { *bestRatio = ratio; *bestCnt = cntMatch; *bestErr = errSum; }
  return goodMatch;
}

/* the serial fold over n candidates: the threshold test (:338), the ratio (:342), the rating; the winner's index or -1 */
int rnr_select(const int* cnt, const int* max_cnt, const double* err, int n, int thresh)
{
  double bestRatio = 0.0, bestErr = 1e12;
  unsigned int bestCnt = 0;
  int win = -1;
  for (int c = 0; c < n; c++) {
    const unsigned int cntMatch = (unsigned int)cnt[c], maxCntMatch = (unsigned int)max_cnt[c];
    if (cntMatch <= (unsigned int)thresh) continue;
    double ratio = (double)cntMatch / (double)maxCntMatch;
    if (rnr_rate(ratio, cntMatch, err[c], &bestRatio, &bestCnt, &bestErr)) win = c;
  }
  return win;
}

/* Returns 0, 1 (an early return: identity) or 2 (resolution not set: identity).  out_counts = {candidates, valid model, valid scene,
 * control points, idx, i, winner (candidate index), pad}; out_best = {bestRatio, bestErr}.  Per candidate (serial order, up to cap):
 * cntMatch, maxCntMatch, errSum and whether an in-view err lies within 1e-12 of 1.0. */
int rnr_match(const double* M, const uint8_t* maskM, const double* S, const uint8_t* maskS, int n, const rnr_params* p,
              const int* draws_subsample, const int* draws_control, const int* draws_trials, double T_out[9], double out_best[2],
              int out_counts[8], int* cnt_out, int* max_out, double* err_out, uint8_t* near_out, int cap)
{
  const int SR = 10 / 2;                                            /* _pcaSearchRange / 2 */
  const double scaleDistance = 1.0 / (p->eps_thresh * p->eps_thresh), scaleOrientation = 0.33;
  for (int i = 0; i < 9; i++) T_out[i] = (i % 4 == 0) ? 1.0 : 0.0;
  out_best[0] = 0.0; out_best[1] = 1e12;
  for (int i = 0; i < 8; i++) out_counts[i] = 0;
  out_counts[4] = out_counts[5] = out_counts[6] = -1;
  if (n < 3) return 1;                                              /* :88-92 */
  double* NM = (double*)calloc(2 * (size_t)n, sizeof(double));
  double* NS = (double*)calloc(2 * (size_t)n, sizeof(double));
  double* phiM = (double*)malloc(sizeof(double) * (size_t)n);
  double* phiS = (double*)malloc(sizeof(double) * (size_t)n);
  uint8_t* maskMpca = (uint8_t*)malloc((size_t)n);
  uint8_t* maskSpca = (uint8_t*)malloc((size_t)n);
  int* idxMValid = (int*)malloc(sizeof(int) * (size_t)n);
  int* idxSValid = (int*)malloc(sizeof(int) * (size_t)n);
  int* rest = (int*)malloc(sizeof(int) * (size_t)n);
  double* Mv = (double*)malloc(sizeof(double) * 2 * (size_t)n);
  int* kd_idx = (int*)malloc(sizeof(int) * (size_t)n);
  int* kd_axis = (int*)malloc(sizeof(int) * (size_t)n);
  int nM = 0, nS = 0, rc = 0;
  /* model (:94-114): normals, phi, extractSamples, the kd-tree over the valid points in idxMValid order */
  memcpy(maskMpca, maskM, (size_t)n);
  rm_calc_normals(M, n, NM, maskM, maskMpca, SR);
  for (int i = 0; i < n; i++) phiM[i] = maskMpca[i] ? atan2(NM[2 * i + 1], NM[2 * i]) : -1e6;
  for (int i = SR; i < n - SR; i++) if (maskMpca[i]) idxMValid[nM++] = i;
  for (int k = 0; k < nM; k++) { Mv[2 * k] = M[2 * idxMValid[k]]; Mv[2 * k + 1] = M[2 * idxMValid[k] + 1]; kd_idx[k] = k; }
  kdtree kd = {kd_idx, nM, Mv, kd_axis};
  kd_build_rec(&kd, 0, nM);
  /* scene (:118-138) */
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
  /* control set (:142-154): the points and calcPhi(NControl, NULL, phiControl) */
  int pointsInC = p->size_control_set < nS ? p->size_control_set : nS;
  double* Control = (double*)malloc(sizeof(double) * 2 * (size_t)(pointsInC > 0 ? pointsInC : 1));
  double* phiControl = (double*)malloc(sizeof(double) * (size_t)(pointsInC > 0 ? pointsInC : 1));
  {
    int left = nS;
    memcpy(rest, idxSValid, sizeof(int) * (size_t)nS);
    for (int k = 0; k < pointsInC; k++) {
      const unsigned r = (unsigned)draws_control[k] % (unsigned)left;
      const int idx = rest[r];
      memmove(rest + r, rest + r + 1, sizeof(int) * (size_t)(left - (int)r - 1)); left--;
      Control[2 * k] = S[2 * idx]; Control[2 * k + 1] = S[2 * idx + 1];
      phiControl[k] = atan2(NS[2 * idx + 1], NS[2 * idx]);
    }
  }
  const unsigned int cntMatchThresh = (unsigned int)pointsInC / 3;  /* :152 */
  out_counts[1] = nM; out_counts[2] = nS; out_counts[3] = pointsInC;
  if (nS < 3 || nM < 3) { rc = 1; goto done; }                      /* :165-175 */
  {
    const double thetaBoundMin = atan2(M[2 * idxMValid[0] + 1], M[2 * idxMValid[0]]);            /* :159-160 */
    const double thetaBoundMax = atan2(M[2 * idxMValid[nM - 1] + 1], M[2 * idxMValid[nM - 1]]);
    int trials = p->trials;
    if (nM < trials) trials = nM;
    double phiMax = p->phi_max < M_PI * 0.5 ? p->phi_max : M_PI * 0.5;
    int span;
    if (p->ang_res > 1e-6) { span = (int)floor(phiMax / p->ang_res); if (span > n) span = n; }
    else { rc = 2; goto done; }
    double bestRatio = 0.0, bestErr = 1e12;
    unsigned int bestCnt = 0;
    int left = nM, cand = 0;
    memcpy(rest, idxMValid, sizeof(int) * (size_t)nM);
    for (int trial = 0; trial < trials; trial++) {
      const int r = (int)((unsigned)draws_trials[trial] % (unsigned)left);
      const int idx = rest[r];
      memmove(rest + r, rest + r + 1, sizeof(int) * (size_t)(left - r - 1)); left--;
      const int iMin = (idx - span > SR) ? idx - span : SR;
      const int iMax = (idx + span < n - SR) ? idx + span : n - SR;
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
        unsigned int maxCntMatch = 0, cntMatch = 0;
        double errSum = 0;
        int near = 0;
        for (int s = 0; s < pointsInC; s++) {
          /* STemp = T * Control (dgemm: k ascending from 0.0) */
          double cx = 0.0, cy = 0.0;
          cx += T[0] * Control[2 * s]; cx += T[1] * Control[2 * s + 1]; cx += T[2] * 1.0;
          cy += T[3] * Control[2 * s]; cy += T[4] * Control[2 * s + 1]; cy += T[5] * 1.0;
          const double thetaControl = atan2(cy, cx);
          if (thetaControl > thetaBoundMax || thetaControl < thetaBoundMin) continue;   /* :274-282 */
          maxCntMatch++;
          const double q[2] = {cx, cy};
          int k = nM; double distConsensus = INFINITY;
          kd_search_rec(&kd, 0, nM, q, &k, &distConsensus);
          const int idxQuery = idxMValid[k];
          double normalConsensus = (1.0 - cos(phiM[idxQuery] - phiControl[s] - phi)) / 2.0;   /* :322 */
          double err = distConsensus * scaleDistance + normalConsensus * scaleOrientation;   /* :324 */
          errSum += err;
          if (err < 1.0) cntMatch++;
          if (fabs(err - 1.0) <= 1e-12) near = 1;
        }
        if (cand < cap) { cnt_out[cand] = (int)cntMatch; max_out[cand] = (int)maxCntMatch; err_out[cand] = errSum; near_out[cand] = (uint8_t)near; }
        cand++;
        if (cntMatch <= cntMatchThresh) continue;                   /* :338-339 */
        double ratio = (double)cntMatch / (double)maxCntMatch;      /* :342 */
        if (rnr_rate(ratio, cntMatch, errSum, &bestRatio, &bestCnt, &bestErr)) {
          memcpy(T_out, T, sizeof(T));
          out_counts[4] = idx; out_counts[5] = i; out_counts[6] = cand - 1;
        }
      }
    }
    out_best[0] = bestRatio; out_best[1] = bestErr;
    out_counts[0] = cand;
  }
done:
  free(NM); free(NS); free(phiM); free(phiS); free(maskMpca); free(maskSpca); free(idxMValid); free(idxSValid); free(rest);
  free(Mv); free(kd_idx); free(kd_axis); free(Control); free(phiControl);
  return rc;
}
