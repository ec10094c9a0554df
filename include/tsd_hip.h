/*
 * tsd_hip.h -- C ABI of the MI355X (gfx950) implementation of ohm_tsd_slam's per-scan hot path.
 *
 * This is the drop-in boundary: three device entry points (push / raycast / icp, plus the fused
 * localize) that replace the three places where the reference's worker threads enter the vendored
 * "obviously" library, with the TSD grid resident in HBM between calls.  Plain pointers and sizes
 * only; no C++/torch types.  Host pointers unless the name ends in _dev.  Every call returns
 * TSD_OK (0), a negative TSD_E* code (argument / HIP failure; text via tsd_last_error), or -- for the
 * registration calls -- fills `state` with the reference's EnumIcpState.  Nothing throws.
 *
 * Citations `file:line` are relative to the reference tree (autonohm/ohm_tsd_slam, src/).
 * A tsd_ctx serialises its work on one HIP stream; distinct contexts are independent (one grid per
 * GPU for the multi-robot case).  Calls on one ctx must not be issued concurrently from two threads
 * (the C++ facade in ohm_tsd_slam_amd/csrc/host serialises them with a mutex).
 */
#ifndef TSD_HIP_H
#define TSD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSD_OK            0
#define TSD_E_ARG        -1   /* bad argument (null pointer, size out of range) */
#define TSD_E_HIP        -2   /* a HIP runtime call failed; see tsd_last_error */
#define TSD_E_NODEVICE   -3   /* no usable gfx950 device */
#define TSD_E_BOUNDS     -4   /* freeFootprint rectangle outside the grid (TsdGrid.cpp:617-622) */
#define TSD_E_CAPACITY   -5   /* more beams / points than the kernels are built for */
#define TSD_E_NOMEM      -6   /* the device cannot hold a call's scratch (tsd_frontiers_*); see tsd_last_error */

#define TSD_TILE_DIM     32   /* SlamNode.cpp:77 hard-codes LAYOUT_32x32 */
#define TSD_TILE_PITCH   33   /* 32 cells + 1 halo (TsdGridPartition.cpp:97) */
#define TSD_TILE_CELLS   1089
#define TSD_MAX_BEAMS    4096 /* scan staged in LDS by the push kernel */
#define TSD_MAX_ICP_POINTS 2048 /* model/scene resident in LDS in the ICP kernel */
#define TSD_ICP_TRACE_MAX 256  /* iterations recorded by tsd_icp_trace */
#define TSD_ICP_TRACE_STRIDE 8 /* doubles per recorded iteration */

/* EnumIcpState (obvision/registration/icp/Icp.h:25-32) */
#define TSD_ICP_PROCESSING     1
#define TSD_ICP_NOTMATCHABLE   2
#define TSD_ICP_MAXITERATIONS  3
#define TSD_ICP_SUCCESS        5

typedef struct tsd_ctx tsd_ctx;

/* Work counters of one TsdGrid::push (TsdGrid.cpp:217-284); the terms of the algorithmic-bytes
 * formula of DESIGN.md are computed from these. */
typedef struct {
  int64_t cells_updated;        /* addTsd calls that passed sd >= -maxTruncation */
  int64_t cells_visited;        /* back-projected cells (1024 per UPDATE tile) */
  int32_t tiles_total;
  int32_t tiles_range_pass;     /* passed both range tests of isInRange */
  int32_t tiles_update;         /* isInRange() == true */
  int32_t tiles_new;            /* lazily initialised by this push */
  int32_t tiles_new_from_empty; /* ... of which _initWeight > 0 */
  int32_t tiles_emptied_init;   /* increaseEmptiness() on an initialised tile */
  int32_t tiles_emptied_uninit; /* increaseEmptiness() on an uninitialised tile */
} tsd_push_stats;

/* Registration set-up as ThreadLocalize builds it (ThreadLocalize.cpp:211-225, 571-581) */
/* estimator of Icp::step: the one the node constructs (ThreadLocalize.cpp:214) or the reference's other one */
#define TSD_ESTIMATOR_CLOSED_FORM   0  /* ClosedFormEstimator2D (ClosedFormEstimator2D.cpp:36-109), point to point */
#define TSD_ESTIMATOR_POINT_TO_LINE 1  /* PointToLine2DEstimator (PointToLineEstimator2D.cpp:52-157), needs model normals */

typedef struct {
  int    iterations;            /* icp_iterations: Icp max iterations == convergence counter */
  int    estimator;             /* TSD_ESTIMATOR_*; occupies what used to be padding: set it (0 = the node's choice) */
  double dist_filter_max;       /* DistanceFilter(maxdist, mindist, icp_iterations - 10) */
  double dist_filter_min;
  double min_x, max_x, min_y, max_y; /* OutOfBoundsFilter2D = TsdGrid::getMin/MaxX/Y */
  /* Tinit of Icp::iterate(rms, pairs, iterations, Tinit) (Icp.cpp:464-486): the pre-registration result in
   * registration_mode 1-3 (ThreadLocalize.cpp:531-569, :580), 3x3 row-major.  Used by tsd_icp / tsd_icp_normals when
   * use_t_init != 0 (0 = the identity of registration_mode 0); the fused calls always start from the identity. */
  double t_init[9];
  int    use_t_init;
  int    reserved;
} tsd_icp_params;

typedef struct {
  double T[9];                  /* Icp::getFinalTransformation() 3x3 row-major */
  double rms;                   /* estimator's "rms": mean squared pair distance (closed form) or mean |n.(s - m)| (point to line) */
  int32_t pairs;                /* pairs of the last step */
  int32_t iterations;           /* steps executed */
  int32_t state;                /* EnumIcpState */
  int32_t n_model;              /* valid model points (ray-cast hits)  -- tsd_localize only */
  int32_t n_scene;              /* valid scene points                  -- tsd_localize only */
  int32_t reserved;             /* < 0: a TSD_E_* code (TSD_E_CAPACITY: more points than the registration holds).  >= 0 (diagnostic): the
                                 * scene points whose first neighbour search was delivered by the helper workgroups of the launch
                                 * (0 with tsd_debug_set_icp_helpers(ctx, 0)); the results do not depend on it */
} tsd_icp_result;

/* ---- life cycle ------------------------------------------------------------------------------ */
int      tsd_device_count(void);
/* Free and total memory of `device` in bytes as the HIP runtime this library is linked against reports it (hipMemGetInfo): what a
 * caller sizes map_size against -- the node accepts up to 2^15 x 2^15 cells (SlamNode.cpp:71-75), 18.8 GB of fp64 cells here.
 * TSD_E_NODEVICE without such a device. */
int      tsd_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* new TsdGrid(cellSize, LAYOUT_32x32, map_size) + setMaxTruncation(max_trunc)
 * (SlamNode.cpp:77-78, TsdGrid.cpp:112-169, :206-215).  NULL on failure. */
tsd_ctx* tsd_create(int device, int map_size_log2, double cell_size, double max_trunc);
void     tsd_destroy(tsd_ctx* ctx);
int      tsd_reset(tsd_ctx* ctx);                          /* TsdGrid::reset (TsdGrid.cpp:194-198) */
int      tsd_set_max_truncation(tsd_ctx* ctx, double val); /* TsdGrid::setMaxTruncation (:206-215) */
int      tsd_sync(tsd_ctx* ctx);
int      tsd_device(const tsd_ctx* ctx);                   /* HIP device ordinal of the context */
void*    tsd_stream(tsd_ctx* ctx);                         /* its hipStream_t: work a host enqueues there is ordered with the grid's */
const char* tsd_last_error(const tsd_ctx* ctx);

/* sizeof() of a public struct of this header by name ("tsd_push_stats", "tsd_icp_params", ...; 0 if unknown): lets a
 * binding (ctypes, cgo, JNI) check its mirror of the layout at load time */
int      tsd_abi_sizeof(const char* struct_name);

/* ---- geometry getters (TsdGrid.h getCellsX, getCellSize, getMaxTruncation, getMinX.., getMaxX..) -- */
int    tsd_cells(const tsd_ctx* ctx);
int    tsd_tiles(const tsd_ctx* ctx);
double tsd_cell_size(const tsd_ctx* ctx);
double tsd_max_truncation(const tsd_ctx* ctx);
double tsd_min_x(const tsd_ctx* ctx);
double tsd_max_x(const tsd_ctx* ctx);
double tsd_min_y(const tsd_ctx* ctx);
double tsd_max_y(const tsd_ctx* ctx);

/* ---- map update ------------------------------------------------------------------------------ */
/* TsdGrid::freeFootprint (TsdGrid.cpp:609-638) */
int tsd_free_footprint(tsd_ctx* ctx, const double center[2], double width, double height);

/* TsdGrid::push(SensorPolar2D*) (TsdGrid.cpp:217-284): isInRange classification incl. the
 * increaseEmptiness side effect (TsdGridComponent.cpp:43-124), lazy tile init
 * (TsdGridPartition.cpp:88-134), addTsd (TsdGridPartition.h:170-212), propagateBorders
 * (TsdGrid.cpp:372-427).  `ranges`/`mask` are the sensor's PROCESSED data (after setStandardMask:
 * > max_range -> +inf, no NaN).  Asynchronous unless `stats` is non-NULL (then it waits and fills). */
int tsd_push(tsd_ctx* ctx, const double pose33[9], const double* ranges, const uint8_t* mask,
             int beams, double ang_res, double phi_min, double max_range, double min_range,
             double low_refl_range, tsd_push_stats* stats);

/* ---- localisation ---------------------------------------------------------------------------- */
/* RayCastPolar2D::calcCoordsFromCurrentViewMask (RayCastPolar2D.cpp:113-192).  rays_world_2xB is
 * Sensor::getNormalizedRayMap(cellSize): row 0 = x, row 1 = y of every beam's world ray of length
 * cellSize.  Outputs are in the sensor frame; only hit slots are written. */
int tsd_raycast(tsd_ctx* ctx, const double pose33[9], const double* rays_world_2xB, int beams,
                double min_range, double max_range, double* coords_2B, double* normals_2B,
                uint8_t* mask_B, int* n_valid);

/* Icp::reset + setModel + setScene + iterate + getFinalTransformation with the assigner/filter/
 * estimator chain of ThreadLocalize, registration_mode 0 (ThreadLocalize.cpp:571-581;
 * Icp.cpp:410-512; PairAssignment.cpp:38-84; ClosedFormEstimator2D.cpp:36-109).  `pose33` is the
 * sensor pose handed to OutOfBoundsFilter2D::setPose. */
int tsd_icp(tsd_ctx* ctx, const double* model_xy, int n_model, const double* scene_xy, int n_scene,
            const double pose33[9], const tsd_icp_params* params, tsd_icp_result* result);
/* The same with the model normals Icp::setModel(coords, normals) takes (Icp.cpp:150-203); required by
 * TSD_ESTIMATOR_POINT_TO_LINE, ignored by the closed form.  tsd_localize / tsd_scan use the ray cast's normals. */
int tsd_icp_normals(tsd_ctx* ctx, const double* model_xy, const double* model_normals_xy, int n_model,
                    const double* scene_xy, int n_scene, const double pose33[9], const tsd_icp_params* params,
                    tsd_icp_result* result);

/* Fused body of ThreadLocalize::eventLoop between setStandardMask and isRegistrationError
 * (ThreadLocalize.cpp:353-377): ray cast -> dataToCartesianVectorMask -> maskMatrix compaction ->
 * doRegistration, without leaving the device.  rays_local_2xB = Sensor::_raysLocal.  params->t_init (use_t_init != 0) is the
 * Tinit of Icp::iterate (Icp.cpp:481-486), applied while the device stages the scene: registration_mode 3 hands its
 * pre-registration result over this way (csrc/host/ThreadLocalize.cpp: processScanPreRegistered). */
int tsd_localize(tsd_ctx* ctx, const double pose33[9], const double* rays_world_2xB,
                 const double* rays_local_2xB, const double* ranges, const uint8_t* mask, int beams,
                 double min_range, double max_range, const tsd_icp_params* params,
                 tsd_icp_result* result);

/* ---- relocalisation: where in this grid was this scan taken? ------------------------------------------------ */
#define TSD_RELOC_MAX_PEAKS      64          /* start poses handed to the refinement at most */
#define TSD_RELOC_MAX_CANDIDATES (1 << 26)   /* nx * ny * ntheta at most: a 256 MiB score volume */
#define TSD_RELOC_MAX_REACH      4           /* grid widths a lattice position may lie outside the grid, and a scan point from the sensor */
/* The pose lattice of the search and what is done with its peaks.  Candidate (ix, iy, k) stands for the sensor pose at
 * (x0 + (double)ix * step_xy, y0 + (double)iy * step_xy) turned by rotation k; its index is idx = (k * ny + iy) * nx + ix. */
typedef struct {
  double  x0, y0, step_xy;      /* world coordinates of node (0, 0) and the node spacing (> 0), metres.  Every node within
                                 * TSD_RELOC_MAX_REACH grid widths of the grid's square (TSD_E_ARG beyond): the cell index of a carried
                                 * point then fits an int */
  int32_t nx, ny, ntheta;       /* nodes per axis, each >= 1; nx * ny * ntheta <= TSD_RELOC_MAX_CANDIDATES (TSD_E_CAPACITY beyond) */
  int32_t theta_wraps;          /* != 0: the rotations cover the full circle, k = 0 and k = ntheta - 1 are neighbours */
  const double* cos_sin;        /* [2 * ntheta]: cos, sin of rotation k at [2k], [2k + 1].  NULL: the host fills the table with libm's
                                 * cos / sin of theta0 + (double)k * dtheta (dtheta finite and != 0, else TSD_E_ARG).  The device never
                                 * computes a sine: a restatement on the same table is bit-comparable */
  double  theta0, dtheta;       /* read with cos_sin == NULL only */
  int32_t K;                    /* peaks to refine, 1 .. TSD_RELOC_MAX_PEAKS */
  int32_t min_pairs;            /* found = the winner's pairs >= min_pairs (>= 0) */
} tsd_reloc_params;
typedef struct {
  int32_t  found;               /* the winner's registration ended with at least min_pairs pairs (0 without a peak) */
  int32_t  winner_idx;          /* candidate index of the winning peak, -1 when the search found no peak */
  double   pose33[9];           /* found: winner's coarse pose * T, 3x3 row-major (the sensor pose of the scan); NaN otherwise */
  double   coarse_x, coarse_y, coarse_cos, coarse_sin;   /* the winning peak's lattice pose (NaN without a peak) */
  uint32_t winner_score;        /* its score (0 without a peak) */
  int32_t  n_peaks;             /* peaks the search returned, <= K */
  int32_t  n_refined;           /* ... of which were refined (all of them unless a registration call failed) */
  int32_t  reserved;
  tsd_icp_result icp;           /* the winner's registration, as tsd_localize fills it (zero without a peak) */
  double   search_ms, refine_ms;/* tsd_profile_enable(ctx, 1): stream time of the search (scores + peaks) and of the refinement's
                                 * launches and copies, from HIP events around them; 0 otherwise */
} tsd_reloc_result;
/* Global localisation of one scan in the grid as it is: a dense search over the pose lattice, then the registration from its best peaks.
 *
 * Score of a candidate (k_reloc_score; fp64 in the written order, no contraction): with t = its position and (c, s) its rotation, 0 unless
 * TsdGrid::interpolateBilinear (TsdGrid.h:284-304) at t succeeds with a value > 0 (the sensor stands in seen free space; nothing else is
 * looked up otherwise).  Else the sum over the P points (px, py) of 1048576 - (uint32)rint(fabs(v) * 1048576.0), v the look-up at
 * ((c*px - s*py) + t.x, (s*px + c*py) + t.y), over the look-ups that succeed (outside the grid, uninitialised tile, NaN: 0).  A sum of
 * integers in uint32: independent of the order of summation.  The cells are taken to hold what a push writes, |tsd| <= 1 (or NaN): a term
 * is then 0 .. 2^20 and the sum of TSD_MAX_ICP_POINTS of them fits.  For cells of |tsd| >= 4096, which only tsd_upload_tiles can leave,
 * the conversion to uint32 is undefined and the score is unspecified; nothing else is affected.
 * Peaks (k_reloc_peaks): a candidate with score > 0 that beats each of its up to 26 lattice neighbours n (k wraps when theta_wraps):
 * score > score_n, or score == score_n and idx < idx_n.  The K best by score descending, then idx ascending.
 * Refinement: for each peak in that order the unfused localisation of tsd_localize from the peak's pose [[c, -s, tx], [s, c, ty], [0, 0, 1]]
 * with rays_world = R * rays_local (Sensor::transform, Sensor.cpp:50-55: (0 + c*x) + (-s)*y, (0 + s*x) + c*y) scaled by cellSize
 * (Sensor::getNormalizedRayMap, Sensor.cpp:36-48) and icp_params as given.  The winner is IcpMultiInitIterator's
 * (IcpMultiInitIterator.cpp:26-38): strictly more pairs replace the best so far, so the earlier peak keeps a tie.  pose33 = coarse * T.
 *
 * points_xy: the P valid scan points in the sensor frame (x0 y0 x1 y1 ..), what Sensor::dataToCartesianVectorMask leaves after the
 * mask's compaction; 1 <= P (TSD_E_ARG) <= TSD_MAX_ICP_POINTS (TSD_E_CAPACITY), each coordinate finite and within TSD_RELOC_MAX_REACH grid
 * widths of the sensor (TSD_E_ARG).  rays_local_2xB / ranges / mask / beams /
 * min_range / max_range / icp_params: the scan as tsd_localize takes it.  The search only reads the grid: no cell, no tile flag, none of the
 * push or map-publication bookkeeping and no sensor is touched; the refinement uses the context's ray-cast and registration buffers like
 * tsd_localize.  Refused with TSD_E_ARG while a scan of this context is in flight (tsd_scan_submit / tsd_scan_begin / tsd_batch_begin without
 * their collect): it is not ordered against one silently.  Waits for its result.  Every argument is checked before the context is
 * touched: a refused call allocates nothing.
 * Memory: the score volume (4 bytes per candidate) stays with the context for the next search and for tsd_debug_reloc_scores as long as it
 * holds at most 2^23 candidates (32 MiB); a larger one is freed before the call returns.  tsd_destroy frees what is kept. */
int tsd_relocalize(tsd_ctx* ctx, const tsd_reloc_params* params, const double* points_xy, int P, const double* rays_local_2xB,
                   const double* ranges, const uint8_t* mask, int beams, double min_range, double max_range,
                   const tsd_icp_params* icp_params, tsd_reloc_result* result);
/* TEST HOOK: the score volume of the last tsd_relocalize of this context, scores[idx].  Copies min(n, cap) entries and returns
 * n = nx * ny * ntheta of that search: 0 before the first one and after a search of more than 2^23 candidates, whose volume is not
 * kept.  TSD_E_ARG without a context, TSD_E_HIP when the copy fails. */
int tsd_debug_reloc_scores(tsd_ctx* ctx, uint32_t* scores, int cap);
/* TEST HOOK: the device's peak selection on a given volume scores[(k * ny + iy) * nx + ix]: the K (1 .. TSD_RELOC_MAX_PEAKS) best peaks in
 * idx_out / score_out [K], their number in *n_out.  Leaves the volume of the last search alone.  TSD_OK; TSD_E_ARG for a null
 * pointer, a shape below 1, K outside its range or a scan of the context in flight (as tsd_relocalize); TSD_E_CAPACITY for a volume
 * above TSD_RELOC_MAX_CANDIDATES; TSD_E_HIP when an allocation, a copy or a launch fails. */
int tsd_debug_reloc_peaks(tsd_ctx* ctx, const uint32_t* scores, int nx, int ny, int ntheta, int theta_wraps, int K,
                          int32_t* idx_out, uint32_t* score_out, int* n_out);

/* ---- pre-registration (registration_mode 3) ------------------------------------------------------------- */
/* obvious::TSD_PDFMatching(grid, trials, epsThresh, sizeControlSet, zrand) (TSD_PDFMatching.cpp:6-26; ThreadLocalize.cpp:193)
 * and the arguments of its match() that are not point sets (ThreadLocalize.cpp:559) */
typedef struct {
  int    trials;                /* "trials" (ThreadLocalize.cpp:105), default 100 */
  int    size_control_set;      /* "sizeControlSet" (:106), default 140 */
  double eps_thresh;            /* "epsThresh" (:107); only sets _scaleDistance, which match() never reads */
  double zrand;                 /* "zrand" (:112): clipped probability of a control point without a valid look-up */
  double phi_max;               /* deg2rad("ransac_phi_max"), capped at pi/2 inside (TSD_PDFMatching.cpp:163) */
  double ang_res;               /* sensor->getAngularResolution() */
} tsd_tsdpdf_params;
typedef struct {
  double T[9];                  /* TBest, 3x3 row-major (identity when nothing scored above 0) */
  double probability;           /* bestProb */
  int32_t idx_model, idx_scene; /* the winning pair (beam indices), -1 if none */
  int32_t candidates;           /* (trial, i) pairs scored */
  int32_t valid_model, valid_scene, control_points;   /* idxMValid.size(), idxSValid.size(), Control->getCols() */
  int32_t reserved;
} tsd_tsdpdf_result;
/* obvious::TSD_PDFMatching::match(TSensor, M, maskM, NULL, S, maskS, phiMax, transMax, resolution)
 * (TSD_PDFMatching.cpp:31-294).  model / scene are beam-indexed (beams x 2, row-major) with their masks, exactly what
 * ThreadLocalize builds from _modelCoords / _scene (ThreadLocalize.cpp:367-369).  The reference draws from rand() in
 * three places; here the raw rand() values are inputs: draws_subsample[beams] (RandomMatching::subsampleMask,
 * RandomMatching.cpp:176-189: one per beam, consumed only when 180 / validScenePoints < 0.99), draws_control
 * [size_control_set] (RandomMatching::pickControlSet, :65), draws_trials[trials] (TSD_PDFMatching.cpp:190-194).  Trials
 * are evaluated in trial order (the reference's OpenMP loop leaves the order to the scheduler): the first candidate
 * that reaches the best probability wins.  Scoring runs on the device against the grid in HBM. */
int tsd_tsdpdf_match(tsd_ctx* ctx, const double pose33[9], const double* model_xy_2B, const uint8_t* mask_m,
                     const double* scene_xy_2B, const uint8_t* mask_s, int beams, const tsd_tsdpdf_params* params,
                     const int* draws_subsample, const int* draws_control, const int* draws_trials,
                     tsd_tsdpdf_result* result);

/* ---- pre-registration (registration_mode 2) ------------------------------------------------------------- */
/* obvious::PDFMatching(trials, epsThresh, sizeControlSet, zhit, zphi, zshort, zmax, zrand, percentagePointsInC, rangemax,
 * sigphi, sighit, lamshort, maxAngleDiff, maxAnglePenalty) (PDFMatching.cpp:9-40; ThreadLocalize.cpp:185-187) and the
 * arguments of its match() that are not point sets (ThreadLocalize.cpp:547) */
typedef struct {
  int    trials;                  /* "trials" */
  int    size_control_set;        /* "sizeControlSet" */
  double eps_thresh;              /* "epsThresh"; only sets _scaleDistance, which match() never reads */
  double zhit, zphi, zshort, zmax, zrand;   /* mixture weights of probabilityOfTwoSingleScans (PDFMatching.cpp:435-487) */
  double percentage_points_in_c;  /* "percentagePointsInC": share of the control set that has to be in view (:373) */
  double rangemax;                /* "rangemax" */
  double sigphi, sighit, lamshort;
  double max_angle_diff;          /* "maxAngleDiff", degrees: a control point is in view within this of a model beam (:227, :339) */
  double max_angle_penalty;       /* "maxAnglePenalty"; match() never reads it */
  double phi_max;                 /* deg2rad("ransac_phi_max"), capped at pi/2 inside (:159) */
  double ang_res;                 /* sensor->getAngularResolution() */
} tsd_pdfmatch_params;
/* obvious::PDFMatching::match(M, maskM, NULL, S, maskS, phiMax, transMax, resolution) (PDFMatching.cpp:47-432): the same
 * beam-indexed inputs and rand() streams as tsd_tsdpdf_match (the front end is shared), no grid and no sensor pose: the
 * control set is scored in the sensor frame against the model's polar angles and ranges.  T is TBest (identity on the
 * reference's early returns: too few points, too few valid points, resolution <= 1e-6); `probability` is the winning
 * product, counts as in tsd_tsdpdf_result.  Scoring and arg-max run on the device. */
int tsd_pdf_match(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B,
                  const uint8_t* mask_s, int beams, const tsd_pdfmatch_params* params, const int* draws_subsample,
                  const int* draws_control, const int* draws_trials, tsd_tsdpdf_result* result);
/* TEST HOOK: the last tsd_pdf_match's per-candidate values in candidate order (the reference's serial trial / i order):
 * the product over the control set before the field-of-view gate and the field-of-view count.  Copies min(n, cap) entries
 * and returns n (0 when the last pre-registration call on this context scored nothing or was a tsd_tsdpdf_match). */
int tsd_debug_pdf_match_scores(tsd_ctx* ctx, double* prob_ungated, int* fov, int cap);

/* ---- pre-registration (registration_mode 1) ------------------------------------------------------------- */
/* obvious::RandomNormalMatching(trials, epsThresh, sizeControlSet) (RandomNormalMatching.cpp:19-28; ThreadLocalize.cpp:183:
 * the shared "trials", "epsThresh", "sizeControlSet", not the ransac_* ones) and the arguments of its match() that are not
 * point sets (ThreadLocalize.cpp:537) */
typedef struct {
  int    trials;                  /* "trials" */
  int    size_control_set;        /* "sizeControlSet" */
  double eps_thresh;              /* "epsThresh": _scaleDistance = 1 / (epsThresh * epsThresh) */
  double phi_max;                 /* deg2rad("ransac_phi_max"), capped at pi/2 inside (:190) */
  double ang_res;                 /* sensor->getAngularResolution() */
} tsd_rnmatch_params;
typedef struct {
  double T[9];                  /* TBest, 3x3 row-major (identity when no candidate was accepted) */
  double ratio;                 /* bestRatio = cntMatch / maxCntMatch of the winner (0 if none) */
  double err_sum;               /* bestErr: the winner's errSum (1e12 if none) */
  int32_t cnt_match, max_cnt_match;   /* the winner's counts (0 if none) */
  int32_t idx_model, idx_scene; /* the winning pair (beam indices), -1 if none */
  int32_t candidates;           /* (trial, i) pairs scored */
  int32_t valid_model, valid_scene, control_points;   /* idxMValid.size(), idxSValid.size(), Control->getCols() */
  int32_t reserved[2];
} tsd_rnmatch_result;
/* obvious::RandomNormalMatching::match(M, maskM, NULL, S, maskS, phiMax, transMax, resolution)
 * (RandomNormalMatching.cpp:67-395): the same beam-indexed inputs and rand() streams as tsd_pdf_match (the front end is
 * shared).  Each candidate carries the control set through T and rates it by the exact nearest valid model point (L2, ties to
 * the lowest position in idxMValid) and the normal consensus; the winner is Kuehn's rating folded in the reference's serial
 * (trial, i) order (:344-359).  T is TBest (identity on the reference's early returns and when nothing is accepted).  Scoring
 * and selection run on the device. */
int tsd_rn_match(tsd_ctx* ctx, const double* model_xy_2B, const uint8_t* mask_m, const double* scene_xy_2B,
                 const uint8_t* mask_s, int beams, const tsd_rnmatch_params* params, const int* draws_subsample,
                 const int* draws_control, const int* draws_trials, tsd_rnmatch_result* result);
/* TEST HOOK: the last tsd_rn_match's per-candidate values in candidate order: cntMatch (before the cntMatchThresh test),
 * maxCntMatch (control points in view) and errSum.  Copies min(n, cap) entries and returns n (0 when the last
 * pre-registration call on this context scored nothing or was not a tsd_rn_match). */
int tsd_debug_rn_match_scores(tsd_ctx* ctx, int* cnt, int* max_cnt, double* err_sum, int cap);
/* TEST HOOK: the device selection of tsd_rn_match on given arrays of n candidates (serial order): the index of the winner
 * of Kuehn's rating among those with cnt > thresh in *winner (-1 if none).  Returns TSD_OK. */
int tsd_debug_rn_select(tsd_ctx* ctx, const int* cnt, const int* max_cnt, const double* err_sum, int n, int thresh, int* winner);

/* ---- fused scan: ThreadLocalize::eventLoop + ThreadMapping push without a host round trip ------------ */
/* Device-resident mirror of one robot's obvious::SensorPolar2D (pose, world / local ray maps) and of
 * ThreadLocalize's pose bookkeeping (_lastPose).  Several sensors may share one grid context
 * (multi-robot mode, SlamNode.cpp:101-122). */
typedef struct tsd_sensor tsd_sensor;

/* gates of ThreadLocalize: isRegistrationError(T, reg_trs_max, reg_sin_rot_max) (ThreadLocalize.cpp:593-600)
 * and isPoseChangeSignificant (:728-736) with TRNS_MIN / ROT_MIN (ThreadLocalize.h:63-64) */
typedef struct {
  double reg_trs_max, reg_sin_rot_max;
  double trs_min, rot_min;
} tsd_gate_params;

typedef struct {
  tsd_icp_result icp;           /* as tsd_localize */
  double pose[9];               /* sensor pose after this scan (unchanged on reg_error / no_model) */
  int32_t reg_error;            /* isRegistrationError: pose kept, caller publishes the NaN pose */
  int32_t pushed;               /* isPoseChangeSignificant: the scan was integrated into the grid */
  int32_t no_model;             /* ray cast found no model points: scan skipped (ThreadLocalize.cpp:354-358) */
  int32_t reserved;
} tsd_scan_result;

/* new SensorPolar2D(beams, ang_res, phi_min, max_range, min_range, low_refl_range) (ThreadLocalize.cpp:498) */
tsd_sensor* tsd_sensor_create(tsd_ctx* ctx, int beams, double ang_res, double phi_min, double max_range,
                              double min_range, double low_refl_range);
void tsd_sensor_destroy(tsd_sensor* s);
/* Upload the sensor state after ThreadLocalize::init (pose, Sensor::getNormalizedRayMap(cellSize), local
 * rays); forgets _lastPose. */
int tsd_sensor_set_pose(tsd_sensor* s, const double pose33[9], const double* rays_world_2xB,
                        const double* rays_local_2xB);
/* One scan: ray cast -> registration -> isRegistrationError -> Sensor::transform ->
 * isPoseChangeSignificant -> TsdGrid::push, all in stream order on the device (the body of
 * ThreadLocalize::eventLoop, ThreadLocalize.cpp:353-406, plus ThreadMapping::eventLoop's push,
 * ThreadMapping.cpp:51-56).  `ranges` / `mask` are the processed scan (setStandardMask), `mask_push` is
 * the mask of the copy ThreadMapping::queuePush makes (ThreadMapping.cpp:65-76; NULL = same mask).
 * Returns as soon as the result record is there (the device writes it to pinned host memory right
 * after the gates); the push of this scan may still be running and is ordered before anything enqueued
 * later on this context.  tsd_sync() waits for it. */
int tsd_scan(tsd_sensor* s, const double* ranges, const uint8_t* mask, const uint8_t* mask_push,
             const tsd_icp_params* params, const tsd_gate_params* gates, tsd_scan_result* result);

/* tsd_scan in two halves, and the NEXT scan staged ahead.  tsd_scan = tsd_scan_submit + tsd_scan_collect.  Between the two a
 * caller that already holds the next scan (a queued LaserScan; a replayed log) hands it to tsd_scan_stage: its copy and the
 * range-query tables of its push run on the side stream while the current registration is busy, and the next
 * tsd_scan_submit(s, NULL, NULL, NULL, ...) starts from the staged data -- the host's per-scan work no longer sits between
 * the ray cast and the registration.  A staged scan that is not the one that comes next is dropped by passing the real one. */
int tsd_scan_submit(tsd_sensor* s, const double* ranges /* NULL: the staged scan */, const uint8_t* mask, const uint8_t* mask_push,
                    const tsd_icp_params* params, const tsd_gate_params* gates);
int tsd_scan_stage(tsd_sensor* s, const double* ranges, const uint8_t* mask, const uint8_t* mask_push /* may be NULL: = mask */);
int tsd_scan_collect(tsd_sensor* s, tsd_scan_result* result);

/* The same scan in two halves for several robots on ONE grid (the reference's multi-robot mode, SlamNode.cpp:101-122),
 * one calling thread per SENSOR.  tsd_scan_begin enqueues copy, tables, ray cast and registration (+ gates,
 * Sensor::transform) on the sensor's own stream and buffers; tsd_scan_wait blocks the calling thread until the result
 * record is there; tsd_scan_finish (which waits itself if need be) enqueues the push on the grid's stream and returns
 * the result.  Registrations of different robots overlap (each occupies one compute unit and does not touch the grid); a
 * ray cast waits for the grid writes enqueued before it and a push for the ray casts enqueued before it, in the order
 * the calls reach their short, internally locked ordered sections -- pushes are serialised, like the reference's single
 * ThreadMapping does, and no ray cast ever sees a half-written tile.  These calls may be issued concurrently for
 * different sensors of one grid; one scan per sensor in flight.  For calls issued in turn the results are those of
 * tsd_scan. */
int tsd_scan_begin(tsd_sensor* s, const double* ranges, const uint8_t* mask, const uint8_t* mask_push,
                   const tsd_icp_params* params, const tsd_gate_params* gates);
int tsd_scan_wait(tsd_sensor* s);
int tsd_scan_finish(tsd_sensor* s, tsd_scan_result* result);

/* Batched form for several robots on ONE grid: the robots that have a scan pending are registered by ONE launch of each kernel
 * (tables: workgroup = scan; ray cast: block row = sensor; registration: workgroup = robot, one compute unit each) on the
 * batch's own stream, their pushes follow one after the other on the grid's stream.  All ray casts of a batch read the same
 * grid state, the pushes are applied in the order of the batch -- one of the interleavings the reference's N ThreadLocalize
 * workers and its single ThreadMapping can produce (SlamNode.cpp:101-122, ThreadMapping.cpp:47-75).  A caller keeps two or
 * three batches and uses them in turn: while one registers, the other's pushes run.
 *   tsd_batch_begin    copy, tables, ray casts, registrations (+ gates, Sensor::transform) of n sensors; returns at once
 *   tsd_batch_push     enqueue the n pushes (gated on the device); may be called BEFORE the registrations have finished: ray
 *                      casts enqueued later wait for these pushes, ray casts enqueued earlier do not
 *   tsd_batch_poll     1 when every result record of the batch has arrived, 0 otherwise (never blocks)
 *   tsd_batch_results  waits for the records, enqueues the pushes unless tsd_batch_push did, fills results[0..n), frees the slot
 * The sensors of a batch must be distinct, attached to the batch's grid and without a scan in flight; one estimator per batch.
 * Hand-offs inside a batch (ray casts -> registrations, a robot's registration -> its push) are waits on the device (a flag set by
 * a one-wave kernel behind the ray casts; a one-wave gate kernel ahead of each push) ONLY where tsd_batch_create's start-up probe has
 * shown that kernels of the two streams involved run side by side (not a given: HIP maps streams onto a few in-order hardware queues,
 * profilers and blocking launches serialise dispatches); otherwise stream events.  TSD_BATCH_EVENT_WAIT=1 forces events.
 * Failure contract (the reference's: "failures are logged and the scan is skipped", ThreadLocalize.cpp:354-358, :381-387): a
 * device-side wait is bounded, and one that runs out does NOT register or push on stale data -- the robots concerned get
 * tsd_scan_result.reserved = 1 (timeout) / 2 (batch abandoned), pose and grid untouched, and tsd_batch_results (or the next
 * tsd_batch_* call on the slot, for a push gate) returns TSD_E_HIP with tsd_last_error() saying so; the slot then uses events, and
 * slot and sensors stay usable. */
#define TSD_BATCH_MAX_SCANS 64
typedef struct tsd_batch tsd_batch;
tsd_batch* tsd_batch_create(tsd_ctx* ctx, int max_scans);
void tsd_batch_destroy(tsd_batch* b);
int tsd_batch_capacity(const tsd_batch* b);
int tsd_batch_inflight(const tsd_batch* b);      /* scans begun and not yet collected */
int tsd_batch_begin(tsd_batch* b, int n, tsd_sensor* const* sensors, const double* const* ranges, const uint8_t* const* mask,
                    const uint8_t* const* mask_push /* NULL or per-scan NULL: = mask */, const tsd_icp_params* params /* [n] */,
                    const tsd_gate_params* gates /* [n] */);
int tsd_batch_push(tsd_batch* b);
int tsd_batch_poll(tsd_batch* b);
int tsd_batch_results(tsd_batch* b, tsd_scan_result* results /* [n] */);

/* Per-iteration record of the most recent tsd_icp / tsd_localize on this ctx (the role of
 * Icp::activateTrace, Icp.cpp:60-70): out[TSD_ICP_TRACE_STRIDE * i + {0..7}] = pairs, rms, DistanceFilter threshold
 * before the step, state after loop control, and the step's Tlast = [[c, -s, tx], [s, c, ty]] as c, s, tx, ty (NaN
 * when the step had too few pairs to estimate), for i < min(iterations, max_iters). */
int tsd_icp_trace(tsd_ctx* ctx, double* out, int max_iters);

/* Parity / debug entry: the pair lists of the first `calls` PairAssignment::determinePairs calls (PairAssignment.cpp:38-84: exact
 * 1-NN, then DistanceFilter.cpp:32-64 with its threshold schedule for params->iterations, then ReciprocalFilter.cpp:32-78) on a
 * STATIC scene -- the scene is not moved between the calls -- as the registration kernel itself forms them (the same code path as
 * tsd_icp: tiers of the exact NN search, LDS atomic-min reciprocal filter; a dedicated instantiation writes the winners out).
 * n_pairs[k] pairs of call k at model_idx / scene_idx[k * n_scene + i], in ascending model index like the reference's output.
 * This is what tests/golden/ref_chain_pairs.npz holds from the COMPILED reference, so the HIP filter chain is pinned to it directly. */
int tsd_icp_pairs(tsd_ctx* ctx, const double* model_xy, int n_model, const double* scene_xy, int n_scene, const double pose33[9],
                  const tsd_icp_params* params, int calls, int* n_pairs /* [calls] */, int* model_idx /* [calls * n_scene] */,
                  int* scene_idx /* [calls * n_scene] */);

/* ---- map I/O --------------------------------------------------------------------------------- */
/* Canonical dump / restore of the tile state: initialized[tiles], init_weight[tiles],
 * tsd[tiles][1089], weight[tiles][1089] (uninitialised tiles read back NaN / 0).  Logical content of
 * TsdGrid::storeGrid / file ctor (TsdGrid.cpp:25-110, 548-607) plus the halo. */
int tsd_download_tiles(tsd_ctx* ctx, uint8_t* initialized, double* init_weight, double* tsd,
                       double* weight);
int tsd_upload_tiles(tsd_ctx* ctx, const uint8_t* initialized, const double* init_weight,
                     const double* tsd, const double* weight);
/* Digest of that canonical dump without moving it: an order-free 64-bit hash over (tile flag, initWeight, the bit
 * patterns of every cell's tsd and weight of the initialised tiles, halo included; NaN and -0.0 canonicalised), the
 * number of non-NaN cells and the sums of tsd / weight over them (per tile, then in tile order).  The hash of the
 * oracle's dump is computed by the same rule (oracle/tsd_oracle.c: ora_grid_digest); tests/golden pins it for
 * BASELINE configs 1-3. */
typedef struct {
  uint64_t hash;
  int64_t  cells_valid;
  int32_t  tiles_initialized;
  int32_t  reserved;
  double   sum_tsd, sum_weight;
} tsd_grid_digest_t;
int tsd_grid_digest(tsd_ctx* ctx, tsd_grid_digest_t* out);
/* bits per stored cell value of this build: 64 (fp64 like the reference, cells bit-identical to the oracle's) or 32
 * (libtsd_hip_q32.so: fixed point, 8 bytes per cell; within n * 2^-27 of the fp64 result after n pushes) */
int tsd_storage_bits(void);
/* tile flags only (cheap) */
int tsd_download_tile_state(tsd_ctx* ctx, uint8_t* initialized, double* init_weight);
/* TsdGrid::storeGrid(path) (TsdGrid.cpp:548-607) and the file constructor TsdGrid(path, FILE_SOURCE) (:25-110): the
 * reference's text format (one value per line, 6 significant digits; per tile its identifier and, for content
 * tiles, tsd and weight of the 32 x 32 interior cells).  Loading replaces the grid's content; the file's layout and
 * cell size must be the context's (TSD_E_ARG otherwise), its maxTruncation is taken over. */
int tsd_store_grid_text(tsd_ctx* ctx, const char* path);
int tsd_load_grid_text(tsd_ctx* ctx, const char* path);

/* Occupancy map of ThreadGrid::eventLoop (ThreadGrid.cpp:72-118) built from
 * RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105): int8 cells*cells,
 * -1 unknown / 0 free / 100 occupied.  The map persists inside the ctx between calls like
 * ThreadGrid::_occGridContent: -1 at tsd_create, and cleared by nothing afterwards (tsd_reset, tsd_upload_tiles and
 * tsd_load_grid_text replace the grid, not this map -- TsdGrid::reset does not touch ThreadGrid's copy either).  The _dev form writes to a device pointer (e.g. a torch tensor that is
 * then max-all-reduced over RCCL). */
int tsd_occupancy(tsd_ctx* ctx, int8_t* occ_host, int inflate, int inflate_factor, int* n_surface);
int tsd_occupancy_dev(tsd_ctx* ctx, void* occ_dev, int inflate, int inflate_factor);
/* the same without the final wait: the extraction kernels are only enqueued on the context's stream (what the RCCL
 * merge of include/tsd_comm.h puts its all-reduce behind) */
int tsd_occupancy_dev_async(tsd_ctx* ctx, void* occ_dev, int inflate, int inflate_factor);
/* TsdGrid::grid2ColorImage(image, width, height) (TsdGrid.cpp:429-488): RGB8, rgb[3 * (h * width + w)], the debug
 * image ThreadGrid publishes with every occupancy map (ThreadGrid.cpp:119-131).  Host buffer of 3*width*height. */
int tsd_color_image(tsd_ctx* ctx, uint8_t* rgb_host, unsigned int width, unsigned int height);

/* ThreadGrid's publication (ThreadGrid.cpp:72-131) as one asynchronous frame: the occupancy map of tsd_occupancy (same rules, same
 * persistent map, int8 cells*cells) and, unless rgb_host is NULL, the image of tsd_color_image(cells, cells) (RGB8, 3*cells*cells
 * bytes), built from one read of each tile.  begin returns once the work is enqueued: the frame reflects every push enqueued on the
 * context before the call, and its copies to the host leave on a stream of their own, so the scans enqueued after it do not wait for
 * them.  The host buffers must stay valid until tsd_map_frame_wait returns; pinned buffers (tsd_host_alloc) keep begin from blocking.
 * One frame may be in flight per context: a second begin fails with TSD_E_ARG.  wait blocks until the frame is on the host and
 * gives its surface count (calcCoords' mapSize / 2). */
typedef struct {
  int32_t inflate;              /* use_object_inflation */
  int32_t inflate_factor;       /* object_inflation_factor */
} tsd_map_params;
int tsd_map_frame_begin(tsd_ctx* ctx, const tsd_map_params* params, int8_t* occ_host, uint8_t* rgb_host);
int tsd_map_frame_wait(tsd_ctx* ctx, int* n_surface);
/* The same frame as a windowed update, the form rviz and nav2's static layer take on <map>_updates (map_msgs/OccupancyGridUpdate): only
 * the rectangle that can differ from the context's previous frame or update is recomputed on the device and copied to the host.
 * occ_host / rgb_host are the caller's FULL buffers (cells*cells, 3*cells*cells); the window's rows and columns alone are written
 * into them, so a caller that passes the same buffers every time always holds the full current frame (what ThreadGrid.cpp:72-131
 * rebuilds from scratch).  *win is that rectangle in cells; width == 0: nothing was pushed or freed since the previous frame, nothing
 * is enqueued and wait returns at once.  The window is the whole map where no previous frame can be built on: the first call, a
 * staging that was replaced (the image switched on), other inflation parameters than the previous frame's, inflate_factor > 31, a
 * grid rewritten wholesale since (tsd_reset, tsd_upload_tiles, tsd_load_grid_text, tsd_set_max_truncation, a tsd_fuse destination),
 * a previous frame that ended in an error.  tsd_map_frame_begin counts as the previous frame as well.  Ordering, the one frame in
 * flight and the buffers' lifetime are tsd_map_frame_begin's; n_surface counts the marks made by this update's tiles only. */
typedef struct {
  int32_t x, y, width, height;  /* cells; width == 0: nothing changed */
} tsd_map_window;
int tsd_map_update_begin(tsd_ctx* ctx, const tsd_map_params* params, int8_t* occ_host, uint8_t* rgb_host, tsd_map_window* win);
int tsd_map_update_wait(tsd_ctx* ctx, int* n_surface);
/* page-locked host memory for the frame buffers (NULL on failure), and its release */
void* tsd_host_alloc(uint64_t bytes);
void tsd_host_free(void* p);

/* ---- clearance: the Euclidean distance to the nearest occupied cell, and the cost map of nav2's inflation layer ------------------- */
/* How far is this cell from the nearest obstacle?  Input: an int8 map, width x height, row = y, `stride` bytes from row to row -- a
 * frame's staged map, a group's merged map, any device map.  In integers throughout (the kernels do no floating point), so a
 * restatement agrees to the byte (tests/clearance_ref.py).
 *   O              the cells of the WHOLE map whose value equals 100; there is no obstacle outside the map
 *   R              the radius in cells, 1 .. TSD_CLEARANCE_MAX_RADIUS
 *   g(x, y)        min over (ox, y) in O of |x - ox|, capped: min(that, R + 1); R + 1 on a row without an obstacle          (row pass)
 *   m(x, y)        min over dy in [-R, R] with 0 <= y + dy < height of g(x, y + dy)^2 + dy^2                                (column pass)
 *   d2(x, y)       m if m <= R*R, else 0xFFFF                                                              (uint16, the distance field)
 * which is min over (ox, oy) in O of (x - ox)^2 + (y - oy)^2 where that minimum is <= R*R, 0xFFFF otherwise: the cut-off is Euclidean
 * (at R = 5 an obstacle at offset (3, 4) counts, one at (5, 1) does not).
 * Cost map (int8) from a table T[0 .. R*R] of int8, s = the source cell:
 *   d2 <= R*R      c = T[d2];  out = -1 if s == -1 and c < 99, else max(s, c)            (signed; nav2: unknown stays unknown unless
 *   d2 == 0xFFFF   out = s                                                                 it lies inside the inscribed band)
 * A window w is the unit of work: only the cells of w are written; the map is read in w grown by R, clipped to the map. */
#define TSD_CLEARANCE_MAX_RADIUS 255
/* The table of nav2's inflation layer (host code, no GPU): T[0] = 100; with d = sqrt((double)d2) * cell_size, T[d2] = 99 where
 * d <= inscribed_radius_m, else clamp((int)(98.0 * exp(-cost_scaling * (d - inscribed_radius_m))), 1, 98) -- nav2's 252 * exp(..) taken
 * through the 1..252 -> 1..98 scale of its OccupancyGrid publisher.  table: radius_cells^2 + 1 entries.  TSD_E_ARG for a NULL
 * table, a radius outside 1 .. TSD_CLEARANCE_MAX_RADIUS, a cell size that is not > 0. */
int tsd_costmap_table(double cell_size, int radius_cells, double inscribed_radius_m, double cost_scaling, int8_t* table);
/* The generic form, for any map on the context's device (e.g. tsd_group_map_dev): enqueues on the context's stream and waits.
 * win NULL: the whole map.  table: radius_cells^2 + 1 host entries, NULL: no cost map (cost_dev must be NULL then).  dist2_dev (uint16)
 * / cost_dev (int8): width x height each, rows of `width` elements, either may be NULL (not both); only the window is written.
 * Scratch (one bit per cell, one byte per 32 x 32 tile) stays with the context and grows on demand: a repeated call allocates
 * nothing.  TSD_E_ARG: a NULL map, a side outside 1 .. 65536, stride < width, a radius out of range, an empty window or one not
 * inside the map, no output, a cost map of this context in flight. */
int tsd_clearance_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_map_window* win /* NULL: whole */,
                      int radius_cells, const int8_t* table /* host, NULL: no cost map */, void* dist2_dev /* or NULL */,
                      void* cost_dev /* or NULL */);
/* The cost map of the frame just taken: reads the device copy of the map that the context's last tsd_map_frame_* / tsd_map_update_*
 * left in its frame staging -- the bytes <node>/map carried, so map and cost map never disagree.  map_win: the window that update
 * returned (NULL: the whole map; width 0: nothing changed, nothing is enqueued, *out_win is empty and wait returns at once).  The cost
 * map is recomputed in map_win grown by radius_cells and clipped, returned in *out_win; only those rows and columns are copied into
 * the caller's FULL buffers cost_host (cells*cells int8) and dist2_host (cells*cells uint16; with want_dist2), as tsd_map_update_begin
 * does -- the staged map differs from the previous one only inside map_win, so d2 can differ only within R of it, and those cells
 * read obstacles within 2R of it from a map that is complete on the device.  Kernels and copies run on the context's copy stream
 * behind the frame's event; the grid's stream never waits for them.  The table is tsd_costmap_table(cell size, params).  The
 * buffers must stay valid until tsd_costmap_wait returns.  TSD_E_ARG: no completed previous frame, a frame in flight, a radius out of
 * range, a window not inside the map, a cost map already in flight, want_dist2 without dist2_host.  A frame begun while a cost map is
 * in flight is refused like a second frame.  The grid and its write ledger are not touched. */
typedef struct {
  int32_t radius_cells;         /* R */
  int32_t want_dist2;           /* != 0: the distance field is copied to dist2_host as well */
  double  inscribed_radius_m;
  double  cost_scaling;
} tsd_costmap_params;
int tsd_costmap_begin(tsd_ctx* ctx, const tsd_costmap_params* params, int8_t* cost_host, uint16_t* dist2_host /* or NULL */,
                      const tsd_map_window* map_win /* NULL: whole */, tsd_map_window* out_win);
int tsd_costmap_wait(tsd_ctx* ctx);
/* Plain device memory on the context's device for a caller without a HIP runtime of its own (a ctypes driver), e.g. a map handed to
 * tsd_clearance_dev and its outputs: allocation (NULL on failure), release (waits for the context's stream first), and a copy of
 * `bytes` between host and device (to_device != 0: host to device) on the context's stream, which waits for it. */
void* tsd_dev_alloc(tsd_ctx* ctx, uint64_t bytes);
void  tsd_dev_free(tsd_ctx* ctx, void* p);
int   tsd_dev_copy(tsd_ctx* ctx, void* dst, const void* src, uint64_t bytes, int to_device);
/* TEST HOOK: on = 0 makes every workgroup of the column pass walk its rows instead of skipping where no tile within R holds an
 * obstacle.  The outputs are the same byte for byte (tests/test_gpu_clearance.py); only the time differs. */
int tsd_debug_set_clearance_skip(tsd_ctx* ctx, int on);

/* ---- frontiers: where to drive to make the map bigger --------------------------------------------------------- */
/* The free cells that border unknown space, grouped into connected frontiers, each with its size, the sums its centroid follows from,
 * its bounding box, and whether a robot standing on a seed cell can reach it.  Input: an int8 map on the context's device, width x
 * height, `stride` bytes from row to row (as tsd_clearance_dev); bytes beyond `width` in a row are never read.  Sides 1 .. 32768, so a
 * linear index y * width + x fits a uint32 and 0xFFFFFFFF means "none".  In integers throughout (the kernels do no floating point): a
 * restatement agrees to the byte and the list's order is fixed (tests/frontier_ref.py).
 *   unknown        v < 0
 *   traversable    0 <= v <= free_max           (free_max = 0: the free cells of an occupancy map; larger: the low costs of a cost map)
 *   frontier cell  a traversable cell with at least one of its four edge neighbours INSIDE THE MAP unknown (the border is not unknown)
 *   frontier       an 8-connected component of frontier cells; its root is the smallest linear index among its cells
 *   region         a 4-connected component of traversable cells, root likewise (a diagonal gap in a wall is no passage)
 *   used seed      a seed inside the map on a traversable cell; other seeds are ignored, *seeds_used counts the used ones
 *   reachable      1 where a cell of the frontier lies in the region of a used seed, else 0; -1 in every record with n_seeds == 0
 *                  (no regions are computed then)
 * Outputs: a label image, uint32 width x height, rows of `width` elements, every cell written -- the root's linear index on frontier
 * cells, 0xFFFFFFFF elsewhere, for ALL frontiers whatever min_size is -- and the list of tsd_frontier records of the frontiers with
 * size >= min_size in ascending root index.  The centroid is host arithmetic: (sum_x / size, sum_y / size) in cells. */
#define TSD_FRONTIER_MAX_SEEDS 16
#define TSD_FRONTIER_MAX_SIDE  32768
#define TSD_FRONTIER_NONE      0xFFFFFFFFu
typedef struct {
  int32_t  root_x, root_y;      /* the frontier's cell with the smallest linear index */
  uint32_t size;                /* cells */
  int32_t  reachable;           /* 1 / 0; -1: no seeds were given */
  uint64_t sum_x, sum_y;        /* sums of the cells' x and y */
  int32_t  min_x, min_y, max_x, max_y;   /* bounding box, inclusive */
} tsd_frontier;                 /* 48 bytes */
typedef struct {
  int32_t  free_max;            /* 0 .. 99 */
  uint32_t min_size;            /* >= 1: smaller frontiers keep their labels but get no record */
  int32_t  n_seeds;             /* 0 .. TSD_FRONTIER_MAX_SEEDS */
  int32_t  reserved;
  const int32_t* seeds_xy;      /* n_seeds pairs (x, y) of cells, host memory; may be NULL with n_seeds == 0 */
} tsd_frontier_params;
/* The generic form, for any map on the context's device (a group's merged map, a cost map): enqueues on the context's stream and
 * waits.  *n: the list's length, *seeds_used (may be NULL): the seeds that counted.  Scratch stays with the context and grows on
 * demand -- 4 bytes per cell for the labels, 4 for the roots' ranks, 4 more for the regions' labels once a call brings seeds, one
 * count per 32 cells of a row, 2 bytes per tile, the records -- so a repeated call at the same size allocates nothing.  Both forms
 * share that scratch and the result: one frontier call at a time per context, from the call to the last fetch of its result -- the
 * caller's duty (the facade: obvious::TsdGrid::frontierMutex, taken by ThreadGrid and ThreadGridGroup alike).  TSD_E_NOMEM
 * (tsd_last_error says which buffer) where the device cannot hold it; the previous result is gone then.  TSD_E_ARG, with the previous
 * result left fetchable: a NULL map or params, a side outside 1 .. TSD_FRONTIER_MAX_SIDE, stride < width, free_max outside 0 .. 99,
 * min_size < 1, n_seeds outside 0 .. TSD_FRONTIER_MAX_SEEDS, seeds_xy NULL with n_seeds > 0, a NULL n. */
int tsd_frontiers_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_frontier_params* params,
                      int* n, int* seeds_used /* or NULL */);
/* The same for the map that the context's last tsd_map_frame_* / tsd_map_update_* left in its frame staging (cells x cells, the bytes
 * <node>/map carried).  Runs where the cost map runs: on the context's copy stream behind the frame's event, never on the grid's
 * stream, and waits for it.  TSD_E_ARG also without a completed frame and with a frame or a cost map in flight.  The grid and its write
 * ledger are not touched. */
int tsd_frontiers_frame(tsd_ctx* ctx, const tsd_frontier_params* params, int* n, int* seeds_used /* or NULL */);
/* Records first .. first + count - 1 of the last result.  TSD_E_ARG for a range outside [0, n) (count == 0 is served anywhere in
 * [0, n]) and for a NULL out with count > 0. */
int tsd_frontiers_fetch(tsd_ctx* ctx, int first, int count, tsd_frontier* out);
/* The last result on the device: the records (n of them), the label image (uint32, width x height of that call).  Valid until the
 * next frontier call on the context or tsd_destroy.  TSD_E_ARG without a result. */
int tsd_frontiers_dev_ptrs(tsd_ctx* ctx, const void** records_dev, const void** labels_dev, int* n);
/* What the last call counted (each pointer may be NULL): the frontiers before min_size, and the unions the seam pass made between
 * tiles for the frontiers' and for the regions' labels. */
int tsd_frontiers_counts(tsd_ctx* ctx, int* n_all, int* seam_unions, int* region_seam_unions);

/* ---- routes: what it costs to drive to a cell, which robot is nearest, and the way there ------------------------ */
/* The cost-to-go field of an int8 map from up to 16 seed cells (the robots), the cheapest cell of every frontier with the seed it is
 * cheapest from, and the paths.  Input: an int8 map on the context's device as for the frontiers -- width x height, `stride` bytes
 * from row to row, bytes beyond `width` in a row never read, sides 1 .. TSD_FRONTIER_MAX_SIDE.  In integers throughout (the kernels
 * do no floating point), so a restatement agrees to the byte (tests/route_ref.py).
 *   traversable    0 <= v <= free_max, free_max in 0 .. 99                                                  (the frontiers' rule)
 *   W[v]           the weight of a traversable cell of value v: a host table of uint8 W[0 .. free_max], each 1 .. 255; NULL: all 1
 *   neighbour k    k = 0 .. 7 in this order: (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (1,-1) (-1,1) (1,1)
 *   move a -> b    both cells inside the map and traversable; a diagonal move also needs both cells it cuts, (a.x, b.y) and (b.x, a.y),
 *                  traversable -- a diagonal gap in a wall is no passage, so the cells a seed reaches are its 4-connected region
 *   cost of a move c_k * W[v_b], the weight of the cell entered; c_k = 5 for k < 4, 7 for the diagonals
 *   used seed      a seed inside the map on a traversable cell (*seeds_used counts them); seed i keeps its index i of the caller's
 *                  list whether or not earlier seeds were used
 *   key(cell)      uint32 (d << 4) | i: the minimum over all used seeds i and all paths from seed i to the cell of
 *                  (path cost << 4) | i -- d is the least cost, i the lowest seed index that attains it; a seed's cell has d = 0
 *   limit          only d <= limit counts, 1 <= limit <= TSD_ROUTE_MAX_DIST; 0 means TSD_ROUTE_MAX_DIST.  The largest step is
 *                  7 * 255 = 1785, so no candidate d + step leaves 28 bits
 *   every other cell -- not traversable, not reached, beyond the limit -- holds TSD_ROUTE_NONE
 * The weights are positive, so the key image is the unique fixed point of key[b] = min(key[b], key[a] + (c_k * W[v_b] << 4)) over
 * all moves, started from the seeds; candidates beyond the limit are dropped, which is exact because every prefix of a path within the
 * limit is within the limit.  The result does not depend on the order of the work.
 * Output: the key image, uint32 width x height, rows of `width` elements, every cell written.
 *   goal of a frontier   over the frontier's cells with a key, the minimum of (key << 32) | linear index: the cheapest cell to reach,
 *                        the smallest index among ties, and in the key the nearest robot
 *   path to a cell b     from b with d > 0 step to a = b - offset_k for the first k in the order above where a -> b is a move and
 *                        key[a] + (c_k * W[v_b] << 4) == key[b]; b is written, then a, ... the seed's cell (d = 0) last */
#define TSD_ROUTE_NONE     0xFFFFFFFFu
#define TSD_ROUTE_MAX_DIST 0x0FFFF000u
#define TSD_ROUTE_MAX_ROUNDS (1 << 20)
#define TSD_ROUTE_MAX_GOALS  4096
#define TSD_ROUTE_MAP      0            /* tsd_route_frame's sources: the staged map of the last frame or update ... */
#define TSD_ROUTE_COSTMAP  1            /* ... the cost map of the last completed tsd_costmap_begin / _wait */
typedef struct {
  int32_t  free_max;            /* 0 .. 99 */
  int32_t  n_seeds;             /* 1 .. TSD_FRONTIER_MAX_SEEDS */
  const int32_t* seeds_xy;      /* n_seeds pairs (x, y) of cells, host memory */
  const uint8_t* weights;       /* W[0 .. free_max], host memory; NULL: all 1 */
  uint32_t limit;               /* 0: TSD_ROUTE_MAX_DIST */
  int32_t  max_rounds;          /* 0: 16 * (tiles_x + tiles_y) + 64; at most TSD_ROUTE_MAX_ROUNDS */
} tsd_route_params;
typedef struct {
  int32_t  seeds_used;
  int32_t  rounds;              /* launches of the relaxation */
  int32_t  converged;           /* 0: max_rounds ran out; every key is then an upper bound of the rule's key */
  uint32_t reached;             /* cells with a key */
} tsd_route_info;
typedef struct {
  uint32_t cell;                /* linear index y * width + x; TSD_ROUTE_NONE where no cell of the frontier has a key */
  uint32_t dist;                /* d; TSD_ROUTE_NONE likewise */
  int32_t  seed;                /* i; -1 likewise */
  uint32_t reserved;
} tsd_route_goal;               /* 16 bytes */
/* W[v] = min(255, 1 + v * (max_weight - 1) / 98) by integer division for v = 0 .. free_max: 1 on a free cell, max_weight at 98, the
 * highest cost outside the inscribed band of a cost map (the minimum only binds at v = 99).  Host code, no GPU.  TSD_E_ARG for a NULL table, free_max outside 0 .. 99, max_weight
 * outside 1 .. 255. */
int tsd_route_weights(int free_max, int max_weight, uint8_t* table /* free_max + 1 entries */);
/* The generic form, for any map on the context's device: enqueues on the context's stream and waits.  The relaxation runs in
 * rounds, one launch each, one workgroup per 32 x 32 tile; a tile works in a round only where a neighbour's keys fell in the round
 * before, and the host reads one word per batch of rounds.  Only kernel boundaries order the tiles: no workgroup waits for another.
 * Scratch stays with the context and grows on demand -- 4 bytes per cell for the keys, 1 for the cells' weights (what the paths are
 * traced on, so the map may be released after the call), 2 bytes per tile, the goals, the paths and their pinned copy -- so a repeated
 * call at the same size allocates nothing.  One route call at a time per context, from the call to the last fetch, and since the
 * goals read the frontier result, under the same lock as the frontier calls.  TSD_E_NOMEM (tsd_last_error says which buffer) where
 * the device cannot hold it; the previous result is gone then.  TSD_E_ARG, with the previous result left in place: a NULL map, params
 * or info, a side outside 1 .. TSD_FRONTIER_MAX_SIDE, stride < width, free_max outside 0 .. 99, a weight of 0, limit >
 * TSD_ROUTE_MAX_DIST, n_seeds outside 1 .. TSD_FRONTIER_MAX_SEEDS, seeds_xy NULL, max_rounds outside 0 .. TSD_ROUTE_MAX_ROUNDS. */
int tsd_route_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_route_params* params,
                  tsd_route_info* info);
/* The same for what the context's last frame left on the device (cells x cells), on the context's copy stream behind the frame's
 * event like tsd_frontiers_frame, never on the grid's stream.  source TSD_ROUTE_MAP: the staged map; TSD_ROUTE_COSTMAP: the cost
 * map of the last completed tsd_costmap_begin / _wait.  TSD_E_ARG also without a completed frame, for TSD_ROUTE_COSTMAP without a
 * completed cost map or with one of another size, with a frame or a cost map in flight, and for another source.  The grid and its
 * write ledger are not touched. */
int tsd_route_frame(tsd_ctx* ctx, int source, const tsd_route_params* params, tsd_route_info* info);
/* The goals of the frontier result the context holds (tsd_frontiers_*), one per record and in the records' order, from the key image
 * it holds: *n is their number.  Labels whose root has no record (min_size) are skipped.  TSD_E_ARG without a route result, without
 * a frontier result, or where their widths or heights differ. */
int tsd_route_goals(tsd_ctx* ctx, int* n);
/* Goals first .. first + count - 1 of the last tsd_route_goals, as tsd_frontiers_fetch. */
int tsd_route_goals_fetch(tsd_ctx* ctx, int first, int count, tsd_route_goal* out);
/* The paths to n_goals cells (any cells, linear indices; 1 .. TSD_ROUTE_MAX_GOALS of them, n_goals * max_len <= 1 << 24, max_len >=
 * 1) on the key image the context holds: paths_host[g * max_len + j], j < min(len, max_len), goal first and seed last; len_host[g] is
 * the full length even where the path is cut at max_len, 0 for a goal without a key or outside the map, -1 where no neighbour
 * matches (only on an image that did not converge).  TSD_E_ARG without a route result. */
int tsd_route_trace(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, int max_len, uint32_t* paths_host, int32_t* len_host);
/* The last result on the device: the key image (uint32, width x height of that call), valid until the next route call on the
 * context or tsd_destroy.  Each pointer may be NULL.  TSD_E_ARG without a result. */
int tsd_route_dev_ptrs(tsd_ctx* ctx, const void** keys_dev, int* width, int* height);
/* What the last call counted (each pointer may be NULL): the workgroups that found their tile active, over all rounds, and the
 * times the host waited for the device. */
int tsd_route_counts(tsd_ctx* ctx, long long* tile_visits, int* host_waits);
/* TEST HOOK: the sweeps a tile makes inside one launch before it hands itself on to the next round (default 2048; 0 restores it).
 * 1 is the other extreme of the schedule: the keys are the same byte for byte (tests/test_gpu_route.py), only the rounds differ. */
int tsd_debug_set_route_sweeps(tsd_ctx* ctx, int n);

/* ---- waypoints: a traced path straightened into cells joined by straight drivable segments ----------------------- */
/* For each goal cell a short list of cells of its path, in DRIVING order -- the seed's cell first, the goal last: the opposite of
 * tsd_route_trace's order -- such that consecutive cells are joined by a straight segment a robot can drive.  It works on the route
 * result the context holds: the key image and the weight image w the paths are traced on (0: not traversable), with the routes'
 * constants: c = 5 for a straight step, 7 for a diagonal one, d = key >> 4.  In integers throughout (the kernel does no floating
 * point), so a restatement agrees to the byte (tests/waypoint_ref.py).
 *   path           tsd_route_trace's path of the goal cell, reversed: p_0 is the seed's cell (d = 0), p_{n-1} the goal, n the trace's
 *                  full length `len`
 *   line p -> q    dx = q.x - p.x, dy = q.y - p.y, N = max(|dx|, |dy|) >= 1; step j = 1 .. N lies at
 *                  p + (sgn(dx) * ((2 j |dx| + N) / 2N), sgn(dy) * ((2 j |dy| + N) / 2N)) by integer division: the views' ray with
 *                  R = N, and step N is q.  The major axis advances by exactly one per step, the minor axis by zero or one, so every
 *                  step is a straight or a diagonal neighbour step and the line stays inside the bounding box of p and q
 *   a segment p -> q passes   if every step is a move of the routes' rule: the cell entered has w != 0, and on a diagonal step
 *                  both cells it cuts have w != 0 -- ONE blocked corner cell refuses the step (the routes' rule, not the views',
 *                  where both must block).  Its cost is the sum over its steps of c * w[cell entered]
 *   next waypoint  from an anchor p_a the LARGEST j in (a, min(a + lookahead, n - 1)] whose segment p_a -> p_j passes and costs at
 *                  most d[p_j] - d[p_a] + slack.  j = a + 1 always qualifies (a traced step: its cost is exactly the difference).
 *                  p_j is emitted and becomes the anchor, until the goal is emitted; p_0 is emitted first
 * The result is defined by "largest j", not by a search order: it does not depend on how the work is scheduled.  On a converged key
 * image a passing segment is a path of the routes' graph and never costs less than d[p_j] - d[p_a], so with slack = 0 every segment
 * is an equally cheap way and the total cost equals d(goal); with unit weights the line's cost is the octile distance, a lower bound
 * of every path, so the slack never binds, the rule is pure line of sight and the total is d(goal) again; in general the total is at
 * most d(goal) + (n_way - 1) * slack.  With cost-map weights, slack is how much extra cost per segment a shortcut may pay to leave
 * the cost valley.
 *   record         len: as tsd_route_trace gives it (0: no key or outside the map, -1: no matching neighbour);  n_way: the full
 *                  count even where it is larger than max_way, 0 where len <= 0 or len > max_len (a path the trace buffer cuts is
 *                  not straightened), 1 for a goal on its seed;  cost: the sum of the segments' costs (modulo 2^32);  dist: the
 *                  goal's d, TSD_ROUTE_NONE without a key */
#define TSD_WAYPOINT_MAX_LOOKAHEAD 1024
typedef struct {
  int32_t  lookahead;           /* path cells a segment may span: 1 .. TSD_WAYPOINT_MAX_LOOKAHEAD */
  uint32_t slack;               /* extra cost a segment may pay over the field's difference */
  int32_t  max_len;             /* the trace buffer per goal, >= 1 */
  int32_t  max_way;             /* waypoints returned per goal, >= 1 */
} tsd_waypoint_params;          /* 16 bytes */
typedef struct {
  int32_t  len;
  int32_t  n_way;
  uint32_t cost;
  uint32_t dist;
} tsd_waypoint_info;            /* 16 bytes */
/* The waypoints of n_goals cells (any cells, linear indices; 1 .. TSD_ROUTE_MAX_GOALS of them, n_goals * max_len <= 1 << 24 and
 * n_goals * max_way <= 1 << 24): way_host[g * max_way + i], i < min(n_way, max_way), seed first and goal last; words beyond that are
 * not written.  The trace runs into the route's scratch and k_route_waypoints right behind it, one workgroup per goal, on the stream
 * of the route result like tsd_route_trace and under the same lock as the frontier, route and view calls; the call waits.  Scratch
 * stays with the context and grows on demand: a repeated call at the same size allocates nothing.  TSD_E_ARG, with the outputs and
 * the context's result left as they were: no route result, a NULL argument, lookahead outside 1 .. TSD_WAYPOINT_MAX_LOOKAHEAD,
 * max_len < 1, max_way < 1, n_goals outside 1 .. TSD_ROUTE_MAX_GOALS, n_goals * max_len or n_goals * max_way above 1 << 24. */
int tsd_route_waypoints(tsd_ctx* ctx, const uint32_t* goal_cells, int n_goals, const tsd_waypoint_params* params,
                        uint32_t* way_host /* [g * max_way + i], i < min(n_way, max_way): linear cell indices, seed first, goal last */,
                        tsd_waypoint_info* info_host /* n_goals */);

/* ---- fields: a cost-to-go field per robot, for a fleet whose robots compete for the same goals ------------------- */
/* A fields call takes tsd_route_params like a route call and relaxes L = n_seeds key images ("layers") side by side in the same
 * rounds, uint32 each, layer r at keys + r * width * height:
 *   layer r        the key image of the routes' rule with seed r ALONE; its index r stays in the key's low four bits.  It is byte
 *                  for byte what tsd_route_dev leaves when every other seed of the list lies outside the map
 *   unused seed    a seed outside the map or not on a traversable cell gives a layer of TSD_ROUTE_NONE only (used[r] = 0)
 *   shared cell    two seeds on one cell get a full field each
 *   identity       the element-wise minimum of the layers is tsd_route_dev's image for the whole list
 *   goal matrix    tsd_route_goal[L][n] over the n records of the frontier result: row r holds the routes' goal of every frontier
 *                  on layer r -- robot r's cheapest cell of that frontier, seed == r -- or {NONE, NONE, -1} where the frontier
 *                  has no cell with a key on that layer
 *   paths          a goal is a pair (cell, layer): the routes' path and waypoint rules on that layer's keys
 * The fields result is a second instance of the route result in the context: a tsd_route_dev / _frame result and a fields result
 * live side by side, and neither kind of call touches the other's keys, goals or paths.  The same kernels run both, a route call
 * with one layer: one workgroup per tile AND layer in a round, the "any" word shared by all layers (one host wait per batch of
 * rounds serves them all), so `rounds` is the rounds of the slowest layer.  Scratch stays with the context and grows on demand -- 4
 * bytes per cell and layer for the keys, 1 per cell for the weights, 2 per tile and layer, the matrix, the paths and their pinned
 * copies -- so a repeated call at the same size and seed count allocates nothing.  The fields calls take the same lock as the
 * frontier, route and view calls.  TSD_E_NOMEM (tsd_last_error names the buffer) where the device cannot hold it; the fields
 * result is gone then.  tsd_debug_set_route_sweeps applies to fields calls as well. */
typedef struct {
  int32_t  layers;              /* L = n_seeds */
  int32_t  rounds;              /* launches of the relaxation: the slowest layer's */
  int32_t  converged;           /* 0: max_rounds ran out; every key of every layer is then an upper bound of the rule's key */
  int32_t  seeds_used;
  uint8_t  used[TSD_FRONTIER_MAX_SEEDS];       /* 1: seed r is used */
  uint32_t reached[TSD_FRONTIER_MAX_SEEDS];    /* cells with a key on layer r; 0 for r >= layers */
} tsd_route_fields_info;        /* 96 bytes */
/* The layers of any map on the context's device: as tsd_route_dev -- the context's stream, waited for, the same refusals with the
 * previous fields result left in place.  Timed launches: "route_fields_init", "route_fields_relax". */
int tsd_route_fields_dev(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_route_params* params,
                         tsd_route_fields_info* info);
/* The same for what the context's last frame left on the device, as tsd_route_frame: sources, stream and refusals are its. */
int tsd_route_fields_frame(tsd_ctx* ctx, int source, const tsd_route_params* params, tsd_route_fields_info* info);
/* The goal matrix of the frontier result the context holds on the fields result it holds: *n is the number of records, the row
 * length.  A frontier cell finds its record by one search and lowers its slot on every layer whose key it has.  TSD_E_ARG as
 * tsd_route_goals: without a fields result, without a frontier result, or where their sizes differ.  Timed: "route_fields_goals". */
int tsd_route_fields_goals(tsd_ctx* ctx, int* n);
/* Goals first .. first + count - 1 of row `layer` of the last matrix, as tsd_route_goals_fetch; TSD_E_ARG also for a layer outside
 * 0 .. layers - 1. */
int tsd_route_fields_goals_fetch(tsd_ctx* ctx, int layer, int first, int count, tsd_route_goal* out);
/* tsd_route_trace with a layer per goal: goal g is traced on layer goal_layers[g], all goals in one launch ("route_fields_trace").
 * A goal without a key on its layer has len 0 whatever the other layers hold.  TSD_E_ARG, with the outputs untouched, as
 * tsd_route_trace, and for a NULL goal_layers or a goal_layers[g] >= layers. */
int tsd_route_fields_trace(tsd_ctx* ctx, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals, int max_len,
                           uint32_t* paths_host, int32_t* len_host);
/* tsd_route_waypoints with a layer per goal, likewise: the same trace launch, then the same waypoint launch ("route_waypoints") on
 * each goal's layer.  Refusals as tsd_route_waypoints and as tsd_route_fields_trace for the layers. */
int tsd_route_fields_waypoints(tsd_ctx* ctx, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals,
                               const tsd_waypoint_params* params, uint32_t* way_host, tsd_waypoint_info* info_host);
/* The fields result on the device: layer r at keys + r * width * height (uint32), valid until the next fields call on the context or
 * tsd_destroy.  Each pointer may be NULL.  TSD_E_ARG without a result. */
int tsd_route_fields_dev_ptrs(tsd_ctx* ctx, const void** keys_dev, int* width, int* height, int* layers);
/* As tsd_route_counts, over all layers: the workgroups that found their tile active, and the host's waits. */
int tsd_route_fields_counts(tsd_ctx* ctx, long long* tile_visits, int* host_waits);

/* ---- drive: the velocity of the next step -- arcs rolled out on the weight image and rated on a goal field --------- */
/* For each robot a grid of (speed, turn) samples is rolled forward T time steps from the robot's pose; a sample whose arc leaves the
 * traversable cells is refused, the others are rated by the cost-to-go at their end, and the best one is the command.  It works on
 * the route result the context holds (tsd_drive_rollout) or on a layer of the fields result (tsd_drive_fields_rollout): the weight
 * image w (0: not traversable) and the key image, d = key >> 4.  A key image holds the cost FROM its seeds, so to drive towards a
 * goal the result must have been seeded AT the goal (the navigation potential).  In integers throughout (the kernel does no floating
 * point), so a restatement agrees to the byte (tests/drive_ref.py).
 *   directions     D[h] = (cx, cy), int32 Q16, h = 0 .. H - 1, H = TSD_DRIVE_HEADINGS, from tsd_drive_table: for h = 0 .. H/8
 *                  cx = lrint(65536 cos(2 pi h / H)), cy = lrint(65536 sin(2 pi h / H)); every other entry follows from those by the
 *                  octant symmetries -- D[h] = (cy, cx)[H/4 - h] for H/8 < h <= H/4, D[h] = (-cx, cy)[H/2 - h] for H/4 < h <= H/2,
 *                  D[h] = -D[h - H/2] above -- so D[h + H/2] = -D[h], D[H/4] = (0, 65536) exactly, and only the first octant
 *                  depends on libm.  Heading 0 looks along +x, H/4 along +y of the image
 *   pose           the cell (x0, y0), the offset (fx, fy) inside it in Q16, each 0 .. 65535, the heading index h0 in 0 .. H - 1,
 *                  and a layer (the route form ignores it)
 *   samples        step_q16[V]: the step length per time step, 0 .. 65536 (at most one cell, so consecutive centre cells are
 *                  neighbours or the same); turn[Wn]: the heading increment per time step, |t| <= H/8; T steps, 1 .. 256.  Sample
 *                  (i, j) has the index i * Wn + j
 *   trajectory     of sample (i, j) with s = step_q16[i], t = turn[j], for k = 1 .. T, products in 64 bits, >> arithmetic:
 *                    h_k = (h0 + k t) mod H, non-negative
 *                    X_k = X_{k-1} + ((s cx[h_k] + 32768) >> 16), X_0 = fx;   Y_k likewise with cy[h_k], Y_0 = fy
 *                    the centre cell c_k = (x0 + (X_k >> 16), y0 + (Y_k >> 16));  c_0 = (x0, y0)
 *   body           B points (bx, by) in Q16 cells in the robot's frame, x forward; 0 <= B <= 64, |bx|, |by| <= 64 * 65536.  Point b at
 *                  step k lies at (X_k + ((bx cx[h_k] - by cy[h_k] + 32768) >> 16), Y_k + ((bx cy[h_k] + by cx[h_k] + 32768) >> 16));
 *                  its cell is taken like the centre's
 *   step k is refused   by the first of these that holds, in this order:
 *                    1  c_k lies outside the map
 *                    2  w[c_k] == 0
 *                    3  c_k differs from c_{k-1} in x AND in y, and one of the two cells the step cuts, (c_{k-1}.x, c_k.y) and
 *                       (c_k.x, c_{k-1}.y), has w == 0 (the routes' rule: ONE blocked corner refuses)
 *                    4  for the lowest b whose cell lies outside the map or has w == 0
 *                  and after step T:  5  key[c_T] == TSD_ROUTE_NONE on the sample's key image.
 *                  The start pose itself is not tested (but c_1 is, also where it is the start's cell)
 *   why            uint16 per sample: 0 where it is admissible, else (reason << 12) | k for the smallest refusing k with its first
 *                  reason; k = T for reason 5
 *   score          of an admissible sample, uint64: a_end d_end + a_nose d_nose + a_cost cost + a_turn |t|, with d_end = key[c_T] >> 4,
 *                  cost = the sum over k = 1 .. T of w[c_k], and d_nose = key >> 4 at the cell of
 *                  (X_T + ((nose_q16 cx[h_T] + 32768) >> 16), Y_T + ((nose_q16 cy[h_T] + 32768) >> 16)) where that cell lies inside
 *                  the map and has a key, d_end + nose_miss otherwise.  nose_q16 in 0 .. 64 * 65536, the coefficients in 0 .. 255,
 *                  nose_miss <= TSD_ROUTE_MAX_DIST.  The nose term makes a robot that faces away from its way turn on the spot:
 *                  d_end alone cannot tell two rotations apart
 *   choice         the minimum of (score << 16) | index over the admissible samples: the best score, among ties the lowest index
 *                  -- the caller orders its lists by preference.  Without an admissible sample speed = turn = -1, score =
 *                  TSD_DRIVE_NONE, end_cell = d_end = d_nose = TSD_ROUTE_NONE, cost = 0
 * The result is defined by a minimum, not by a search order: it does not depend on how the work is scheduled. */
#define TSD_DRIVE_HEADINGS   4096
#define TSD_DRIVE_MAX_STEPS  256
#define TSD_DRIVE_MAX_SPEEDS 64
#define TSD_DRIVE_MAX_TURNS  129
#define TSD_DRIVE_MAX_BODY   64
#define TSD_DRIVE_MAX_ROBOTS 16
#define TSD_DRIVE_NONE       0xFFFFFFFFFFFFFFFFull
typedef struct {
  int32_t  steps;               /* T: 1 .. TSD_DRIVE_MAX_STEPS */
  int32_t  n_speeds;            /* V: 1 .. TSD_DRIVE_MAX_SPEEDS */
  int32_t  n_turns;             /* Wn: 1 .. TSD_DRIVE_MAX_TURNS */
  int32_t  n_body;              /* B: 0 .. TSD_DRIVE_MAX_BODY */
  const int32_t* step_q16;      /* [V], host memory, each 0 .. 65536 */
  const int32_t* turn;          /* [Wn], host memory, each |t| <= TSD_DRIVE_HEADINGS / 8 */
  const int32_t* body_q16;      /* [B] pairs (bx, by), host memory; may be NULL where B == 0 */
  int32_t  a_end, a_nose, a_cost, a_turn;      /* each 0 .. 255 */
  int32_t  nose_q16;            /* 0 .. 64 * 65536 */
  uint32_t nose_miss;           /* <= TSD_ROUTE_MAX_DIST */
} tsd_drive_params;             /* 64 bytes */
typedef struct {
  int32_t x, y;                 /* the cell */
  int32_t fx, fy;               /* the offset inside it, Q16: 0 .. 65535 */
  int32_t heading;              /* 0 .. TSD_DRIVE_HEADINGS - 1 */
  int32_t layer;                /* the fields form: 0 .. layers - 1; the route form ignores it */
} tsd_drive_pose;               /* 24 bytes */
typedef struct {
  int32_t  speed, turn;         /* the chosen sample's indices i, j; -1 without an admissible sample */
  int32_t  admissible;          /* the number of admissible samples */
  uint32_t end_cell;            /* c_T as a linear index y * width + x */
  uint32_t d_end, d_nose, cost;
  uint32_t reserved;
  uint64_t score;
} tsd_drive_choice;             /* 40 bytes */
/* The direction table, 2 * TSD_DRIVE_HEADINGS words: cx of heading h at table[2 h], cy at table[2 h + 1].  Host code, no GPU.
 * TSD_E_ARG for a NULL table. */
int tsd_drive_table(int32_t* table);
/* The pose after n_steps steps of the rule's trajectory at step length step_q16 and heading increment `turn`, cell and offset
 * renormalised (x = x0 + (X_n >> 16), fx = X_n & 65535), the heading h_n of the rule, the layer kept: the pose a controller should
 * expect after it has executed the first steps of its arc.  out may be p.  Host code, no GPU.  TSD_E_ARG for a NULL pointer, an
 * offset outside 0 .. 65535, a heading outside 0 .. TSD_DRIVE_HEADINGS - 1, |x| or |y| above 1 << 30, step_q16 outside 0 .. 65536,
 * |turn| above TSD_DRIVE_HEADINGS / 8, n_steps outside 0 .. TSD_DRIVE_MAX_STEPS. */
int tsd_drive_advance(const tsd_drive_pose* p, int step_q16, int turn, int n_steps, tsd_drive_pose* out);
/* The choice of n_robots robots on the route result the context holds: choice_host[r]; where given, scores_host[r * V * Wn + index]
 * (TSD_DRIVE_NONE where the sample is refused) and why_host[r * V * Wn + index]; nothing else is written.  One launch for all robots
 * ("drive_rollout": one wave per sample, its lanes over 64 consecutive steps; the re-roll of each robot's winner for its record runs
 * right behind it under the same name) on the stream of the route result, waited for, under the same lock as the frontier, route and
 * view calls.  Scratch stays with the context and grows on demand: a repeated call of the same shape allocates nothing.  TSD_E_ARG,
 * with the outputs and the context's results left as they were: no route result, a NULL params, poses, choice_host or list, a count
 * or value outside the ranges above, a pose with its cell outside the map (a cell with w == 0 is legal), an offset outside
 * 0 .. 65535 or a heading outside 0 .. TSD_DRIVE_HEADINGS - 1, n_robots outside 1 .. TSD_DRIVE_MAX_ROBOTS. */
int tsd_drive_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_pose* poses, int n_robots,
                      tsd_drive_choice* choice_host, uint64_t* scores_host /* or NULL */, uint16_t* why_host /* or NULL */);
/* The same on the fields result: robot r reads the keys of layer poses[r].layer.  TSD_E_ARG also without a fields result and for a
 * layer outside 0 .. layers - 1. */
int tsd_drive_fields_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_pose* poses, int n_robots,
                             tsd_drive_choice* choice_host, uint64_t* scores_host /* or NULL */, uint16_t* why_host /* or NULL */);
/* The context's drive block on the device and its capacity in 32-bit words: the direction table in its first 2 * TSD_DRIVE_HEADINGS
 * words, the last call's samples behind it.  Valid until a drive call that needs a larger block or tsd_destroy; a repeated call of
 * the same shape leaves both as they are.  Each pointer may be NULL.  TSD_E_ARG before the first drive call. */
int tsd_drive_dev_ptrs(tsd_ctx* ctx, const void** block_dev, unsigned long long* words);
/* The fleet form: the choice of n_robots robots on the fields result as tsd_drive_fields_rollout makes it, but the robots decide one
 * after the other and each one's arcs are rated against the arcs CHOSEN by those that decided before it (prioritised planning in
 * space-time).  The trajectory, the reasons 1 .. 5, the score and the minimum are those of the rule above; one reason is added.
 *   order          order[n_robots], a permutation of 0 .. n_robots - 1: order[0] decides first (rank 0)
 *   parked         a pose with layer == -1: the robot takes no samples; its choice is the record without an admissible sample, its
 *                  scores are TSD_DRIVE_NONE and its `why` 0; it stands at its pose for every k and counts as decided before
 *                  order[0], whatever its place in `order`
 *   positions      P_r(k) = ((x0 << 16) + X_k, (y0 << 16) + Y_k), int64, k = 0 .. T: the absolute Q16 position of robot r at step k of
 *                  an arc; of a decided robot: of the arc it chose, its pose ((x0 << 16) + fx, (y0 << 16) + fy) for every k where
 *                  it is parked or found no admissible sample.  All robots share T and the lists, so step k is one instant for all
 *   distance       against a robot q decided before r (a parked one, or one of a lower rank), dx, dy = P_r(k) - P_q(k):
 *                  D_k = dx^2 + dy^2 where |dx| < sep_q16 and |dy| < sep_q16, "far" otherwise -- larger than any number; the
 *                  products stay below 2^47
 *   step k is refused   (1 <= k <= T) by the first of 1, 2, 3, 4 above, and then by
 *                    6  for some such q: D_k is not far, D_k < sep_q16^2, and D_k <= D_{k-1} (D_0 from the two poses).  The last
 *                       clause is the way out: two robots that stand closer than the separation may still take arcs on which every
 *                       step takes them further apart; without it neither could ever move
 *                  and reason 5 stays behind step T.  The smallest refusing k wins with its first reason: why = (6 << 12) | k
 *   tracks         where given, tracks_host[(r * (T + 1) + k) * 2 + {0, 1}] = P_r(k) of the arc robot r chose (its pose in every slot
 *                  without one)
 * With sep_q16 == 0, or with one robot, choices, scores and `why` equal tsd_drive_fields_rollout's byte for byte.  The robot of
 * rank 0 depends on no other robot but the parked ones.  Every rank's choice is a minimum over its samples: the result does not
 * depend on how the work is scheduled.  One launch rates every robot's arcs on the map as tsd_drive_fields_rollout does; then each
 * rank takes two small launches on the same stream -- its samples against the tracks decided so far (a table read, a 64-bit product
 * and the in-wave scan per lane, no map bytes) and the winner's record and track -- so ranks are ordered by kernel boundaries: no
 * workgroup waits for another and the host waits once, at the end.  All of it is timed as "drive_fleet".  The block of
 * tsd_drive_dev_ptrs serves this call too (it holds the map pass's per-sample results as well, so it is larger at the same shape).
 * TSD_E_ARG, with the outputs and the context's results left as they were: what tsd_drive_fields_rollout refuses (but layer -1), a
 * layer below -1, a NULL fleet or order, an order that is no permutation, sep_q16 outside 0 .. TSD_DRIVE_MAX_SEP. */
#define TSD_DRIVE_MAX_SEP (128 * 65536)
/* The key under each robot's pose on the fields result, for a priority by cost-to-go: togo_host[r] = the key of layer
 * poses[r].layer at the cell (poses[r].x, poses[r].y) -- d = key >> 4, and the low bits hold the layer's seed index, so keys of
 * different layers never tie --, TSD_ROUTE_NONE where the cell has no key and for a parked robot (layer -1).  One small launch and
 * one copy back on the fields result's stream, waited for; offsets and headings are not read.  TSD_E_ARG: no fields result, a NULL
 * pointer, n_robots outside 1 .. TSD_DRIVE_MAX_ROBOTS, a cell outside the map, a layer outside -1 .. layers - 1. */
int tsd_drive_fields_togo(tsd_ctx* ctx, const tsd_drive_pose* poses, int n_robots, uint32_t* togo_host);
typedef struct {
  const int32_t* order;         /* [n_robots], host memory */
  int32_t sep_q16;              /* 0 .. TSD_DRIVE_MAX_SEP */
  int32_t reserved;
} tsd_drive_fleet_params;       /* 16 bytes */
int tsd_drive_fleet_rollout(tsd_ctx* ctx, const tsd_drive_params* params, const tsd_drive_fleet_params* fleet, const tsd_drive_pose* poses,
                            int n_robots, tsd_drive_choice* choice_host, uint64_t* scores_host /* or NULL */, uint16_t* why_host /* or NULL */,
                            int64_t* tracks_host /* or NULL */);
/* The live layer: what a scanner sees this instant, kept off the arcs.  The three rollouts above read the weight image of a route or
 * fields result, which was made from a map published some time ago; a context may hold beside it at most one live layer, made from
 * the end points of the current scans, and while one is set the rollouts refuse every arc that enters it.
 *   the layer      a bit per cell of a width x height image, rows padded to 32-bit words: bit x & 31 of word
 *                  y * stride_words + (x >> 5) is the cell (x, y), stride_words = (width + 31) / 32; the tail bits of a row's last
 *                  word are always 0
 *   points         n pairs (px, py), int32: the map cell of a scan end point, |px|, |py| <= 1 << 30 -- a point may lie outside the
 *                  map --, 0 <= n <= TSD_DRIVE_LIVE_MAX_POINTS; n == 0 is legal and gives an empty layer that is set
 *   skip discs     n_skip <= TSD_DRIVE_LIVE_MAX_SKIP triples (ox, oy, ro), |ox|, |oy| <= 1 << 30, 0 <= ro <= 1 << 15: a point is
 *                  dropped where (px - ox)^2 + (py - oy)^2 <= ro^2 for some disc (products in 64 bits; a point further than ro from
 *                  the centre along one axis is outside without a product).  The discs are the robots themselves: one robot's
 *                  scanner sees another robot's body, and a robot that stands inside a stamped disc could not move
 *   radius         r in 0 .. TSD_DRIVE_LIVE_MAX_RADIUS cells
 *   the live set   L: every cell (x, y) inside the map with (x - px)^2 + (y - py)^2 <= r^2 for some point that was not dropped
 * Every set rebuilds the layer whole from its own points: no ray clearing, no decay, and no bit of the set before it survives.
 * While a layer is set, tsd_drive_rollout, tsd_drive_fields_rollout and tsd_drive_fleet_rollout refuse step k by the first of 1, 2,
 * 3, 4 as above, and then by
 *                    7  c_k lies in L or, failing that, for the lowest body point b whose cell lies in L (every such cell lies
 *                       inside the map: 4 has passed)
 * and in the fleet form reason 6 follows: at one step the order is 1, 2, 3, 4, 7, 6.  The smallest refusing k wins with its first
 * reason, reason 5 stays behind step T; why = (7 << 12) | k.  The layer refuses and never rates: score, choice, tie order, tracks and
 * the winner's record are those of the rule above over the samples that are left.  c_1 is tested also where it is the start's
 * cell, as for w == 0: a robot that stands on a live cell cannot move, and the skip discs are the caller's way out.  The corner rule
 * (3) is NOT restated for live cells: a disc of r >= 1 is 4-connected, so no centre passes diagonally between two of its cells, but
 * at r == 0 a centre can slip diagonally between two live cells.  A layer whose width or height differ from the result's image
 * makes the three rollouts return TSD_E_ARG, outputs and results left as they were.  Without a layer -- the state of a new context
 * and after tsd_drive_live_clear -- the three rollouts answer byte for byte as they do without this section (the kernels keep an
 * instantiation without the test).  The route and fields calls do not read the layer: plans still lead through live cells.
 * The calls below take no lock of their own: like the other drive calls they run under the lock the caller holds for the frontier,
 * route and view calls (one thread per context at a time). */
#define TSD_DRIVE_LIVE_MAX_POINTS 32768
#define TSD_DRIVE_LIVE_MAX_SKIP   16
#define TSD_DRIVE_LIVE_MAX_RADIUS 64
typedef struct {
  int32_t radius;               /* r: 0 .. TSD_DRIVE_LIVE_MAX_RADIUS */
  int32_t n_skip;               /* 0 .. TSD_DRIVE_LIVE_MAX_SKIP */
  const int32_t* skip;          /* [3 n_skip] triples (ox, oy, ro), host memory; may be NULL where n_skip == 0 */
} tsd_drive_live_params;        /* 16 bytes */
/* Sets the layer from n points for a width x height image, sides 1 .. TSD_FRONTIER_MAX_SIDE; *n_kept, where given, is the number of
 * points no disc dropped.  The old layer is emptied (one memset of the bit image), then one launch
 * ("drive_live": a thread per (point, row of its disc): the skip test, the row's half-width floor(sqrt(r^2 - dy^2)) from a table the
 * host builds per call with integer arithmetic, the span clipped to the map and written as word masks with atomic ORs) on the
 * context's stream, waited for.  Scratch -- the bit image, a block for the points -- stays with the context and grows on demand: a
 * repeated set of the same shape allocates nothing.  TSD_E_ARG, with the previous layer left in place: a NULL params, a NULL
 * points_xy where n > 0, a NULL skip where n_skip > 0, a count, radius, coordinate or side outside the ranges above. */
int tsd_drive_live_set(tsd_ctx* ctx, const tsd_drive_live_params* params, const int32_t* points_xy /* [2 n], host */, int n,
                       int width, int height, int* n_kept /* or NULL */);
/* No layer: the rollouts are those of the rule without the layer again.  Legal without a layer. */
int tsd_drive_live_clear(tsd_ctx* ctx);
/* The layer's words, stride_words * height of them, into words_host (cap_words: its capacity in words), and its shape; each pointer
 * may be NULL (words_host NULL: the shape alone).  TSD_E_ARG without a layer, or where cap_words is too small. */
int tsd_drive_live_fetch(tsd_ctx* ctx, uint32_t* words_host, long long cap_words, int* width, int* height, int* stride_words);
/* The layer on the device.  Valid until a set that needs a larger image or tsd_destroy.  TSD_E_ARG without a layer. */
int tsd_drive_live_dev_ptr(tsd_ctx* ctx, const void** words_dev, int* width, int* height, int* stride_words);

/* ---- views: what a scan from a cell would uncover, and who is about to see it ------------------------------------ */
/* The expected information gain of candidate cells (exploration goals) and the coordination rule on top of it: what one robot is
 * about to see is no longer worth a visit by another.  Input: an int8 map on the context's device as for the frontiers and routes --
 * width x height, `stride` bytes from row to row, bytes beyond `width` in a row never read, sides 1 .. TSD_FRONTIER_MAX_SIDE.  In
 * integers throughout (the kernels do no floating point), so a restatement agrees to the byte (tests/view_ref.py).
 *   cell classes   unknown: v < 0; clear: 0 <= v <= free_max; blocking: v > free_max; free_max in 0 .. 99.  A cell outside the map
 *                  is neither seen nor passed
 *   targets        for a candidate c = (cx, cy) and a radius R in 1 .. TSD_VIEW_MAX_RADIUS the 8R cells of the Chebyshev ring of
 *                  radius R around c, in this order: the top row, x from -R to R at y = -R; the right column, y from -R + 1 to R;
 *                  the bottom row, x from R - 1 to -R; the left column, y from R - 1 to -R + 1
 *   ray to (tx, ty) step j = 1 .. R lies at the offset o(j) = (sgn(tx) * ((2 j |tx| + R) / 2R), sgn(ty) * ((2 j |ty| + R) / 2R)) by
 *                  integer division: a closed form in j, no accumulated error term; consecutive steps differ by at most one cell
 *                  per axis and |ox|, |oy| never decrease
 *   a ray ends     before step j -- step j and everything behind it stay unseen -- at the first j where, tested in this order,
 *                  1. ox^2 + oy^2 > R^2 (the range is a disc), 2. the cell lies outside the map, 3. the step is diagonal against
 *                  step j - 1 and both cells it cuts, (x_j, y_j-1) and (x_j-1, y_j), are blocking or outside the map (an
 *                  8-connected wall drawn on the diagonal is a wall), 4. the cell is blocking.  Otherwise the cell is seen; if it
 *                  is unknown and unknown_depth > 0, the ray ends behind the unknown_depth-th unknown cell it has seen (the
 *                  candidate's own cell is no step and does not count).  unknown_depth 0: no such end
 *   V(c)           the cells seen by any of the 8R rays, plus c itself.  A candidate outside the map (cell >= width * height) or on
 *                  a blocking cell has an empty V: its record holds its cell and zeros
 *   record         visible = |V|, unknown = the unknown cells of V, gain = the unknown cells of V that are not claimed (= unknown
 *                  where claims are not in use); every cell counts once however many rays cross it
 *   claims         a uint8 image (0 / 1) of width x height that belongs to the context; claim(c) stores 1 on every unknown cell of
 *                  V(c) -- byte stores of one value, no atomics on global memory --, so claiming is idempotent and independent of order
 * The scanner is taken to see all around (the robot can turn): its field of view and beam count are not modelled. */
#define TSD_VIEW_MAX_RADIUS 511
#define TSD_VIEW_MAX_CELLS  4096
typedef struct {
  int32_t free_max;             /* 0 .. 99 */
  int32_t radius;               /* R, in cells: 1 .. TSD_VIEW_MAX_RADIUS */
  int32_t unknown_depth;        /* >= 0; 0: a ray does not end in unknown space */
  int32_t use_claims;           /* tsd_view_gains: 0 / 1, gain leaves out the claimed cells */
} tsd_view_params;              /* 16 bytes */
typedef struct {
  uint32_t cell;                /* the candidate, as given */
  uint32_t gain, unknown, visible;
} tsd_view_gain;                /* 16 bytes */
/* The records of n candidates (linear indices y * width + x, host memory; 1 .. TSD_VIEW_MAX_CELLS of them), one workgroup each, whose
 * seen set is a bit mask of the candidate's window in LDS sized by the radius.  map_dev != NULL: any map on the context's device; the
 * call runs on the context's stream.  map_dev == NULL: the staged map of the context's last frame or update (width, height and
 * stride are ignored), on the context's copy stream behind the frame's event, under tsd_route_frame's conditions and refusals.
 * Either way the call waits; the grid and its write ledger are not touched.  Candidates, records, claims and their pinned copies stay
 * with the context and grow on demand, so a repeated call at the same size allocates nothing.  One view call at a time per context,
 * under the same lock as the frontier and route calls.  TSD_E_NOMEM (tsd_last_error says which buffer) where the device cannot
 * hold it.  TSD_E_ARG, with the claims image left as it was: a NULL params, cells or out, n outside 1 .. TSD_VIEW_MAX_CELLS, a
 * radius outside 1 .. TSD_VIEW_MAX_RADIUS, free_max outside 0 .. 99, unknown_depth < 0, a side outside 1 .. TSD_FRONTIER_MAX_SIDE,
 * stride < width, use_claims without a claims image of the map's width and height. */
int tsd_view_gains(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                   const uint32_t* cells_host, int n, tsd_view_gain* out_host);
/* claim(c) for n candidates: the same rays, a store pass in place of the count.  use_claims is ignored.  TSD_E_ARG as above, and
 * without a claims image of the map's width and height. */
int tsd_view_claim(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                   const uint32_t* cells_host, int n);
/* Allocates the claims image at width x height, or clears it; on the context's stream, waited for.  TSD_E_ARG for a side outside
 * 1 .. TSD_FRONTIER_MAX_SIDE. */
int tsd_view_claims_reset(tsd_ctx* ctx, int width, int height);
/* The claims image on the device (uint8, rows of `width` bytes), valid until the next reset at a larger size or tsd_destroy.  Each
 * pointer may be NULL.  TSD_E_ARG without an image. */
int tsd_view_claims_dev_ptr(tsd_ctx* ctx, const void** claims_dev, int* width, int* height);
/* The coordination rule, on the goals of a route plan (tsd_route_goals_fetch; host memory, 0 .. TSD_VIEW_MAX_CELLS of them) for
 * robots 0 .. n_robots - 1 (the route's seeds; 1 .. TSD_FRONTIER_MAX_SEEDS):
 *   1. the claims are reset at the map's size;  2. the goals with cell != TSD_ROUTE_NONE and 0 <= seed < n_robots are remaining;
 *   3. a round takes the gains of all remaining goals with claims in use;  4. it scores (int64) gain * gain_weight - dist;
 *   5. it picks the highest score, on a tie the lower goal index;  6. it stops if that goal's gain is 0;
 *   7. it gives the goal to robot `seed` and claims V of its cell;  8. it drops that goal and every goal with the same seed;
 *   9. it goes on while goals remain.
 * goal_of_robot[r]: the index of robot r's goal, -1 where it got none; picked[r] (may be NULL): that goal's record as its round saw it,
 * {TSD_ROUTE_NONE, 0, 0, 0} without a goal; *rounds: the rounds begun (at most n_robots), each one launch for the gains, one wait and,
 * where a goal was given, one launch for the claim.  The limit of the rule: a robot is only ever offered the goals it is nearest to,
 * because the route's key image holds one field for all seeds (tsd_view_assign_fields lifts it).  The claims image holds the claims of the goals given when the call
 * returns.  The map source, the stream and the refusals are tsd_view_gains'; TSD_E_ARG also for n_goals or n_robots out of range, a
 * NULL goals with n_goals > 0, a NULL goal_of_robot or rounds -- the claims image is left as it was then. */
int tsd_view_assign(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                    const tsd_route_goal* goals, int n_goals, int n_robots, uint32_t gain_weight,
                    int32_t* goal_of_robot /* n_robots, -1: none */, tsd_view_gain* picked /* n_robots or NULL */, int* rounds);
/* The coordination rule across robots, on the goal matrix of a fields plan (tsd_route_fields_goals_fetch, row by row into host
 * memory: goals[r * n_frontiers + f]).  Pair (r, f) stands for robot r and frontier f; cell_rf and dist_rf are goals[r][f]'s.
 *   1. The claims are reset at the map's size.
 *   2. Every pair with goals[r][f].cell != TSD_ROUTE_NONE is remaining.  Each robot drives to ITS cheapest cell of the frontier.
 *   3. A round takes the gains, with claims in use, of the cells of all remaining pairs.  Each distinct cell is rated once.  A launch
 *      takes at most TSD_VIEW_MAX_CELLS candidates, so a round makes as many launches as that needs.
 *   4. score(r, f) = gain(cell_rf) * gain_weight - dist_rf in int64.
 *   5. Only pairs with gain > 0 compete.  The highest score wins.  On a tie the lower f wins, then the lower r.
 *   6. The call stops when no pair competes.
 *   7. goal_of_robot[r] = f, picked[r] is that record, and V(cell_rf) is claimed.
 *   8. Every pair of robot r and every pair of frontier f is dropped.
 *   9. The call goes on while pairs remain.  There are at most min(n_robots, n_frontiers) rounds.
 * Step 5 differs from tsd_view_assign on purpose: there a best-scored goal with gain 0 ends the call; here such a pair does not
 * compete, and a pair with a gain behind it may still win.  Limits: n_frontiers in 0 .. TSD_VIEW_MAX_CELLS, n_robots in 1 ..
 * TSD_FRONTIER_MAX_SEEDS.  goal_of_robot[r]: the FRONTIER index f of robot r's goal (its goal is goals[r][f]), -1 where it got none;
 * picked[r] (may be NULL): the record of cell_rf as its round saw it, {TSD_ROUTE_NONE, 0, 0, 0} without a goal; *rounds: the rounds
 * that took gains, the one in which no pair competed included; each makes its launches for the gains with one wait apiece and, where
 * a pair won, one launch for the claim and one wait.  Host logic over the views' launches, like tsd_view_assign: the map source,
 * the stream and the refusals are its, with n_frontiers in n_goals' place -- the claims image is left as it was on a refusal, and
 * holds the claims of the cells given when the call returns. */
int tsd_view_assign_fields(tsd_ctx* ctx, const void* map_dev, int width, int height, int stride, const tsd_view_params* params,
                           const tsd_route_goal* goals /* [r * n_frontiers + f] */, int n_frontiers, int n_robots, uint32_t gain_weight,
                           int32_t* goal_of_robot /* n_robots, -1: none */, tsd_view_gain* picked /* n_robots or NULL */, int* rounds);

/* ---- the map's surface as an ordered point list --------------------------------------------------------------- */
/* The `coords` array of RayCastAxisAligned2D::calcCoords (RayCastAxisAligned2D.cpp:13-105), point for point and in its serial order:
 * the linear zero crossings of the TSD along every row and column of every initialised tile of the processed ring (tiles 1 .. PX-2 in
 * x and y, y outer; inside a tile the row scans py = 0..32, px = 1..32, then the column scans px = 0..32, py = 1..32, over the 33 x 33
 * form with the halo), in fp64 and in the reference's operation order -- the points tsd_occupancy rounds into its 100 marks, so n
 * equals its n_surface.  A seam point that two tiles find appears twice, as in the reference.  Coordinates are the grid's own (the ray
 * cast's model points).
 * Normals: TsdGrid::interpolateNormal (TsdGrid.cpp:517-546) AT EACH POINT.  (The reference passes the array's base pointer, so every
 * normal it writes is the first point's: not reproduced.)  normal_ok[i] = 0 and normal (0, 0) where one of the four bilinear look-ups
 * fails; a length <= 10e-6 leaves the normal unnormalised with normal_ok = 1.
 * params == NULL: the whole grid, with normals.  Otherwise the tiles [tx0, tx1) x [ty0, ty1), clipped to the processed ring: the
 * sublist those tiles contribute, in the same order; an empty window gives n = 0 and enqueues nothing.
 * tsd_surface_extract runs on the context's stream, behind every push enqueued before it, and returns when the list is complete on
 * the device; it reads the grid and writes nothing but the context's surface buffers (kept and grown geometrically: no allocation
 * where the capacity suffices).  The grid must not be written while the call runs, as for every reading entry point.
 * tsd_surface_fetch copies points [first, first + count) of the last list: xy[2 * count] interleaved, normals[2 * count] and
 * normal_ok[count] where given.  TSD_E_ARG for a range outside [0, n) and for normals / normal_ok after an extraction without them.
 * tsd_surface_dev gives the device arrays themselves (normals / ok NULL after an extraction without normals), valid until the next
 * extraction on the context or tsd_destroy. */
typedef struct {
  int32_t tx0, ty0, tx1, ty1;   /* tiles, half open */
  int32_t want_normals;
  int32_t reserved;
} tsd_surface_params;
int tsd_surface_extract(tsd_ctx* ctx, const tsd_surface_params* params, int* n);
int tsd_surface_fetch(tsd_ctx* ctx, int first, int count, double* xy, double* normals, uint8_t* normal_ok);
int tsd_surface_dev(tsd_ctx* ctx, const double** xy_dev, const double** normals_dev, const uint8_t** ok_dev, int* n);

/* ---- map-to-map alignment: surface points against the TSD ------------------------------------------------------ */
/* Which rigid transform carries one map into another?  tsd_align_points places a list of points (the surface of another map) in this
 * context's grid; tsd_map_align takes the list from a second context.  Two stages, both on the device: a search over a pose lattice
 * scored on the TSD (as tsd_relocalize, over map points and without its free-space gate), then a point-to-TSD Gauss-Newton refinement
 * of the K best peaks, all peaks in one launch.
 *
 * Lattice: candidate (ix, iy, k), idx = (k * ny + iy) * nx + ix, carries a point p to R_k * (p - pivot) + (x0 + ix * step_xy,
 * y0 + iy * step_xy): a lattice node is where the PIVOT lands, the rotation turns about the pivot (about the origin, one degree would
 * move a point 13 m away by 0.2 m and smear the peaks).  The lattice fields have tsd_reloc_params' meaning and limits.
 * Coarse score (k_align_score): over the coarse points -- every stride-th point of the list, stride = ceil(n / TSD_MAX_ICP_POINTS), minus
 * the pivot (fp64 subtraction) -- the sum of 1048576 - (uint32)rint(fabs(v) * 1048576.0), v = TsdGrid::interpolateBilinear at
 * ((c*px - s*py) + t.x, (s*px + c*py) + t.y), over the look-ups that succeed: tsd_relocalize's sum (one copy of the loop), no gate.  Peaks
 * as there.
 * Refinement (k_align_refine), per peak, state m = where the pivot lands (the node), (c, s) = the peak's rotation, gain = 1, prev = 0.
 * One accumulation at the state, over ALL n points, p relative to the pivot: q = ((c*px - s*py) + m.x, (s*px + c*py) + m.y);
 * v = interpolateBilinear(q), (nx, ny) = TsdGrid::interpolateNormal(q) (TsdGrid.cpp:517-546, normalised); the point counts (n_ok) when
 * all five look-ups succeed and the unnormalised normal's length is > 10e-6; u = v / v_cut, w = (1 - u*u)^2 for |u| < 1, else 0 (Tukey);
 * r = v * max_truncation; J = (nx, ny, nx * (-(q.y - m.y)) + ny * (q.x - m.x)); sums[11] = the six entries of A = sum w J J^T
 * (00 01 02 11 12 22), b = -sum w J r, sum w, sum w r^2.  Every thread sums its points in index order, the workgroup's sums are
 * reduced in a fixed order, no floating-point atomics: the same call twice gives the same bits.
 * The iteration: accumulate; n_ok < 3: "degenerate", stop.  Converged, or `iterations` steps done: stop.  Solve A d = b by LDL^T without
 * pivoting (fp64); a pivot <= 0 (or NaN): "degenerate", stop.  If d.prev < 0 in the metric dx*dx' + dy*dy' + lever^2 * dth*dth', gain =
 * max(gain / 2, 1/16) (without this the iteration falls into a two-cycle on the kinks of the bilinear field); d *= gain; prev = d.
 * (c, s) <- (c - s*dth, s + c*dth) / hypot(1, dth), renormalised by its own hypot (no sine on the device); m += (dx, dy).  Converged
 * when hypot(dx, dy) < eps and lever * |dth| < eps; the sums of the record are then taken once more at the final state.
 * Winner: the peak with the largest sum w whose status is not degenerate, the earlier peak keeps a tie (decided on the host).
 * What the lattice has to be: the refinement sees a point only inside the cut, |tsd| < v_cut, i.e. within v_cut * max_truncation of
 * a surface, so some node must bring most points that close: step_xy of the order of v_cut * max_truncation, and a rotation step of
 * that length divided by the distance of the farthest surfaces from the pivot, unless near surfaces can pull the far ones in.
 *
 * The list sits half a cell below the field: calcCoords places a crossing between cells px-1 and px at (px - 1 + interp) * cs, while
 * interpolateBilinear takes a cell's value to lie at its centre (px + 0.5) * cs.  A surface list is displaced by (-cs/2, -cs/2) against
 * the zero set the look-ups read; tsd_map_align therefore stages p + (cs_src/2, cs_src/2).  tsd_align_points takes its points as
 * they are: in field coordinates.  tsd_surface_* is unchanged. */
#define TSD_ALIGN_MAX_POINTS (1 << 20)
#define TSD_ALIGN_MAXITER    0   /* status of a peak: `iterations` steps without meeting eps */
#define TSD_ALIGN_CONVERGED  1
#define TSD_ALIGN_DEGENERATE 2
typedef struct {
  double  x0, y0, step_xy;      /* as tsd_reloc_params */
  int32_t nx, ny, ntheta;
  int32_t theta_wraps;
  const double* cos_sin;
  double  theta0, dtheta;
  int32_t K;                    /* peaks to refine, 1 .. TSD_RELOC_MAX_PEAKS */
  int32_t iterations;           /* Gauss-Newton steps at most, 0 .. 64 (0: the coarse pose with its sums) */
  double  pivot_x, pivot_y;     /* in the points' (src's) coordinates, finite; tsd_map_align with both NaN: the centre of src's grid */
  double  v_cut;                /* Tukey cut on the normalised tsd, in (0, 1]; 0 = the default 0.75 */
  double  eps;                  /* metres, > 0; 0 = the default 1e-6 */
  double  lever;                /* metres per radian in the step metric; <= 0: half of dst's grid width */
  double  min_overlap, max_rms; /* found = converged, sum w / n >= min_overlap, rms <= max_rms (max_rms <= 0: no limit) */
} tsd_align_params;
typedef struct {                /* one refined peak (tsd_debug_align_peaks) */
  int32_t  idx;                 /* lattice candidate */
  uint32_t score;
  int32_t  status;              /* TSD_ALIGN_* */
  int32_t  iterations;          /* steps taken */
  int32_t  n_ok;
  int32_t  reserved;
  double   m[2], c, s;          /* the final state */
  double   gain;
  double   sums[11];            /* at the final state */
} tsd_align_peak;
typedef struct {
  int32_t  found;
  int32_t  winner_idx;          /* candidate index of the winning peak, -1 without one */
  double   T33[9];              /* src -> dst, 3x3 row-major: rotation (c, s), translation m - R * pivot; NaN without a winner */
  double   coarse_x, coarse_y, coarse_cos, coarse_sin;   /* the winner's lattice pose (where the pivot lands) */
  uint32_t winner_score;
  int32_t  n_peaks, n_refined, iterations, converged;
  int32_t  n, stride, n_ok;
  double   weight_sum, rms, overlap;   /* sum w, sqrt(sum w r^2 / sum w), sum w / n */
  double   info[6];             /* A at the end (00 01 02 11 12 22): the information matrix a pose graph would take */
  int32_t  cell_off[2];         /* the whole-cell shift nearest to T in tsd_fuse's cell_off_xy convention for the pair (dst at 0, src at
                                 * cell_off): src's cell (x, y) is dst's cell (x + cell_off[0], y + cell_off[1]) */
  double   cell_error;          /* largest distance, in dst cells, between T p and p + cell_off * cs over the four corners p of src's grid
                                 * (tsd_align_points: of a square of dst's size): < 0.5 says a whole-cell shift describes T */
  double   search_ms, refine_ms;/* tsd_profile_enable: stream time of scores + peaks and of the refinement launch; 0 otherwise */
} tsd_align_result;
/* points_xy: n points x0 y0 x1 y1 .. in field coordinates, on the host or (on_device != 0) on ctx's device, complete before the call;
 * 1 <= n (TSD_E_ARG) <= TSD_ALIGN_MAX_POINTS (TSD_E_CAPACITY); every coordinate finite and within TSD_RELOC_MAX_REACH grid widths
 * (TSD_E_ARG; a device list is checked by the staging kernel and refused when the call's one wait returns).  Contract of tsd_relocalize:
 * every argument is checked before the context is touched, refused with TSD_E_ARG while a scan of the context is in flight, only the
 * grid is read (no cell, flag, ledger state or sensor changes), the call waits for its result, tsd_destroy frees the buffers kept
 * (the score volume up to 2^23 candidates, the staged list, the records).  No peak or only degenerate ones: TSD_OK with found = 0. */
int tsd_align_points(tsd_ctx* ctx, const tsd_align_params* params, const double* points_xy, int n, int on_device,
                     tsd_align_result* result);
/* The transform that carries src's map coordinates into dst's.  dst and src distinct contexts on one device (TSD_E_ARG otherwise), no
 * scan of either in flight.  Runs tsd_surface_extract(src, NULL, &n) -- it REPLACES src's last surface list --, stages p + cs_src/2 into
 * a buffer dst owns (a small kernel on dst's stream) and calls tsd_align_points.  n == 0 is no error: found = 0.  A caller that
 * serialises each context with a lock of its own holds both for the call. */
int tsd_map_align(tsd_ctx* dst, tsd_ctx* src, const tsd_align_params* params, tsd_align_result* result);
/* TEST HOOK: the score volume of the last alignment of this context, as tsd_debug_reloc_scores */
int tsd_debug_align_scores(tsd_ctx* ctx, uint32_t* scores, int cap);
/* TEST HOOK: the per-peak records of the last alignment, in the peaks' order: copies min(n, cap), returns n */
int tsd_debug_align_peaks(tsd_ctx* ctx, tsd_align_peak* records, int cap);
/* TEST HOOK: one accumulation of the refinement kernel (its own code, iterations = 0) over n host points at the state (m, c, s) with
 * pivot[2] and v_cut: sums[11] and n_ok */
int tsd_debug_align_sums(tsd_ctx* ctx, const double* points_xy, int n, const double pivot[2], const double m[2], double c, double s,
                         double v_cut, double sums[11], int* n_ok);

/* ---- same-device merge group: N grids of one process on ONE GPU, one merged occupancy map ------------------ */
/* The one-GPU counterpart of include/tsd_comm.h (whose RCCL all-reduce needs one GPU per rank): n contexts of this process on one
 * device, member i shifted by (cell_off_xy[2i], cell_off_xy[2i+1]) whole cells, merged by a local kernel into a width x height window.
 * Member i's cell (x, y) lands in cell (x + ox_i, y + oy_i) of the offsets' frame; a merged cell is the SIGNED int8 maximum over the
 * members that cover it (what ncclMax gives: occupied 100 > free 0 > unknown -1, and any other int8 value in its signed order), -1 where
 * no member covers it; what falls outside the window is clipped.  width = height = 0: the window is the members' bounding box, and its
 * corner (tsd_group_corner) is (min ox, min oy); an explicit window has its corner at (0, 0).  The members must be distinct contexts
 * on one device with bit-equal cell sizes (their map sizes may differ), 1 <= n <= 64; anything else is refused before the first HIP
 * call: tsd_group_create returns NULL with a message on stderr, the calls below return TSD_E_ARG.  Part of libtsd_hip.so: no RCCL.
 *
 * Nothing waits on the host before tsd_group_merge_wait.  tsd_group_merge_begin enqueues every member's extraction
 * (tsd_occupancy_dev_async, into the group's buffer for that member) on that member's own stream; the group's own stream waits for
 * them through events, runs the merge kernel and the copy to merged_host (width * height bytes, row = y; page-locked memory from
 * tsd_host_alloc keeps the call from blocking; NULL: no copy).  A member's next extraction waits on the device for the merge that
 * still reads its buffer.  One merge at a time per group: call tsd_group_merge_wait before the next begin if merged_host is reused.
 * A caller that serialises each context with a lock of its own (the C++ facade) enqueues the members one by one with
 * tsd_group_extract_begin, holding only that member's lock, and then calls tsd_group_merge_maps_begin(g, NULL, host).
 * The contexts must outlive the group. */
typedef struct tsd_group tsd_group;
tsd_group*  tsd_group_create(int n, tsd_ctx* const* ctxs, const int32_t* cell_off_xy /* 2n, NULL = all 0 */,
                             int width, int height /* 0, 0 = bounding box of the members */);
void        tsd_group_destroy(tsd_group* g);
int         tsd_group_size(const tsd_group* g);
int         tsd_group_width(const tsd_group* g);
int         tsd_group_height(const tsd_group* g);
int         tsd_group_corner(const tsd_group* g, int32_t* x0, int32_t* y0);   /* the window's corner in the offsets' frame */
const char* tsd_group_last_error(const tsd_group* g);
int   tsd_group_merge_begin(tsd_group* g, const tsd_map_params* params, int8_t* merged_host);
/* member i's extraction alone (ordered on its context's stream), for tsd_group_merge_maps_begin(g, NULL, ...) */
int   tsd_group_extract_begin(tsd_group* g, int i, const tsd_map_params* params);
/* the merge of maps the caller wrote: member_maps_dev[i] is member i's map on the device (cells_i * cells_i int8, row = y, 16-byte
 * aligned, complete before the call), NULL = the group's own buffers (tsd_group_member_map_dev; extractions begun on them are waited for) */
int   tsd_group_merge_maps_begin(tsd_group* g, const void* const* member_maps_dev, int8_t* merged_host);
/* copy a host map (cells_i * cells_i bytes) into the group's buffer of member i, on the group's stream ahead of the next merge */
int   tsd_group_member_map_upload(tsd_group* g, int i, const int8_t* map_host);
int   tsd_group_merge_wait(tsd_group* g, int* n_occupied /* cells equal to 100 in the merged map; may be NULL */);
void* tsd_group_map_dev(tsd_group* g);          /* merged map, width * height int8, row = y */
void* tsd_group_member_map_dev(tsd_group* g, int i);
/* what a merge costs, measured with HIP events when switched on: the members' extractions (summed over members) and the merge
 * kernel; tsd_group_merge_times waits for the merges issued so far and returns the running totals since tsd_group_create */
int   tsd_group_profile(tsd_group* g, int on);
int   tsd_group_merge_times(tsd_group* g, double* extract_ms_total, double* merge_ms_total, int* merges);

/* ---- the same group under rigid transforms: members rotated and shifted by fractions of a cell ------------------ */
/* Member i is placed by a rigid transform T_i (3x3 row-major) that carries its grid coordinates (metres from the grid's corner, the
 * coordinates tsd_map_align speaks) into the group's frame: c = T[0][0], s = T[1][0], t = (T[0][2], T[1][2]).  The merged window is
 * W x H cells of the members' common cell size cs with its corner at (x0, y0) in frame cells.  For window cell (X, Y) and member i,
 * all in fp64, in this order, every operation rounded on its own (no contraction):
 *   px = ((double)(x0 + X) + 0.5) * cs;   py = ((double)(y0 + Y) + 0.5) * cs        the cell's centre in the frame
 *   dx = px - t.x;   dy = py - t.y
 *   qx = c*dx + s*dy;   qy = c*dy - s*dx                                            T_i^-1 of the centre
 *   u = qx / cs;   v = qy / cs
 *   kx in [ceil(u - 1.25), floor(u + 0.25)],   ky in [ceil(v - 1.25), floor(v + 0.25)]
 * The footprint: the source cells whose centre (k + 0.5) lies within 0.75 cells (Chebyshev) of the back-projected centre, 1 or 2 cells
 * per axis.  Member i's value at (X, Y) is the SIGNED int8 maximum over the footprint cells that lie inside the member (0 <= kx, ky <
 * cells_i); if none does, the member does not cover the cell.  The merged cell is the signed maximum over the covering members, -1
 * without one: the group's rule above.  No occupied cell is dropped: the centre of an occupied source cell lands in some window cell D,
 * and D's centre back-projects to within 0.5 * sqrt(2) < 0.75 cells of that source centre on both axes, so the source cell is in D's
 * footprint (a nearest-neighbour warp loses cells of walls one cell thick; here a wall may thicken to two cells, the "occupied wins"
 * bias the maximum has anyway).  At c = 1, s = 0 and a whole-cell translation the fractions of u and v are .5, a quarter cell from
 * both thresholds: the footprint is the one source cell and the result is tsd_group_create's, byte for byte.
 *
 * width = height = 0: the window is the bounding box of the members.  Over the corners (x, y) in {0, L_i}^2, L_i = (double)cells_i * cs,
 * of every member, carried to ((c*x - s*y) + t.x, (s*x + c*y) + t.y):  x0 = floor(min_x / cs + 1e-9), x1 = ceil(max_x / cs - 1e-9),
 * W = x1 - x0, and y likewise (the 1e-9 keeps 17 * cs / cs from falling to 16; with whole-cell identity transforms the box is
 * tsd_group_create's).  An explicit window has its corner at frame cell (0, 0).  tsd_group_corner gives (x0, y0).
 *
 * T33: 9n doubles, NULL = identities.  tsd_group_create's conditions hold (one device, bit-equal cell sizes, distinct contexts, 1 .. 64
 * members, sides 0 or 1 .. 65536); refused as well, before the first HIP call, with NULL and a message on stderr: an entry that is not
 * finite, a last row other than (0, 0, 1), |T00 - T11| or |T01 + T10| above 1e-12 (shear, reflection), |c*c + s*s - 1| above 1e-9 (scale),
 * a translation beyond 2^24 cells, a bounding box over 65536 cells.  Every other tsd_group_* call works on such a group as on a
 * translation group, with the same ordering; tsd_group_merge_maps_begin launches k_group_merge_rigid. */
tsd_group* tsd_group_create_rigid(int n, tsd_ctx* const* ctxs, const double* T33 /* 9n, NULL = identities */, int width, int height);
/* member i's transform into the group's frame; on a translation group the shift (ox_i * cs, oy_i * cs) as a transform */
int   tsd_group_member_transform(const tsd_group* g, int i, double T33[9]);
/* the members' whole-cell offsets (what tsd_group_create and tsd_fuse_begin take) when every member is a whole-cell shift, by the
 * group's own decision (tsd_group_create: always; tsd_group_create_rigid: no rotation, within 1e-6 cells); TSD_E_ARG otherwise */
int   tsd_group_cell_offsets(const tsd_group* g, int32_t* cell_off_xy /* 2n */);

/* ---- TSD-level fusion: the grids of several robots on ONE GPU fused into one grid ------------------------------- */
/* dst becomes the grid that would have seen every member's scans: member i's cell (x, y) is dst's cell (x + ox_i, y + oy_i), offsets
 * in whole cells, any integer in +-2^24 (no multiple of 32 is asked for); members are clipped to dst, what no member reaches becomes
 * unknown, dst's previous content is discarded.  dst is an ordinary context afterwards: ray cast, localise, push, store, colour image.
 *
 * Contribution of member i at one of its cells: an initialised tile gives (tsd, weight) where tsd is not NaN and nothing where it is;
 * an uninitialised tile with _initWeight > 0 (an "empty" tile, shorthand for tsd = 1, W = _initWeight: TsdGridPartition::init) gives
 * (1.0, _initWeight); anything else gives nothing.  The fused cell, contributors in member order, fp64, no contraction:
 *   none          (NaN, 0)
 *   exactly one   (t, min(w, 32)), verbatim: fusing one grid at offset 0 is an identity
 *   several       num = 0 + t1 w1 + t2 w2 + ..., den = 0 + w1 + w2 + ..., summed left to right; den > 0: (num / den, min(den, 32));
 *                 den == 0 (cells freed by tsd_free_footprint): (t of the first contributor, 0)
 * A dst tile is materialised when a member's initialised tile intersects its 32 x 32 cells; otherwise it stays unmaterialised when
 * its 1024 fused cells are all equal (_initWeight = their weight, 0 for unknown) and is materialised with those cells when they are not
 * (the empty tiles of members shifted by less than a tile).  _initWeight of a tile materialised by the first rule is that of the first
 * member (member order, then source tile row by row) whose initialised tile intersects it, 0 by the second rule.  Every halo cell of a
 * materialised tile holds the fused state of the grid cell it duplicates, (NaN, 0) beyond the grid's edge.  The ray cast's sign masks
 * are rebuilt, the push bookkeeping is left as after tsd_reset.  Bit-exactness is claimed for fp64 cell storage.
 *
 * Refused with TSD_E_ARG before the first HIP call and with the grids untouched (tsd_last_error(dst) names the reason): n outside
 * 1 .. 64, a NULL member, dst among the members, a member listed twice, members on another device than dst, a member whose cell size
 * or max_truncation differs bitwise from dst's, an offset outside +-2^24.
 *
 * Everything runs behind events; the host waits for nothing before tsd_fuse_wait.  The kernel runs on dst's stream, behind whatever
 * dst's own ordering asks for and behind every grid write the members have enqueued so far (the push stream of the asynchronous
 * mapping included); what a member enqueues after the call runs behind the kernel.  The call holds the members' and dst's internal
 * locks while it enqueues; a caller that serialises each context with a lock of its own holds those of all contexts involved for
 * the duration of tsd_fuse_begin only.  tsd_destroy of a member or of dst with a fusion in flight is safe.  The counters: tiles of
 * dst by representation, cells_valid = cells of dst with a fused value = cells_one_source + cells_many_sources (contributors). */
typedef struct tsd_fuse_stats {
  int64_t tiles_materialised, tiles_empty, cells_valid, cells_one_source, cells_many_sources;
} tsd_fuse_stats;
int tsd_fuse_begin(tsd_ctx* dst, int n, tsd_ctx* const* src, const int32_t* cell_off_xy /* 2n, NULL = 0 */);
int tsd_fuse_wait(tsd_ctx* dst, tsd_fuse_stats* stats /* may be NULL */);
int tsd_fuse(tsd_ctx* dst, int n, tsd_ctx* const* src, const int32_t* cell_off_xy, tsd_fuse_stats* stats);

/* ---- measurement ----------------------------------------------------------------------------- */
/* Per-kernel HIP-event timing on the ctx stream.  Kernel names: "push_classify", "push_update",
 * "push_halo", "raycast", "icp", "occupancy", "tsdpdf", "fuse", "clearance" (both kernels of tsd_clearance_dev), and the passes of
 * tsd_frontiers_dev: "frontier_tile", "frontier_seam", "frontier_flatten" (each once for the frontiers and once more for the regions
 * where seeds are given), "frontier_rank" (count, scan, emit), "frontier_stats" (with the min_size compaction), and those of
 * tsd_route_dev, tsd_route_goals and tsd_route_trace: "route_init", "route_relax" (a batch of rounds), "route_goals", "route_trace",
 * tsd_route_waypoints' launch behind its trace: "route_waypoints" (tsd_route_fields_waypoints' as well),
 * the same passes of tsd_route_fields_dev / _goals / _trace: "route_fields_init", "route_fields_relax", "route_fields_goals",
 * "route_fields_trace",
 * tsd_drive_rollout's and tsd_drive_fields_rollout's launch: "drive_rollout", tsd_drive_fleet_rollout's launches: "drive_fleet",
 * tsd_drive_live_set's emptying and stamp: "drive_live",
 * and the launches of tsd_view_gains and tsd_view_claim on the context's stream: "view_gain", "view_claim". */
int tsd_profile_enable(tsd_ctx* ctx, int on);
/* restrict timing to a comma separated list of kernel names, or "all"; a "/n" suffix times every n-th
 * launch only (two event records cost ~13 us of stream time per timed launch); a name may carry its own
 * period, "push_update:1,all/8" = every dispatch of k_push_update, every 8th of the others */
int tsd_profile_select(tsd_ctx* ctx, const char* kernels_csv);
int tsd_profile_reset(tsd_ctx* ctx);
int tsd_profile_get(tsd_ctx* ctx, const char* kernel, double* total_ms, int* launches);
/* spread of the timed dispatches of one kernel since the last reset: shortest, longest, standard deviation (ms) */
int tsd_profile_get_spread(tsd_ctx* ctx, const char* kernel, double* min_ms, double* max_ms, double* std_ms);
/* the timed dispatches themselves, in launch order (ms; at most 65 536 are kept): copies up to `cap` of them, returns how many there are */
int tsd_profile_get_samples(tsd_ctx* ctx, const char* kernel, float* ms_out, int cap);

/* Counter calibration for profiles/: `reps` launches of k_calib_rmw, a read-modify-write of two arrays
 * of n_doubles fp64 values with the push kernel's 8-byte-per-lane access shape (known traffic: 16 B read
 * + 16 B written per element and launch).  Allocates and frees its own scratch. */
int tsd_calibrate_rmw(tsd_ctx* ctx, int64_t n_doubles, int reps);

/* The box's own stream bandwidth with the push kernel's access shape: `reps` event-timed launches of k_calib_rmw over two
 * arrays of n_doubles (each read and written once per launch: 32 B per element).  Choose n_doubles so that the footprint
 * (16 B per element) exceeds the 256 MiB Infinity Cache, or the figure is a cache bandwidth.  GB/s, best and mean launch. */
int tsd_measure_stream(tsd_ctx* ctx, int64_t n_doubles, int reps, double* gbs_best, double* gbs_mean);

/* Sum of the work counters of every push completed on this ctx since the last reset (the numerator of
 * the algorithmic-bytes formula without a host sync per push).  Waits for pushes still in flight. */
int tsd_push_stats_total(tsd_ctx* ctx, tsd_push_stats* total, int64_t* pushes, int reset);

/* registration_mode 3 inside the fused scan (ThreadLocalize.cpp:557-567 with the call structure of tsd_scan): arms the
 * pre-registration -- obvious::TSD_PDFMatching::match, as tsd_tsdpdf_match -- for the NEXT tsd_scan_submit / tsd_scan of this sensor.
 * It then runs on the device between that scan's ray cast (whose hits are its model) and its registration (whose Tinit it becomes,
 * Icp.cpp:481-486): PCA normals of both point sets, extractSamples, pickControlSet, the trial picks and the candidate list in the
 * reference's serial order, scoring, arg-max -- nothing returns to the host in between.  scene_xy_2B / mask_s: what
 * Sensor::dataToCartesianVectorMask gives for the scan (beam-indexed); the draws as in tsd_tsdpdf_match.  One-shot.  The inputs are
 * copied at the call (the caller's buffers are free on return) and travel to the device on the side stream right away.  It may be
 * called while a scan of this sensor is in flight (submitted, not yet collected): it then arms the scan AFTER that one, and the copy is
 * ordered behind the in-flight scan's own pre-registration kernels (refused with TSD_E_ARG when that needs a larger layout than the
 * in-flight scan's: arm it after the collect).
 * Several robots on one grid: a sensor armed this way may be part of a tsd_batch_begin -- its pre-registration then runs inside the
 * batch, on the grid's stream behind the batch's ray casts (all armed robots score against the grid as it is before any push of the
 * batch; the reference runs `case TSD` in every robot's own thread, ThreadLocalize.cpp:557-567), and its result is that robot's Tinit.
 * Armed and unarmed sensors may share a batch.  Not while the sensor has a batched / split scan in flight. */
int tsd_scan_preregister(tsd_sensor* s, const tsd_tsdpdf_params* params, const double* scene_xy_2B, const uint8_t* mask_s,
                         const int* draws_subsample, const int* draws_control, const int* draws_trials);
/* Asynchronous mapping for the fused scan of this sensor.  The reference's ThreadMapping is a thread of its own: queuePush returns at
 * once and the push lands when the mapping thread gets to it (ThreadMapping.cpp:51-76), so the localiser's next ray cast may or may not
 * see it.  on = 0 (default): strict order -- the next scan's ray cast sees this scan's push.  on = 1: the next scan's ray cast is taken
 * right behind this scan's registration, on a grid WITHOUT this scan's push (exactly one push behind, every scan: one of the
 * reference's interleavings, and a deterministic one), and the push runs beside the next registration on a stream of its own.  Every
 * other entry point of the context is ordered behind a push still in flight there.  Not while a scan is in flight. */
int tsd_sensor_set_async_mapping(tsd_sensor* s, int on);
/* TEST HOOK: every asynchronous push of this context is held back by `microseconds` on the push stream (a one-wave kernel ahead of
 * it), 0 = off.  Lets a test make the push stream lag behind the registrations the way a busy device can
 * (tests/test_gpu_async_mapping.py: the scan / table buffers of a lagging push must not be re-staged under it). */
int tsd_debug_stall_push_stream(tsd_ctx* ctx, unsigned int microseconds);
/* TEST HOOK: on = 0 makes every registration of this context search for itself in its first step instead of taking that step's
 * nearest neighbours from the helper workgroups the launch brings by default (icp_kernels.hip: IcpSeed).  The results are the same
 * either way, bit for bit (tests/test_gpu_parity.py::test_icp_helpers_change_nothing); only the time differs. */
int tsd_debug_set_icp_helpers(tsd_ctx* ctx, int on);
/* TEST HOOK: on = 0 makes tsd_batch_push enqueue one push per robot, in the batch's order (the reference's mapper: one sensor after the
 * other, ThreadMapping.cpp:43-76), instead of the one pass per tile that applies the robots' updates in that order inside every tile
 * (csrc/push_multi.hip).  The grids are the same cell for cell, halo included (tests/test_gpu_batch.py). */
int tsd_debug_set_push_multi(tsd_ctx* ctx, int on);
/* TEST HOOK: how a scan of this sensor reaches the device -- 1: the host stores it into device memory through the PCIe BAR (the default
 * wherever the device's memory is mapped into the host's address space and the start-up probe's kernel read back what the host wrote),
 * 0: through a pinned host buffer (no such mapping, or TSD_SCAN_PINNED=1), 2: as 1 with TSD_SCAN_BAR_VERIFY's device-side cross-check. */
int tsd_debug_sensor_scan_path(const tsd_sensor* s);

/* the pre-registration's outcome for the scan collected last (TBest, probability, winning pair, counts) */
int tsd_scan_preregistration_result(tsd_sensor* s, tsd_tsdpdf_result* result);

#ifdef __cplusplus
}
#endif
#endif /* TSD_HIP_H */
