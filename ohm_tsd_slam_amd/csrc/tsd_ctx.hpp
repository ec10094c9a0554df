// tsd_ctx.hpp -- host-side state behind the opaque tsd_ctx of include/tsd_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <mutex>

#include "tsd_device.hpp"
#include "grid_ledger.hpp"
#include "scan_ledger.hpp"
#include "../../include/tsd_hip.h"

namespace tsd {

// scalar inputs of a push, passed by value as a kernel argument
struct PushArgs {
  double Pi[6];              // first two rows of pose^-1
  double trx, try_;          // Sensor::getPosition
  double phi_min, ang_res_inv, phi_lower, phi_upper;
  double max_range, min_range, low_refl;
  int beams;
  int enabled;               // 0: this push was gated off on the device (fused scan): every kernel is a no-op
};

struct RaycastArgs {
  double Pi[6];
  double trx, try_;
  double gxmin, gymin, gxmax, gymax;   // RayCastPolar2D::_xmin.. (RayCastPolar2D.cpp:128-146)
  double idx_min, idx_max;             // _idxMin / _idxMax (:148-149)
  int beams;
  int pad;
};

struct IcpArgs {
  double P[6];               // first two rows of the pre-registration sensor pose
  double min_x, max_x, min_y, max_y;
  double thr0, min_sqr, multiplier;    // DistanceFilter state (DistanceFilter.cpp:11-20)
  int iterations;
  int n_model, n_scene;      // direct mode
  int beams;                 // fused mode (compaction from per-beam arrays) when > 0
  int ccw;                   // model slots ascend counter-clockwise about the sensor (1) or clockwise (0)
  int estimator;             // TSD_ESTIMATOR_*
  double Tinit[6];           // rows 0, 1 of Icp::iterate's Tinit (identity in registration_mode 0)
  const double* Tinit_dev;   // the same on the device (fused registration_mode 3: the pre-registration's result, first six doubles), or nullptr
};

struct IcpResultDev {
  double T[9];
  double rms;
  int pairs, iterations, state, n_model, n_scene, reserved;
};

// what one fused scan reports (layout of tsd_scan_result in include/tsd_hip.h)
struct ScanResultDev {
  IcpResultDev icp;
  double pose[9];
  int reg_error, pushed, no_model, reserved;
  unsigned long long seq;    // the scan's sequence number
};
// On its way to the host the record travels as SCAN_RESULT_WORDS tagged 8-byte words {low half of seq, four bytes of the record}
// (scan_post_body): the pinned buffer holds those, the host decodes them into a ScanResultDev of its own once all carry the tag.
constexpr int SCAN_RESULT_WORDS = (int)(sizeof(ScanResultDev) / 4);
static_assert(sizeof(ScanResultDev) % 8 == 0 && SCAN_RESULT_WORDS <= 64, "ScanResultDev: one store instruction of one wave");

// gates of ThreadLocalize (ThreadLocalize.cpp:593-600, :728-736; ThreadLocalize.h:63-64)
struct GateArgs {
  double reg_trs_max, reg_sin_rot_max, trs_min, rot_min;
};

// device-resident SensorPolar2D + ThreadLocalize pose bookkeeping of one robot (fused scan path)
struct SensorDev {
  double pose[9];            // Sensor::_T
  double last_pose[9];       // ThreadLocalize::_lastPose
  int have_last_pose;
  int pad;
  double last_angle;         // ThreadLocalize::calcAngle(_lastPose), kept with it (the push gate needs it every scan)
  RaycastArgs rc;            // arguments of the NEXT ray cast / registration, derived from `pose`
  double icpP[6];
  PushArgs push;             // arguments of this scan's push (enabled = gate result)
  unsigned long long done_seq;   // sequence number of the latest scan whose epilogue has written all of the above (device scope):
                                 // what the gate kernel ahead of a batched robot's push waits for (launch_wait_seq)
};

// fused scan path: what k_icp's epilogue needs (st == nullptr: plain registration)
struct ScanPostArgs {
  SensorDev* st;
  double* rays;              // world ray map of the sensor, turned in place
  ScanResultDev* out;        // coherent host memory
  unsigned long long seq;
  GateArgs gates;
  double gmin_x, gmax_x, gmin_y, gmax_y;   // TsdGrid::getMin/Max* (RayCastPolar2D's isInsideGrid)
  int beams;
  int publish_done;          // also publish st->done_seq (agent-scope release): a gate kernel on another stream waits for it (batched scans)
  PushArgs* push_copy;       // asynchronous mapping: where this scan's push arguments are left for a push that runs beside the NEXT
                             // registration (whose epilogue rewrites st->push); nullptr = strict order, the push reads st->push
};

// Where a ray cast and a registration run and what they write: the context's own stream and buffers (ctx_target: the unfused entry
// points and the fused scan) or a sensor's (sensor_target: tsd_scan_begin).  Always filled completely; launch_raycast and launch_icp
// take it as an argument.
struct LaunchTarget {
  hipStream_t stream;
  double* coords; double* normals; uint8_t* mask_m;    // the ray cast's outputs = the registration's model
  IcpResultDev* icp_res; double* trace;
  void* icp_seed; int icp_seed_points;                 // the registration's helper hand-off (icp_seed_bytes(points))
};

// One push as the host describes it: the arguments on the device, the scan, its range-query tables (launch_push_tables, ordered before
// the push), where the host knows the sensor to be (cx, cy) and how far the device-side pose may be from there (slack), and what sizes
// the launches (beams: LDS; max_range: tile window).
struct PushJob {
  const PushArgs* a_dev; const double* ranges; const uint8_t* mask; char* rmq;
  double cx, cy, slack;
  int beams; double max_range;
};

// ---- batched scans (tsd_batch_*): one launch of each kernel for the robots of a batch; block (.., y) of the batched ray cast /
// block x of the batched registration and tables kernels read their arguments from entry y / x of these device arrays
struct RaycastBatchEntry {
  const RaycastArgs* a_dev; const double* rays;
  double* coords; double* normals; uint8_t* mask;
};
constexpr int RC_BATCH_BYVAL = 16;     // ray-cast entries that travel as kernel arguments (640 B): no copy to wait for
struct RaycastBatchArgs { RaycastBatchEntry e[RC_BATCH_BYVAL]; };
struct TablesBatchEntry {
  const double* ranges; const uint8_t* mask; char* rmq;
  double phi_min, ang_res;
  int beams, pad;
};
// step 0's searches of a registration, done by helper workgroups (icp_kernels.hip, ICP_HELPER_POINTS): the hand-off granules
// ([2][stride] 8-byte {launch number, value}), this launch's number, the helper workgroups the launch brings
struct IcpSeedArgs { unsigned long long* g; unsigned int seq; int helpers; int stride; };
struct IcpBatchEntry {
  IcpArgs a;
  const double* P_dev; const double* coords; const uint8_t* mask_m; const double* rays_local; const double* ranges;
  const uint8_t* mask; IcpResultDev* out; double* trace; const double* normals;
  ScanPostArgs post;
  const unsigned int* rc_flag;       // the slot's hand-off words (nullptr: the stream waited already): [0] number of the latest batch
                                     // whose ray casts are done, [1] number of the latest batch the host gave up on (tsd_batch_begin failed)
  unsigned int rc_target;
  unsigned int poll_bound;           // polls (about a microsecond each) before the wait gives up and REPORTS it (BATCH_FAIL_*)
  IcpSeedArgs seed;
};
// why a batched registration did not run (ScanResultDev::reserved / tsd_scan_result.reserved; 0 = it ran)
constexpr int BATCH_FAIL_TIMEOUT = 1;    // its ray casts never reported done within the poll bound
constexpr int BATCH_FAIL_ABORTED = 2;    // the host abandoned the batch
constexpr unsigned int BATCH_POLL_BOUND = 1u << 21;   // ~2 s

// A scan as it lies in every scan buffer (the sensors', the batches' staging): ranges[beams] | mask[beams] | mask_push[beams].
struct ScanView { const double* ranges; const uint8_t* mask; const uint8_t* mask_push; };
constexpr size_t scan_bytes(int beams) { return (size_t)beams * 10; }            // what a copy of a scan moves
constexpr size_t scan_alloc_bytes(int beams) { return scan_bytes(beams) + 64; }   // what a buffer for one scan is allocated with
inline ScanView scan_view(const char* base, int beams)
{
  const size_t nb = (size_t)beams;
  return ScanView{reinterpret_cast<const double*>(base), reinterpret_cast<const uint8_t*>(base + nb * 8), reinterpret_cast<const uint8_t*>(base + nb * 9)};
}
// (a scan without a mask of its own for the push is pushed with the registration's)
inline void scan_pack(char* dst, int beams, const double* ranges, const uint8_t* mask, const uint8_t* mask_push)
{
  const size_t nb = (size_t)beams;
  std::memcpy(dst, ranges, nb * 8);
  std::memcpy(dst + nb * 8, mask, nb);
  std::memcpy(dst + nb * 9, mask_push ? mask_push : mask, nb);
}

constexpr size_t KERNEL_TIMER_SAMPLES = 65536;
struct KernelTimer {
  double total_ms = 0.0;
  double sum_sq = 0.0, min_ms = 1e300, max_ms = 0.0;   // of the timed dispatches (tsd_profile_get_spread)
  int launches = 0;
  unsigned tick = 0;         // launches seen (sampling: every profile_every-th one is timed)
  std::vector<float> samples;    // the timed dispatches themselves, in order (tsd_profile_get_samples; at most KERNEL_TIMER_SAMPLES are kept)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// The score volume of a pose-lattice search (reloc.hip): one uint32 per candidate of the last search.  Relocalisation and alignment
// keep one each.  Up to RELOC_KEEP_CANDIDATES it stays with the context for the next search and for the debug entry points.
struct ScoreVolume {
  uint32_t* d = nullptr; size_t cap = 0;   // [cap]
  int nx = 0, ny = 0, ntheta = 0;          // shape of the last search (0: none)
  int ensure(tsd_ctx* ctx, size_t candidates);
  void drop();
  // tsd_debug_*_scores: copies min(n, room) scores to the host, returns n = nx * ny * ntheta
  int copy_out(tsd_ctx* ctx, uint32_t* scores, int room) const;
  // a volume beyond RELOC_KEEP_CANDIDATES is given back when the call that holds this ends, whichever way it ends
  struct GiveBack { ScoreVolume& v; ~GiveBack(); };
};

}  // namespace tsd

struct tsd_sensor;
struct tsd_ctx {
  int device = 0;
  int n_cus = 256;                           // compute units of the device (MI355X: 256): persistent grids are sized by it
  hipStream_t stream = nullptr;
  std::mutex order_mutex;                    // the ordered sections of the concurrent multi-robot path and every grid-writing entry point
  std::mutex misc_mutex;                     // timers / per-kernel attribute cache: touched by launches that run outside the caller's lock
  unsigned long long ticket = 0;             // order of the ray casts / pushes of the concurrent multi-robot path
  unsigned long long last_push_ticket = 0;
  std::vector<tsd_sensor*> sensors;          // device sensors attached to this grid (multi-robot mode, SlamNode.cpp:101-122)
  std::vector<struct tsd_batch*> batches;    // batch slots of the multi-robot path
  hipEvent_t ev_grid = nullptr;              // "every grid write enqueued so far is done" (recorded on `stream` by tsd_scan_begin)
  tsd::GridDev grid{};
  int map_log2 = 0;
  std::string err;

  // push state
  char* d_rmq2[2] = {nullptr, nullptr};      // range-query tables of an unfused tsd_push (k_push_tables), used in turn (next_ctx_tables):
  int rmq_slot = 0;                          // the next scan's tables are built while the current push still reads its own
  std::map<const void*, size_t> lds_configured;   // dynamic LDS every kernel was configured for on this context's device (ensure_dynamic_lds)
  hipEvent_t ev_h2d = nullptr;               // fused scan: the scan's copy (side stream) is complete
  uint32_t* d_tile_rec = nullptr;            // [tiles] what the last push did to every tile
  uint8_t* d_dirty = nullptr;                // [tiles] written by freeFootprint since the last push
  uint32_t* d_tile_totals = nullptr;         // [tiles][8] records summed over the pushes since the last reset
  unsigned long long* d_pushes = nullptr;    // [2] pushes since the last reset, pushes whose launch window missed the sensor
  uint32_t* d_list = nullptr;               // [tiles] work list of the current push (tile | kind << 28)
  uint32_t* d_list_h = nullptr;             // [tiles] the UPDATE tiles of that list k_push_halo has work for (materialised by the push, or dirty)
  char* d_list_aux = nullptr;               // [tiles] PushListAux of every list entry (push_kernels.hip): beam window, partition weight,
                                            // the linear forms of k_push_update's beam estimate
  tsd::PushArgs* d_push_args = nullptr;     // arguments of an unfused tsd_push (the fused scan keeps them in the sensor state)
  unsigned int* d_list_cnt = nullptr;       // by push parity: UPDATE tiles listed, other tiles listed, the ticket heads of k_push_update's tile queue
  unsigned int push_parity = 0;
  // The grid's write ledger (grid_ledger.hpp): the epoch, the push launches' tile window, what the next windowed frame covers.  Its
  // methods are the only writers.  The grid-writing entry points of the split and batched paths and the frame's begin call them under
  // order_mutex (WriterScope, frame_begin); the fused scan, which takes no lock, and the unfused entry points that only outdate a ray
  // cast call them under the caller's own grid mutex (host/: obvious::TsdGrid::mutex(), which also covers frame_begin there).  One
  // grid is driven either way, never both at once.  (frame_wait reports a failed copy with neither lock held.)
  tsd::GridLedger ledger;
  hipStream_t stream2 = nullptr;             // side stream: the tables are built while ray cast / ICP run
  // asynchronous mapping (tsd_sensor_set_async_mapping): the fused scan's push on a stream of its own, beside the next registration
  hipStream_t stream_push = nullptr;
  hipEvent_t ev_async_rc = nullptr;          // "the next scan's ray cast has read the grid" (recorded on `stream`)
  hipEvent_t ev_async_push = nullptr;        // "the push enqueued last on stream_push is done" (one of a sensor's ev_slot_push[], not owned)
  unsigned int debug_push_stall_us = 0;      // tsd_debug_stall_push_stream (tests)
  bool async_pending = false;                // a push on stream_push that `stream` has not been ordered behind yet
  hipEvent_t ev_tables = nullptr;

  // scan staging: ring of pinned slots + device buffers
  static constexpr int kSlots = 8;
  int slot = 0;
  char* h_stage[kSlots] = {};
  hipEvent_t stage_ev[kSlots] = {};
  size_t stage_bytes = 0;
  double* d_ranges = nullptr;    // [TSD_MAX_BEAMS]
  uint8_t* d_mask = nullptr;     // [TSD_MAX_BEAMS]
  double* d_rays = nullptr;      // [2*TSD_MAX_BEAMS] world rays
  double* d_rays_local = nullptr;// [2*TSD_MAX_BEAMS]
  double* d_coords = nullptr;    // [2*TSD_MAX_BEAMS]
  double* d_normals = nullptr;   // [2*TSD_MAX_BEAMS]
  double* d_mnormals = nullptr;  // [2*TSD_MAX_ICP_POINTS] model normals of tsd_icp_normals, in the model's slot order
  uint8_t* d_mask_m = nullptr;   // [TSD_MAX_BEAMS]
  double* d_model = nullptr;     // [2*TSD_MAX_ICP_POINTS]
  double* d_scene = nullptr;     // [2*TSD_MAX_ICP_POINTS]
  int* d_morig = nullptr;        // [TSD_MAX_ICP_POINTS] original index of every angle-sorted model point
  int* d_start = nullptr;        // [TSD_MAX_ICP_POINTS] first search slot of every scene point
  int icp_shape = 0;             // 0 = default workgroup shape (env TSD_ICP_SHAPE for experiments)
  int push_multi = 1;            // the pushes of a batch of robots in one pass per tile (push_multi.hip; tsd_debug_set_push_multi: 0 = one push per robot)
  void* d_mp_mask = nullptr; void* d_mp_rec = nullptr; void* d_mp_list = nullptr;      // its per-window-tile masks, (tile, robot) records, tile list
  size_t mp_tiles = 0; unsigned mp_parity = 0;
  int icp_helpers = 1;           // step 0's searches by helper workgroups (tsd_debug_set_icp_helpers: 0 = the registration searches itself)
  void* d_icp_seed = nullptr;    // their hand-off buffer (icp_seed_bytes(TSD_MAX_ICP_POINTS))
  tsd::IcpResultDev* d_icp_res = nullptr;
  double* d_icp_trace = nullptr;            // [TSD_ICP_TRACE_MAX][TSD_ICP_TRACE_STRIDE]
  tsd::IcpResultDev* h_icp_res = nullptr;    // pinned
  char* h_out = nullptr;                     // pinned D2H staging (ray-cast outputs)
  size_t h_out_bytes = 0;

  // TSD_PDF pre-registration (tsdpdf.hip): one device + one pinned staging buffer, grown on demand
  char* d_pdf = nullptr; char* h_pdf = nullptr; size_t pdf_bytes = 0;
  // where the last tsd_pdf_match (mode 2: ungated products, fov counts) / tsd_rn_match (mode 1: cntMatch, maxCntMatch, errSum) left its
  // per-candidate arrays in d_pdf (tsd_debug_pdf_match_scores / tsd_debug_rn_match_scores); any later pre-registration call on this
  // context reuses the buffer and clears the count
  struct { int n = 0, mode = 0; size_t off[3] = {0, 0, 0}; } match_dbg;

  // occupancy
  int8_t* d_occ = nullptr;       // persistent map (ThreadGrid::_occGridContent)
  int* d_occ_count = nullptr;
  unsigned int* d_occ_heads = nullptr;   // sharded counters (two sets, used in turn) of k_occ_mark's work list (occupancy_kernels.hip)
  int occ_parity = 0;
  uint32_t* d_occ_list = nullptr;
  int8_t* d_occ_out = nullptr;   // tsd_occupancy's device staging (allocated on first use, kept)
  hipStream_t stream_io = nullptr; hipEvent_t ev_io = nullptr;   // ... and the stream its copy to the host leaves on (created on first use)
  uint8_t* d_img = nullptr; size_t img_bytes = 0;   // tsd_color_image's (coordinate tables + image), grown on demand
  // ThreadGrid's publication (tsd_map_frame_begin / _wait, map_publish.hip): at most one frame in flight
  char* d_frame = nullptr; size_t frame_bytes = 0;  // device staging: coordinate tables, surface count, map, image (kept, grown on demand)
  int* h_frame_count = nullptr;                     // pinned: the frame's surface count
  hipEvent_t ev_frame = nullptr;                    // on `stream`: the frame's kernels are done
  hipEvent_t ev_frame_done = nullptr;               // on stream_io: the frame's copies to the host are done
  bool frame_inflight = false;
  bool frame_empty = false;                         // the frame in flight is a windowed one that nothing was written for: no copy to wait for
  bool frame_map_valid = false;                     // the staging holds the complete map of the frame or update enqueued last (what
                                                    // tsd_costmap_begin reads once that frame has been waited for)
  // clearance field and cost map (clearance.hip: tsd_clearance_dev, tsd_costmap_begin / _wait).  Scratch of the kernels -- the obstacle
  // bit mask, the per-tile summary, the cost table and its pinned copy -- and the frame's device outputs, all allocated on first use,
  // grown on demand and kept; at most one cost map in flight
  struct Clearance {
    uint8_t* d_mask = nullptr; size_t mask_bytes = 0;
    uint8_t* d_tiles = nullptr; size_t tiles_bytes = 0;
    int8_t* d_table = nullptr; int8_t* h_table = nullptr;   // [TSD_CLEARANCE_MAX_RADIUS^2 + 4]; h_table pinned
    int8_t* d_cost = nullptr; uint16_t* d_dist2 = nullptr; size_t out_cells = 0, dist2_cells = 0;
    size_t cost_cells = 0;                   // the cells of the cost map d_cost holds (0: none yet; what tsd_route_frame asks before it reads d_cost)
    hipEvent_t ev_done = nullptr;            // on stream_io: the cost map's copies to the host are done
    bool inflight = false, empty = false;
    int skip = 1;                            // the tile skip of the column pass (tsd_debug_set_clearance_skip: 0 = every block walks)
  } clearance;
  // frontiers (frontier.hip: tsd_frontiers_dev / _frame / _fetch / _dev_ptrs).  Scratch of the kernels and the last result, allocated on
  // first use, grown on demand and kept.  Every call waits for its own work, so nothing of this is ever in flight between calls
  struct Frontier {
    uint32_t* d_lab = nullptr; uint32_t* d_rank = nullptr; size_t cells = 0;      // the frontiers' labels, the roots' ranks
    uint32_t* d_lab_t = nullptr; size_t cells_t = 0;                              // the regions' labels (calls with seeds only)
    uint8_t* d_any = nullptr; size_t tiles = 0;                                   // [2][tiles]: a tile holds a frontier / a traversable cell
    uint32_t* d_seg = nullptr; size_t segs = 0;                                   // roots per 32 cells of a row, then the scan's block sums
    tsd_frontier* d_rec = nullptr; size_t recs = 0;
    uint32_t* d_res = nullptr; uint32_t* h_res = nullptr;                         // the call's counters and the seeds' roots; h_res pinned
    int n = -1, n_all = 0, W = 0, H = 0;                                          // the last result (n < 0: none)
    int seam_unions = 0, region_seam_unions = 0;
  } frontier;
  // routes (route.hip: tsd_route_dev / _frame / _goals / _trace / _dev_ptrs).  Scratch of the kernels and the last result, allocated on
  // first use, grown on demand and kept.  Every call waits for its own work, so nothing of this is ever in flight between calls
  struct Route {
    uint32_t* d_key = nullptr; size_t keys = 0;                                   // the key images, [layers][cells of the call]
    uint8_t* d_w = nullptr; size_t cells = 0;                                     // the cells' weights (0: not traversable)
    uint8_t* d_act = nullptr; size_t tiles = 0;                                   // [2][layers][tiles of the call]: a tile works in the even / odd rounds
    tsd_route_goal* d_goal = nullptr; size_t goals = 0;
    uint32_t* d_path = nullptr; uint32_t* h_path = nullptr; size_t path_words = 0, h_path_words = 0;   // goal cells, lengths, paths; h_path pinned
    uint32_t* d_res = nullptr; uint32_t* h_res = nullptr;                         // the call's counters; h_res pinned
    uint32_t* d_way = nullptr; uint32_t* h_way = nullptr; size_t way_words = 0, h_way_words = 0;       // waypoint.hip: the records, the waypoints; h_way pinned
    hipStream_t stream = nullptr;                                                 // the stream the result was made on: goals and paths follow it
    bool valid = false;                                                           // the last result (false: none)
    int W = 0, H = 0, n_goals = -1;
    int layers = 1;                                                               // key images in d_key, `cells` apart (route: always 1)
    int sweeps = 0;                                                               // tsd_debug_set_route_sweeps (0: the default; route's holds for both)
    long long tile_visits = 0; int host_waits = 0;
  } route;
  // fields (route.hip: tsd_route_fields_*): a second instance of the same result with one key image per seed.  d_key holds `layers`
  // images (capacity `keys`, in keys), d_act [2][layers][tiles] (capacity `tiles`, in bytes), d_w one weight image (capacity
  // `cells`), d_goal the goal matrix [layers][n_goals].  Neither instance touches the other's buffers
  Route fields;
  // drive (drive.hip: tsd_drive_rollout / tsd_drive_fields_rollout): one device block -- the direction table (uploaded when the block
  // is made), then the call's inputs and outputs (tsd_drive_fleet_rollout: the tracks among them, and behind them the map pass's
  // per-sample rows, which only the device reads) -- and its pinned copy without the table.  Grown on demand and kept; every call
  // waits for its own work
  struct Drive {
    uint32_t* d_buf = nullptr; uint32_t* h_buf = nullptr; size_t words = 0, h_words = 0;
    bool table_ready = false;                // the table has been uploaded into d_buf (cleared whenever d_buf is replaced)
    // the live layer (tsd_drive_live_*): the bit image, and the block of a set's skip discs, half-width table, kept count and points
    // with its pinned copy.  Every call waits for its own work
    struct Live {
      uint32_t* d_words = nullptr; size_t words = 0;
      int32_t* d_pts = nullptr; int32_t* h_pts = nullptr; size_t pts_words = 0, h_pts_words = 0;
      bool set = false;                      // a layer is set: the rollouts test it
      int W = 0, H = 0, stride = 0;
    } live;
  } drive;
  // views (view.hip: tsd_view_gains / _claim / _claims_reset / _assign).  The candidates, their records and the pinned copies of both
  // (one capacity), and the claims image with the size it was reset at (cW == 0: none).  Allocated on first use, grown on demand and
  // kept.  Every call waits for its own work, so nothing of this is ever in flight between calls
  struct View {
    uint32_t* d_cells = nullptr; tsd_view_gain* d_rec = nullptr; uint32_t* h_cells = nullptr; tsd_view_gain* h_rec = nullptr; size_t cap = 0;
    uint8_t* d_claims = nullptr; size_t claims_cap = 0; int cW = 0, cH = 0;
  } view;
  // TSD-level fusion (fuse.hip).  As the destination: the kernel's sharded counters and their pinned copy.  As a member: events of its
  // own -- "every grid write enqueued so far" on its stream / its push stream, "the fusion that read this grid last is done" (recorded
  // on the destination's stream; the member's streams wait for it at once) -- all created on first use
  unsigned long long* d_fuse_stats = nullptr; unsigned long long* h_fuse_stats = nullptr;
  bool fuse_begun = false;
  hipEvent_t ev_fuse_src = nullptr, ev_fuse_src_push = nullptr, ev_fuse_read = nullptr;

  // relocalisation (reloc.hip): the scan points, the rotation table, the score volume of the last search, the per-workgroup and merged
  // peak keys; one device block each, grown on demand, and the pinned copy of the merged keys + their count
  struct Reloc {
    double* d_points = nullptr;              // [2 * TSD_MAX_ICP_POINTS] x0 y0 x1 y1 ..
    double* d_cos_sin = nullptr; size_t rot_cap = 0;
    tsd::ScoreVolume volume;
    unsigned long long* d_keys = nullptr;    // [(RELOC_PEAK_GRID + 1) * 64 + 1]: per-workgroup keys, merged keys, count
    unsigned long long* h_keys = nullptr;    // pinned [64 + 1]
  } reloc;

  // the surface list (surface.hip: tsd_surface_extract / _fetch / _dev): per-window-tile counts and offsets and the per-1024-tile bases
  // of the scan (allocated on first use for the grid's processed ring), the last list (grown geometrically, kept), its pinned total
  struct Surface {
    uint32_t* d_counts = nullptr; uint32_t* d_offsets = nullptr; uint32_t* d_bsum = nullptr;
    unsigned int* h_total = nullptr;         // pinned
    double* d_xy = nullptr; size_t cap = 0;                                  // [2 * cap]
    double* d_normals = nullptr; uint8_t* d_ok = nullptr; size_t ncap = 0;   // [2 * ncap], [ncap]
    int n = 0; bool has_normals = false;     // the last extraction's
  } surface;

  // map alignment (align.hip: tsd_align_points / tsd_map_align): the staged point list, the score volume of the last search (kept like
  // the relocalisation's), the per-peak records and the staging kernel's count of bad coordinates with their pinned copies; the
  // rotation table and the peak keys are tsd_ctx::reloc's
  struct Align {
    double* d_pts = nullptr; size_t pts_cap = 0;     // [2 * pts_cap]
    tsd::ScoreVolume volume;
    tsd_align_peak* d_rec = nullptr;                 // [TSD_RELOC_MAX_PEAKS]
    tsd_align_peak* h_rec = nullptr;                 // pinned [TSD_RELOC_MAX_PEAKS]
    unsigned int* d_bad = nullptr; unsigned int* h_bad = nullptr;   // coordinates refused by the staging kernel (h_bad pinned)
    int n_rec = 0;                                   // records of the last alignment in h_rec
  } align;

  // profiling: bit i of profile_mask times kernel i (names in capi.hip: kKernelNames)
  unsigned profile_mask = 0;
  unsigned profile_every = 1;   // time every n-th launch of a selected kernel ("name/n" in tsd_profile_select)
  unsigned profile_every_k[28] = {};   // a kernel's own period ("name:m"), 0 = the list's
  bool profile = false;
  std::map<std::string, tsd::KernelTimer> timers;
  std::vector<hipEvent_t> event_pool;
};

// device-resident sensor of one robot (tsd_sensor_* / tsd_scan in include/tsd_hip.h): what every scan path uses, then one member per path
struct tsd_sensor {
  tsd_ctx* ctx = nullptr;
  int beams = 0;
  double ang_res = 0, phi_min = 0, max_range = 0, min_range = 0, low_refl = 0;
  bool ccw = true;
  bool posed = false;
  tsd::SensorDev* d_state = nullptr;
  double* d_rays = nullptr;        // [2*beams] world rays, normalised to the cell size
  double* d_rays_local = nullptr;  // [2*beams]
  tsd::ScanResultDev* h_result = nullptr;   // the last record that arrived, decoded (ordinary host memory)
  unsigned long long* h_rwords = nullptr;   // pinned, coherent: SCAN_RESULT_WORDS tagged words, written by the registration's epilogue
  tsd::ScanResultDev* d_result = nullptr;   // device address of h_rwords (ScanPostArgs::out)
  unsigned long long seq = 0;
  double pos[2] = {0, 0};          // host mirror of the sensor position (window of the push launches)
  // Shared by the fused and the split path: scan buffers (tsd::ScanView's layout) and the range-query tables of a scan's push, used in
  // turn -- all three by the fused path, as `ledger` hands them out; 0 / 1 by the split path (split.scan_slot; tables, batched path
  // too: split.rmq_slot).  The tables are allocated on first use (split.ready).
  char* d_scan2[3] = {nullptr, nullptr, nullptr};
  char* d_rmq2[3] = {nullptr, nullptr, nullptr};
  // Where the device's memory is mapped into the host's address space (large PCIe BAR: every MI300-class server), d_scan2[] is
  // fine-grained device memory and the HOST writes a scan straight into it: no pinned copy, no device copy, and the registration reads
  // its 10 KB from local memory (1 us) instead of over the host link (3.5-4 us at the top of every registration: tools/exp/bar.hip).
  bool scan_bar = false;
  // The bookkeeping of the scan paths (scan_ledger.hpp): buffer rotation, which events stand between a buffer and its next writer,
  // staged / submitted / in flight, the ray cast ahead; how the next pre-registration is armed.  Their methods are the only writers.
  // The fused path (tsd_scan_stage / _submit / _collect, tsd_scan_preregister, tsd_sensor_set_async_mapping) calls them under the
  // caller's own grid mutex, like tsd_ctx::ledger; the split and batched paths call split_begin / split_end / split_in_flight and
  // pre_ledger.take / launched_batch from the sensor's own thread (a sensor is driven by one path at a time).
  tsd::ScanLedger ledger;
  tsd::PreLedger pre_ledger;

  // tsd_scan_stage / _submit / _collect
  struct Fused {
    // The same three scans in pinned host memory, where the caller's arrays are copied first.  A scan that was NOT staged ahead is read
    // by its registration from here, over the host link (10 KB, requested at once at the top of k_icp): the registration is launched as
    // soon as the scan is in this buffer, and the device copy + the push's range tables follow on the side stream beside it.
    char* h_scan3[3] = {nullptr, nullptr, nullptr};
    char* hd_scan3[3] = {nullptr, nullptr, nullptr};  // device addresses of h_scan3
    hipEvent_t ev_scan_copy[3] = {nullptr, nullptr, nullptr};   // "the device copy out of h_scan3[i] is done" (before the host rewrites it)
    unsigned int* h_bar_mismatch = nullptr;   // TSD_SCAN_BAR_VERIFY=1: bytes in which a scan's two copies differed on the device (pinned, coherent)
    unsigned int* d_bar_mismatch = nullptr;   // ... its device address
    // the scan that was staged last (ledger.slot()): where it lies and where its push's tables go
    tsd::ScanView scan{};            // in d_scan2[slot]
    tsd::ScanView h_scan{};          // its ranges / mask in h_scan3[slot] (device addresses; scan_bar: the same as `scan`)
    char* rmq = nullptr;
  } fused;

  // asynchronous mapping of the fused path (tsd_sensor_set_async_mapping)
  struct Async {
    bool mapping = false;
    tsd::PushArgs* d_push_slot = nullptr;     // [2] push arguments by scan parity
    hipEvent_t ev_slot_push[3] = {nullptr, nullptr, nullptr};   // "the push that read buffer i is done" (ledger.push_recorded)
  } async;

  // fused registration_mode 3 (tsd_scan_preregister, tsdpdf.hip): inputs of the pre-registration that the next tsd_scan_submit runs
  // on the device between its ray cast and its registration; one device + one pinned buffer, grown on demand (armed or not, copied
  // how, where the collected scan's header / result are: pre_ledger)
  struct PreLayout {
    size_t off_S, off_ms, off_msp, off_dc, off_dt, in_bytes;             // inputs (host -> device each scan)
    size_t off_mo_m, off_mo_s, off_phi_m, off_phi_s, off_C, off_K, off_prob, off_hdr, off_res;
    int n, span, trials, size_control_set, max_cand;
    double phi_max, zrand;
  };
  struct Pre {
    char* d = nullptr; char* h = nullptr; size_t bytes = 0;
    char* h_dev = nullptr;                    // `h` as the device sees it (looked up once per allocation)
    hipEvent_t ev_done = nullptr;             // the in-flight scan's pre-registration kernels have read their inputs (the arg-max's own stop event)
    hipEvent_t ev = nullptr;                  // the pre-registration's inputs are on the device (copied on the side stream by tsd_scan_preregister)
    bool bar = false;         // `d` is fine-grained device memory (tsd_sensor::scan_bar): the host may store the armed inputs into it
    unsigned int* d_flag = nullptr;           // k_icp_pre: the launch number of the last arg-max whose TBest stands (its own small allocation)
    unsigned int seq = 0;
    PreLayout layout{};
  } pre;

  // concurrent multi-robot path (tsd_scan_begin / tsd_scan_wait / tsd_scan_finish): ray cast + registration on the sensor's own stream
  // into its own buffers, created on first use.  The batched path (tsd_batch_*) uses the buffers and `rmq_slot` as well.
  struct Split {
    bool ready = false;
    hipStream_t stream = nullptr;      // ONE stream per sensor: streams are multiplexed onto a few in-order hardware queues
    hipEvent_t ev_rc_done = nullptr, ev_icp_done = nullptr;
    bool rc_event_valid = false;     // ev_rc_done has been recorded at least once
    unsigned long long rc_ticket = 0;            // ticket of the sensor's most recent ray cast ...
    volatile int rc_recorded = 1;                // ... whose ev_rc_done record has been issued (by the sensor's own thread)
    double* d_coords = nullptr; double* d_normals = nullptr; uint8_t* d_mask_m = nullptr;
    tsd::IcpResultDev* d_icp_res = nullptr; double* d_icp_trace = nullptr; void* d_icp_seed = nullptr;
    int scan_slot = 0, rmq_slot = 0;
    char* h_stage2[2] = {nullptr, nullptr};   // pinned staging of the scan, alternating
    tsd_gate_params gates{};         // of the scan in flight (ledger.split_in_flight), and where its push finds ranges / mask_push
    tsd::ScanView scan{};
  } split;
};

// one batch slot of the multi-robot path (tsd_batch_* in include/tsd_hip.h): its own stream, events and staging
struct tsd_batch {
  tsd_ctx* ctx = nullptr;
  int max_scans = 0;
  size_t scan_bytes = 0;             // bytes of one scan (ranges | mask | mask_push) in the staging buffers, 64-byte aligned
  size_t head_bytes = 0;             // bytes of the three entry arrays in front of the scans
  hipStream_t stream = nullptr;
  hipEvent_t ev_rc_done = nullptr, ev_icp_done = nullptr, ev_copy_done = nullptr;
  unsigned int* d_rc_flag = nullptr;    // [2]: number of the slot's latest batch whose ray casts have finished (set by a one-wave kernel
  unsigned int rc_batches = 0;          // behind them on the grid's stream) / that the host abandoned; batches begun on this slot
  bool dev_wait = false;                // the two hand-offs of a batch are waits ON THE DEVICE (proven possible by the probe in
                                        // tsd_batch_create) instead of stream events
  unsigned int poll_bound = tsd::BATCH_POLL_BOUND;
  unsigned int* h_gate_err = nullptr;   // pinned, coherent: set by a push gate (k_wait_seq) whose registration never reported done
  unsigned int* d_gate_err = nullptr;   // its device address
  char* h_stage = nullptr;           // pinned: entries + scans of the batch being enqueued
  char* d_stage2[2] = {nullptr, nullptr};   // device copies, alternating (the pushes of the previous batch still read theirs)
  int stage_slot = 0;
  int n = 0;                         // scans of the batch in flight (0: free)
  bool push_enqueued = false;
  std::vector<tsd_sensor*> sensors;
  std::vector<unsigned long long> seqs;
  std::vector<tsd_gate_params> gates;
  std::vector<size_t> scan_off;      // offset of scan i in d_stage2[slot of the batch]
  char* d_stage_cur = nullptr;
};

namespace tsd {

int set_error(tsd_ctx* ctx, int code, const char* what, hipError_t e);
inline LaunchTarget ctx_target(const tsd_ctx* c)
{
  return LaunchTarget{c->stream, c->d_coords, c->d_normals, c->d_mask_m, c->d_icp_res, c->d_icp_trace, c->d_icp_seed, TSD_MAX_ICP_POINTS};
}
inline LaunchTarget sensor_target(const tsd_sensor* s)    // (after sensor_conc_init(s, true))
{
  const tsd_sensor::Split& p = s->split;
  return LaunchTarget{p.stream, p.d_coords, p.d_normals, p.d_mask_m, p.d_icp_res, p.d_icp_trace, p.d_icp_seed, s->beams};
}
#define TSD_HIP_CHECK(ctx, call)                                                     \
  do {                                                                               \
    hipError_t _e = (call);                                                          \
    if (_e != hipSuccess) return tsd::set_error((ctx), TSD_E_HIP, #call, _e);        \
  } while (0)

// Raises a kernel's dynamic-LDS limit to `bytes` where it is below.  The attribute is per device: remembered per context (and kernel
// instantiation), not per process.
inline int ensure_dynamic_lds(tsd_ctx* ctx, const void* kernel, size_t bytes)
{
  std::lock_guard<std::mutex> lk_misc(ctx->misc_mutex);
  size_t& configured = ctx->lds_configured[kernel];
  if (bytes > configured) {
    TSD_HIP_CHECK(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    configured = bytes;
  }
  return TSD_OK;
}

// Event-timed launch.  Default: the two events are handed to hipExtLaunchKernelGGL, which stamps them with the
// dispatch's own begin / end (the duration rocprofv3 reports, free of the gaps between stream operations).
// around = true brackets whatever the scope enqueues with hipEventRecord (several operations).
struct ScopedKernelTimer {
  tsd_ctx* ctx; const char* name; hipEvent_t a = nullptr, b = nullptr; bool around;
  ScopedKernelTimer(tsd_ctx* c, const char* n, bool around_ = false);
  ~ScopedKernelTimer();
};
void drain_timers(tsd_ctx* ctx);
int drain_async_push(tsd_ctx* ctx);          // asynchronous mapping: order the context's stream behind the push stream's last push (capi.hip)
bool kernel_is_timed(const tsd_ctx* ctx, const char* name);

// per-file launchers.  Which stream a kernel goes to and which buffers it reads and writes are arguments of the call; nothing is
// defaulted below the entry points.  The *_dev pointers are the fused scan path: the kernels then read their pose dependent arguments
// from the device-resident sensor state instead of the by-value copy.
// defer_halo != nullptr: k_push_halo is NOT launched; *defer_halo receives its arguments for the ray cast that follows the push and
// carries that pass in its prologue (launch_raycast(.., halo)) -- or for launch_push_halo() where no such ray cast follows
struct HaloArgs;
int launch_push(tsd_ctx* ctx, hipStream_t stream, const PushJob& job, HaloArgs* defer_halo = nullptr);
int launch_push_halo(tsd_ctx* ctx, hipStream_t stream, const HaloArgs& h, int n_window = 2048);
int launch_push_tables(tsd_ctx* ctx, hipStream_t stream, int beams, const double* d_ranges, const uint8_t* d_mask, char* rmq,
                       double phi_min, double ang_res);
size_t push_rmq_bytes(int beams);
size_t push_list_aux_bytes();
// fused registration_mode 3: normals -> lists -> scoring -> arg-max on `stream`, model = the ray cast's outputs on the device;
// *tinit_dev = where the registration kernel finds Tinit (tsdpdf.hip)
// fold != nullptr: the arg-max is NOT launched; *fold receives what launch_icp(.., pre) needs to carry it
struct IcpPreLaunch;
int launch_preregistration(tsd_ctx* ctx, tsd_sensor* s, hipStream_t stream, const double* d_coords, const uint8_t* d_mask_m,
                           const double* d_pose6, const double** tinit_dev, hipEvent_t before_score = nullptr, IcpPreLaunch* fold = nullptr);
int launch_preregistration_batch(tsd_ctx* ctx, hipStream_t stream, tsd_sensor* const* sensors, int n);
size_t push_list_cnt_bytes();
int launch_free_footprint(tsd_ctx* ctx, unsigned minX, unsigned maxX, unsigned minY, unsigned maxY);
int launch_neg_scan(tsd_ctx* ctx);
int launch_export_tiles(tsd_ctx* ctx, int t0, int n, double* d_t, double* d_w);
int launch_import_tiles(tsd_ctx* ctx, int t0, int n, const double* d_t, const double* d_w);
int launch_grid_digest(tsd_ctx* ctx, unsigned long long* d_out, double* d_sums);
// halo: the push right ahead of this launch left its halo pass to it.  done: an event that completes with the ray cast itself (the
// launch's own stop event: no marker behind it; a timed dispatch needs its stop event for the timer and records `done` behind it)
int launch_raycast(tsd_ctx* ctx, const LaunchTarget& tg, const RaycastArgs& a, const RaycastArgs* a_dev, const double* d_rays,
                   const HaloArgs* halo = nullptr, hipEvent_t done = nullptr);
// ---- the registration (icp_kernels.hip; the workgroup shape of every launch: icp_shape.hpp)
// pre: fused registration_mode 3 -- the pre-registration's arg-max rides as the first workgroup of the registration's launch (k_icp_pre;
// only where icp_pre_supported() says so); pre->done is recorded when the launch has completed
bool icp_pre_supported(const tsd_ctx* ctx, const IcpArgs& a);
int launch_icp(tsd_ctx* ctx, const LaunchTarget& tg, const IcpArgs& a, const double* P_dev, const double* d_rays_local,
               const double* d_ranges, const uint8_t* d_mask, const ScanPostArgs* post = nullptr, const IcpPreLaunch* pre = nullptr);
int launch_icp_pairs(tsd_ctx* ctx, const IcpArgs& a, int* d_pairs);
int icp_pairs_cap(int n_model, int n_scene);
// the registrations of a batch in one launch on `stream`; the entry array lives in device memory, `host` is the host copy it was staged
// from, its seed arguments filled with icp_batch_seed_args() (`batch_beams`: the widest sensor's)
int launch_icp_batch(tsd_ctx* ctx, hipStream_t stream, const IcpBatchEntry* host, const IcpBatchEntry* d_entries, int n);
IcpSeedArgs icp_batch_seed_args(const tsd_ctx* ctx, void* buf, int beams, int batch_beams);
size_t icp_seed_bytes(int points);

int launch_scan_prepare(tsd_ctx* ctx, SensorDev* st);
// one wave on the context's stream that waits (on the device, bounded) until *seq == value; when the bound runs out it switches
// the push behind it off (push->enabled = 0) and raises *err_host (coherent host memory) instead of letting stale arguments through
int launch_wait_seq(tsd_ctx* ctx, const unsigned long long* seq, unsigned long long value, PushArgs* push, unsigned int* err_host,
                    unsigned int poll_bound);
// one wave on `stream` that publishes *flag = value (device scope) once everything ahead of it on the stream is done
int launch_set_flag(tsd_ctx* ctx, hipStream_t stream, unsigned int* flag, unsigned int value);
int launch_stall(tsd_ctx* ctx, hipStream_t stream, unsigned int us);
// start-up probe of tsd_batch_create: can a kernel on stream `a` wait for a flag that a kernel launched AFTER it on stream `b`
// sets?  (No when the two streams share an in-order hardware queue, or when something serialises dispatches.)
int probe_cross_stream_wait(tsd_ctx* ctx, hipStream_t a, hipStream_t b, unsigned int* d_flag2, bool* ok);
// batched launches on `stream`; the entry arrays live in device memory, `host` is the host copy they were staged from
int launch_raycast_batch(tsd_ctx* ctx, hipStream_t stream, const RaycastBatchEntry* d_entries, int n, int max_beams);
int launch_raycast_batch_byval(tsd_ctx* ctx, hipStream_t stream, const RaycastBatchEntry* h_entries, int n, int max_beams);   // n <= RC_BATCH_BYVAL
int launch_push_tables_batch(tsd_ctx* ctx, hipStream_t stream, const TablesBatchEntry* d_entries, int n, int max_beams);
int push_multi_max_robots();
int launch_push_multi(tsd_ctx* ctx, hipStream_t stream, int n, const PushJob* jobs);
int launch_wait_seq_multi(tsd_ctx* ctx, int n, const unsigned long long* const* seq, const unsigned long long* value, PushArgs* const* push,
                          unsigned int* err_host, unsigned int poll_bound);

void reloc_free(tsd_ctx* ctx);               // reloc.hip: releases tsd_ctx::reloc (tsd_destroy)
void surface_free(tsd_ctx* ctx);             // surface.hip: releases tsd_ctx::surface (tsd_destroy)
void align_free(tsd_ctx* ctx);               // align.hip: releases tsd_ctx::align (tsd_destroy)
void clearance_free(tsd_ctx* ctx);           // clearance.hip: releases tsd_ctx::clearance (tsd_destroy)
void frontier_free(tsd_ctx* ctx);            // frontier.hip: releases tsd_ctx::frontier (tsd_destroy)
void route_free(tsd_ctx* ctx);               // route.hip: releases tsd_ctx::route and ::fields (tsd_destroy)
// route.hip: k_route_trace enqueued on the route result's stream, not waited for; where it leaves the goal cells, the lengths and the
// paths ([g * max_len + j], goal first) in tsd_ctx::route's scratch
const char* route_goal_layers_wrong(const tsd_ctx::Route& r, const uint8_t* goal_layers, int n_goals);   // nullptr, or why they are refused
struct RouteTrace { const uint32_t* d_goals; const int32_t* d_len; const uint32_t* d_paths; const uint8_t* d_layers; };
int route_trace_enqueue(tsd_ctx* ctx, tsd_ctx::Route& r, const uint32_t* goal_cells, const uint8_t* goal_layers, int n_goals, int max_len,
                        RouteTrace* out);
void drive_free(tsd_ctx* ctx);               // drive.hip: releases tsd_ctx::drive (tsd_destroy)
void view_free(tsd_ctx* ctx);                // view.hip: releases tsd_ctx::view (tsd_destroy)
int8_t* frame_staged_map(const tsd_ctx* ctx);   // map_publish.hip: the frame staging's map (cells * cells int8), nullptr without a staging
int launch_calibrate(tsd_ctx* ctx, double* t, double* w, size_t n);
int launch_occupancy(tsd_ctx* ctx, int8_t* d_out, int inflate, int inflate_factor);
size_t occ_heads_bytes();
// the list heads of the next extraction (cur) and the set it clears for the one after (next)
struct OccHeads { unsigned int* cur; unsigned int* next; };
OccHeads next_occ_heads(tsd_ctx* ctx);
int launch_occ_mark(tsd_ctx* ctx, int8_t* d_out, int* d_count, int inflate, int inflate_factor, const unsigned int* heads, int max_tiles = -1);
int launch_color_image(tsd_ctx* ctx, const double* d_px, const double* d_py, unsigned width, unsigned height, uint8_t* d_image);

// pose helpers (host): textbook LU inverse with partial pivoting in the order of
// gsl_linalg_LU_decomp / LU_invert as used by obvious::Matrix::invert (gsl/Matrix.cpp:168-179)
void mat3_inv(const double A[9], double Ainv[9]);

}  // namespace tsd
