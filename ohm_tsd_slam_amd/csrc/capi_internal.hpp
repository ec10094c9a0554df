// capi_internal.hpp -- what the three translation units behind include/tsd_hip.h share (capi.hip: context, grid and the unfused
// entry points; capi_io.hip: tile / text / map I/O and profiling; capi_scan.hip: the fused, split and batched scan paths).
#pragma once
#include "tsd_ctx.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

namespace tsd {

extern const char* const kKernelNames[28];         // the kernels tsd_profile_select knows, in profile_mask's bit order
hipEvent_t pool_get(tsd_ctx* ctx);                  // a timing event from the context's pool
char* stage_acquire(tsd_ctx* ctx, int* slot_out);   // next pinned staging slot; waits for the copy that last used it
double distance_filter_multiplier(double maxdist, double mindist, int icp_iterations);
void fill_icp_args(IcpArgs& a, const double pose33[9], const tsd_icp_params* p);
void fill_raycast_args(const tsd_ctx* ctx, RaycastArgs& a, const double pose33[9], int beams, double min_range, double max_range);
void copy_icp_result(const IcpResultDev* h, tsd_icp_result* r);
void fill_stats(tsd_ctx* ctx, const unsigned long long t[7], tsd_push_stats* out);
int read_last_push_stats(tsd_ctx* ctx, tsd_push_stats* out);
int read_total_stats(tsd_ctx* ctx, tsd_push_stats* out, int64_t* pushes, bool reset);
bool host_saw_event(hipEvent_t ev, int us);         // true once `ev` has completed; polls for at most ~`us` microseconds
int wait_for_readers(tsd_ctx* ctx);                 // grid writes on the context's stream go behind the ray casts of the split path
int reset_push_bookkeeping(tsd_ctx* ctx);           // the push's per-tile records, totals and counters as a fresh grid has them (capi.hip)

// The top of an entry point that enqueues on the context's stream: the context's device, and behind a push that asynchronous
// mapping left on the push stream.  `if (int rc = enter(ctx)) return rc;`
inline int enter(tsd_ctx* ctx) { TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device)); return drain_async_push(ctx); }
// The ordered section of an entry point that writes the grid: holds ctx->order_mutex (held = true: the caller holds it already,
// tsd_fuse_begin with several contexts') and has put the context's stream behind the split path's ray casts in flight.
// `WriterScope w(ctx); if (w.rc) return w.rc;`
struct WriterScope {
  std::unique_lock<std::mutex> lk; int rc;
  explicit WriterScope(tsd_ctx* ctx, bool held = false) : lk(ctx->order_mutex, std::defer_lock) { if (!held) lk.lock(); rc = wait_for_readers(ctx); }
};

inline unsigned long long now_ns()
{
  return (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// TSD_CONC_TIMING=1: host time spent inside the scan calls, lap by lap (wall clock, summed over all threads), printed by
// tsd_destroy.  Diagnostic only: unset, a lap is one test of `on` and no clock read.
struct LapTimes {
  std::atomic<unsigned long long> ns[8], max[8], max_at[8];   // per lap: sum, the longest single one and the call it was seen in
  std::atomic<unsigned long long> n;                          // calls
  unsigned long long last_return = 0;                         // (g_scan_timing: when the previous tsd_scan_collect returned)
  bool on;
  LapTimes() : on(getenv("TSD_CONC_TIMING") != nullptr) { for (int i = 0; i < 8; i++) ns[i] = max[i] = max_at[i] = 0; n = 0; }
};
extern LapTimes g_conc_timing;       // the split scan (tsd_scan_begin / _wait / _finish)
extern LapTimes g_scan_timing;       // tsd_scan (one robot): where the host time of a scan goes
extern LapTimes g_stage_timing;      // ... and of the staging of a scan (acquire, host copy, hipMemcpyAsync, records, tables)
struct Lap {
  LapTimes& acc;
  unsigned long long t;
  explicit Lap(LapTimes& a) : acc(a), t(a.on ? now_ns() : 0) {}
  void lap(int i)
  {
    if (!acc.on) return;
    const unsigned long long u = now_ns(), d = u - t;
    acc.ns[i] += d; t = u;
    if (d > acc.max[i]) { acc.max[i] = d; acc.max_at[i] = acc.n.load(); }
  }
};

// What a scan's kernels are given, derived from its sensor (zeroed first: the bytes that reach the device are defined ones).
// sensor_post_args leaves push_copy / publish_done, which are what differs between the scan paths, to the caller; the launch-sizing
// arguments carry what a launcher needs on the host (the rest is read on the device, from the sensor's state).
// sensor_push_job: the push of a scan of `s` that lies in `scan` and whose tables are in `rmq` -- every scan path's.  The host assumes
// the sensor where it last saw it (s->pos); the registration moves it by at most the gate (a larger step is rejected: pose unchanged).
IcpArgs sensor_icp_args(const tsd_sensor* s, const tsd_icp_params* p);
ScanPostArgs sensor_post_args(const tsd_sensor* s, unsigned long long seq, const tsd_gate_params& gates);
PushJob sensor_push_job(const tsd_sensor* s, const ScanView& scan, char* rmq, const tsd_gate_params& gates);
RaycastArgs sensor_raycast_launch_args(const tsd_sensor* s);    // beams: grid size of the launch

}  // namespace tsd
