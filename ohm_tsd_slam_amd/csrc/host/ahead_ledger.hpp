// ahead_ledger.hpp -- what a localiser remembers about the work it did AHEAD of the next scan on the fused path: whether the next scan
// is staged on the device already (_sensor holds it, tsd_scan_stage took it) and which scan that is, whether that scan's
// registration_mode-3 pre-registration is armed there too (tsd_scan_preregister ahead of the collect), and whether the three rand()
// streams taken ahead are still unused.  The NEXT scan's streams are drawn while the device registers this one: 1 311 rand() calls are
// 23 us of host time -- more than the host has between two scans before the device runs dry.  The draws do not depend on the scan, so a
// staged scan that is dropped takes its armed pre-registration along but not its draws: the scan that came instead is armed with the
// very same ones, and a seeded sequence (tsdpdf_seed) stays one drawStreams() call per REGISTERED scan, as on the unfused path.
// Plain host logic: no ROS, no device ABI.  ThreadLocalize keeps the draw vectors and makes every call; the ledger never calls out.
// Every operation is named after what happened and returns what the caller has to do; nothing else writes these fields.
// tests/ahead_ledger_check.cpp runs it on the CPU.
// Who may call: the thread that runs ThreadLocalize::processScan, and ThreadLocalize::startAt while the localiser is idle().
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace ohm_tsd_slam
{

class AheadLedger
{
public:
  // A scan came.  true = it IS the staged one: same stamp, same size AND the same readings (drivers that leave the stamp at 0 or
  // repeat it must not get the previously staged ranges registered in place of the scan they delivered) -- the caller leaves _sensor
  // as it is.  Anything else un-stages the staged scan (tsd_scan_submit drops it) and the caller ingests the readings.  An armed
  // pre-registration is remembered until enter_fused looks at it.
  bool arrived(long long stampNs, const float* ranges, size_t n)
  {
    staged_ = staged_ && stamp_ns_ == stampNs && ranges_.size() == n && (n == 0 || std::memcmp(ranges_.data(), ranges, n * sizeof(float)) == 0);
    return staged_;
  }

  // The scan that came goes down the fused path.  useStaged: submit the staged scan; preStaged: its pre-registration is armed, the
  // caller does not arm.  Single robot: both are used up by this call, and an armed pre-registration whose scan was not accepted
  // gives its draws back (they count as ready again).  Several robots on one grid (concurrent): nothing is staged ahead there, so
  // nothing is used and nothing changes.
  struct Entry { bool useStaged, preStaged; };
  Entry enter_fused(bool concurrent)
  {
    if(concurrent) return Entry{false, false};
    const Entry e{staged_, staged_ && armed_};
    if(armed_ && !staged_) draws_ready_ = true;
    staged_ = armed_ = false;
    return e;
  }

  // A pre-registration of n beams is being armed.  true = drawStreams first: the caller does not want the draws taken ahead (a batch's
  // scan: fresh draws every time), or there are none, or they are of another size (drawsSize: the sub-sampling stream's).  The draws
  // are spent either way.
  bool arm(bool reuseDraws, size_t n, size_t drawsSize)
  {
    const bool draw = !reuseDraws || !draws_ready_ || drawsSize != n;
    draws_ready_ = false;
    return draw;
  }

  // The scan is submitted and the staging attempt is over; the device is busy.  true = take the NEXT scan's draws now, and they are
  // ready from here on.  Not where the staged scan was armed (that spent fresh ones), where draws are still ready, outside
  // registration_mode 3 and after capacity_refused.
  bool submitted_needs_draws(bool mode3)
  {
    if(!mode3 || !pre_fused_ok_ || draws_ready_ || armed_) return false;
    draws_ready_ = true;
    return true;
  }

  // tsd_scan_stage took the next scan: this stamp, these readings (in the sensor's beam order) ...
  void staged(long long stampNs, const float* ranges, size_t n)
  {
    staged_ = true;
    stamp_ns_ = stampNs;
    ranges_.assign(ranges, ranges + n);
  }
  // ... and tsd_scan_preregister armed its pre-registration
  void staged_and_armed() { armed_ = true; }

  // startAt re-seated a running localiser: the staged scan and its arming are forgotten.  Unlike a drop, the draws an armed scan spent
  // are NOT given back: a re-seat with an armed scan advances a seeded sequence by one extra drawStreams() call.
  void reseated() { staged_ = armed_ = false; }

  // TSD_E_CAPACITY from the arming (more trials / control points than the device-side list building holds): registration_mode 3 keeps
  // the unfused call structure from this scan on
  void capacity_refused() { pre_fused_ok_ = false; }
  bool pre_fused_ok() const { return pre_fused_ok_; }

private:
  bool staged_ = false;            // _sensor holds, and the device has staged, the scan with ...
  long long stamp_ns_ = 0;         // ... this stamp ...
  std::vector<float> ranges_;      // ... and these readings
  bool armed_ = false;             // the staged scan's pre-registration is armed on the device already
  bool draws_ready_ = false;       // the caller's three streams were drawn ahead and not used yet
  bool pre_fused_ok_ = true;
};

} /* namespace ohm_tsd_slam */
