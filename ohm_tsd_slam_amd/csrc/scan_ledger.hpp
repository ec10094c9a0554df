// scan_ledger.hpp -- what the host remembers about one sensor's scans: which of the three scan / table buffers the next scan goes
// into and what must be seen done before it is rewritten, which scan is staged / submitted / in flight, whether the ray cast enqueued
// ahead still stands (ScanLedger), and how the next scan's pre-registration is armed (PreLedger).  Plain host logic, no HIP: events
// are named by buffer index, the caller keeps the handles and makes the calls.  tests/scan_ledger_check.cpp runs it on the CPU.
// Every operation is named after what happened and returns what the caller has to do; nothing else writes these fields.
// Who may call, under which lock: see tsd_sensor::ledger.
#pragma once
#include <cstddef>

namespace tsd {

class ScanLedger {
 public:
  static constexpr int kBuffers = 3;
  // ---- the fused path's buffer rotation.  A sensor's scan buffers and the range-query tables of a scan's push are used in turn,
  // THREE of them: the scan staged ahead of scan k+2 goes where scan k was, and by then the host has seen the result of scan k+1,
  // whose ray cast ran behind the push of scan k on the stream -- so that push is done without any event on the stream.  That
  // argument needs the STRICT order, and it needs the rotation to advance exactly ONCE PER SCAN (the buffer two rotations back may
  // still be read by the previous scan's push, which is ordered behind nothing the host has seen).  With asynchronous mapping ray
  // cast k+1 runs behind push k-1 and push k beside registration k+1 on the push stream: the host has no proof that it is done, so
  // whoever rewrites a buffer looks at the buffer's own push event first.
  struct HostWrite { int slot; bool wait_copy, wait_push; };
  // The host is about to write the next scan (host_writes_device: straight into the device buffer; else into the pinned one).
  // It synchronises first with the buffer's copy event (the device copy out of the pinned buffer, three scans back) and, where it
  // stores into the device buffer itself, with the event of the push that last read it -- each only if recorded and not yet seen
  // done; both count as seen from here on.  Afterwards this scan is the staged one, its device half (copy, tables) is not enqueued,
  // and the rotation has advanced by one.
  HostWrite host_write(bool host_writes_device)
  {
    const int b = next_;
    next_ = (next_ + 1) % kBuffers;
    const HostWrite w{b, copy_valid_[b], host_writes_device && push_valid_[b]};
    copy_valid_[b] = false;
    if (w.wait_push) push_valid_[b] = false;
    slot_ = b; device_done_ = false; staged_ = true;
    return w;
  }
  // The staged scan is not the one that came: it is dropped and its buffer is handed out again by the next host_write (the rotation
  // advances once per scan that is SUBMITTED).  Where the host writes the device buffer itself and the dropped scan's device half was
  // enqueued, its tables kernel reads that buffer: the host has to see the tables event done first.  (Pinned buffers: the new copy
  // follows the dropped tables on the side stream.)
  struct Dropped { bool need_tables_seen; };
  Dropped drop_staged(bool host_writes_device)
  {
    next_ = slot_; staged_ = false;
    return Dropped{host_writes_device && device_done_};
  }
  // The side stream is about to write buffer `b` (the copy into device memory, the tables): true = behind the event of the push that
  // last read it -- unless the host finds that event complete already, which it reports with push_seen_done
  bool side_write(int b) const { return push_valid_[b]; }
  void push_seen_done(int b) { push_valid_[b] = false; }
  void copy_recorded(int b) { copy_valid_[b] = true; }     // the device copy out of pinned buffer b
  void push_recorded(int b) { push_valid_[b] = true; }     // asynchronous mapping: the push that reads buffer b, on the push stream
  void device_staged() { device_done_ = true; }            // the staged scan's device half is enqueued
  int slot() const { return slot_; }                       // the buffer of the scan staged or submitted last

  // ---- lifecycle of the fused path: nothing -> staged (tsd_scan_stage, or inside tsd_scan_submit) -> submitted -> collected
  bool may_stage() const { return !staged_; }
  enum class Submit { ok, not_collected, no_scan };
  Submit may_submit(bool have_scan) const { return submitted_ ? Submit::not_collected : !have_scan && !staged_ ? Submit::no_scan : Submit::ok; }
  // the registration of the staged scan reads it from where the HOST wrote it: its device half is not enqueued yet
  bool scan_from_host() const { return !device_done_; }
  // tsd_scan_submit takes the staged scan: nothing is staged any more, the ray cast ahead is used up (ask raycast_stands first) ...
  void submit() { staged_ = false; rc_pending_ = false; }
  // ... and everything of it is enqueued: it is in flight until collect().  (A submit that fails in between leaves neither.)
  void enqueued() { submitted_ = true; }
  bool collect_due() const { return submitted_; }
  void collect() { submitted_ = false; }
  // ---- the split and the batched path (tsd_scan_begin .. _finish, tsd_batch_begin .. _results), from the sensor's own thread.  A
  // scan begun there moves the sensor's pose on a stream of its own: a ray cast the fused path enqueued ahead does not stand.
  void split_begin() { split_inflight_ = true; rc_pending_ = false; }
  void split_end() { split_inflight_ = false; }
  bool split_in_flight() const { return split_inflight_; }
  bool in_flight() const { return submitted_ || split_inflight_; }     // on any path

  // ---- the ray cast ahead: a fused scan enqueues the NEXT scan's ray cast behind its own push and remembers the grid ledger's epoch
  // (GridLedger::epoch) as that push left it; the ray cast stands for the next scan only if the epoch is still the same.
  void raycast_ahead(unsigned long long epoch) { rc_pending_ = true; rc_epoch_ = epoch; }
  bool raycast_stands(unsigned long long epoch) const { return rc_pending_ && rc_epoch_ == epoch; }
  // it saw (strict order) or did not see (asynchronous mapping) the previous scan's push: void when the mapping mode changes
  void raycast_void() { rc_pending_ = false; }

 private:
  int next_ = 0, slot_ = 0;
  bool copy_valid_[kBuffers] = {false, false, false};      // recorded and not yet seen complete
  bool push_valid_[kBuffers] = {false, false, false};
  bool staged_ = false, submitted_ = false, device_done_ = false, split_inflight_ = false;
  bool rc_pending_ = false;
  unsigned long long rc_epoch_ = 0;
};

// Fused registration_mode 3: the inputs of the pre-registration that the next submit (or batch) runs are armed by
// tsd_scan_preregister -- between two scans, or AHEAD of the collect of the scan in flight, whose own pre-registration read the same
// device buffer and left its header and result in the pinned one.
class PreLedger {
 public:
  // Arming comes in two steps, because the buffers may have to grow in between.  First, before the host touches the pinned buffer:
  // sync_prev_copy -- the previous side-stream copy out of it has to be SEEN done (it belongs to the in-flight scan, or to a
  // pre-registration armed ahead and now re-armed without a submit); to be done first, refused or not.  refused -- ahead of a
  // collect (inflight) a layout that needs new buffers (total > cur_bytes), or whose inputs would reach into the in-flight scan's
  // header and result records (its arg-max writes them into the pinned buffer at the offsets of ITS layout, and they are read there
  // after the collect), cannot be armed: the caller arms it after the collect.
  struct MayArm { bool refused, sync_prev_copy; };
  MayArm may_arm(bool inflight, size_t total, size_t in_bytes, size_t cur_bytes) const
  {
    return MayArm{inflight && ran_ && (total > cur_bytes || in_bytes > res_off_hdr_), copied_ && !direct_};
  }
  // Then, with the new inputs in the pinned buffer: how they get to the device.
  enum class Arm {
    refuse_copy_main,    // ahead of a collect they can only go by side copy, and that is switched off (nothing is armed by this call;
                         // the pinned buffer was rewritten all the same: the earlier copy no longer counts)
    direct,              // the host stores them into the device buffer itself: nothing to copy, nothing to wait for
    side_copy,           // copied on the side stream now, the copy's event recorded behind it
    side_copy_behind_done,   // ... behind the done event of the in-flight scan's pre-registration, which reads the same buffer
    at_submit            // copied by the launch, on its stream
  };
  // device_host_visible: the device buffer (as it is now) is memory the host can store into -- only ever done between two scans
  Arm arm(bool inflight, bool device_host_visible, bool copy_main)
  {
    copied_ = false; direct_ = false;
    if (device_host_visible && !inflight && !copy_main) { copied_ = direct_ = armed_ = true; return Arm::direct; }
    if (copy_main && inflight) return Arm::refuse_copy_main;
    armed_ = true;
    if (copy_main) return Arm::at_submit;
    copied_ = true;
    return inflight && done_valid_ ? Arm::side_copy_behind_done : Arm::side_copy;
  }
  // ahead of the kernels of an armed pre-registration, on their stream
  enum class Inputs { ready, copy_now, wait_copy_event };
  Inputs inputs_ready() const { return direct_ ? Inputs::ready : !copied_ ? Inputs::copy_now : Inputs::wait_copy_event; }
  // The kernels went out, their header and result go to these offsets of the pinned buffer (the launch's: the layout may be re-armed
  // before they are read).  A single launch has a done event of the sensor's own behind its arg-max, a batched one has none.
  void launched_single(size_t off_hdr, size_t off_res) { done_valid_ = true; res_off_hdr_ = off_hdr; res_off_res_ = off_res; }
  void launched_batch(size_t off_hdr, size_t off_res) { done_valid_ = false; res_off_hdr_ = off_hdr; res_off_res_ = off_res; }
  // A scan of this sensor is being submitted (tsd_scan_submit, tsd_batch_begin): true = with the armed pre-registration, which is
  // used up; that scan then has a pre-registration result, any other scan has none.
  bool take() { ran_ = armed_; armed_ = false; return ran_; }
  bool result_readable(bool collect_due) const { return ran_ && !collect_due; }
  size_t res_off_hdr() const { return res_off_hdr_; }
  size_t res_off_res() const { return res_off_res_; }

 private:
  bool armed_ = false, ran_ = false;
  bool copied_ = false;      // the armed inputs are on their way to the device (side stream) or there (direct_) ...
  bool direct_ = false;      // ... stored by the host
  bool done_valid_ = false;
  size_t res_off_hdr_ = 0, res_off_res_ = 0;
};

}  // namespace tsd
