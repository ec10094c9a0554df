// scan_ledger_check.cpp -- tsd::ScanLedger and tsd::PreLedger (csrc/scan_ledger.hpp) on the CPU.  The helpers below make the ledger
// calls of the entry points in the entry points' order (tsd_scan_stage / _submit / _collect, tsd_scan_preregister) and note what the
// entry point would have to do; what each row expects is written out by hand from DESIGN 1 and the header's rules (three buffers in
// turn, once per submitted scan; which event stands between a buffer and its next writer; staged / submitted / in flight; when the
// ray cast ahead stands; how a pre-registration is armed).  Built and run by tests/test_cpu_scan_ledger.py under
// -fsanitize=address,undefined.  Prints "ok <case>" per case, "scan_ledger: all cases ok" at the end.
#include "scan_ledger.hpp"

#include <cstdio>

using tsd::PreLedger;
using tsd::ScanLedger;

static int bad = 0;          // failed expectations of the case being run
#define EXPECT(cond) do { if (!(cond)) { std::printf("  line %d: expected %s\n", __LINE__, #cond); bad++; } } while (0)

// One sensor as the fused path drives it.  `epoch` stands for the grid ledger's: every push moves it.
struct Sensor {
  ScanLedger l;
  bool bar = false;          // the host writes the device buffers itself
  bool async = false;        // asynchronous mapping
  bool host_sees_push = false;   // scan_stage_device's shortcut: the host finds a buffer's push event complete
  unsigned long long epoch = 0;
  // what the last call had to do
  int slot = -1;
  bool wait_copy = false, wait_push = false, side_wait = false, tables_seen = false, cast = false, from_host = false;

  void host_half()           // scan_stage_host
  {
    const ScanLedger::HostWrite w = l.host_write(bar);
    slot = w.slot; wait_copy = w.wait_copy; wait_push = w.wait_push;
  }
  void device_half()         // scan_stage_device
  {
    side_wait = false;
    if (l.side_write(l.slot())) { if (host_sees_push) l.push_seen_done(l.slot()); else side_wait = true; }
    if (!bar) l.copy_recorded(l.slot());
    l.device_staged();
  }
  bool stage()               // tsd_scan_stage
  {
    if (!l.may_stage()) return false;
    host_half(); device_half();
    return true;
  }
  ScanLedger::Submit submit(bool have_scan)      // tsd_scan_submit
  {
    const ScanLedger::Submit may = l.may_submit(have_scan);
    if (may != ScanLedger::Submit::ok) return may;
    tables_seen = false;
    if (have_scan) {
      if (!l.may_stage()) tables_seen = l.drop_staged(bar).need_tables_seen;
      host_half();
    }
    from_host = l.scan_from_host();
    cast = !l.raycast_stands(epoch);
    l.submit();
    slot = l.slot();
    if (from_host) device_half();
    epoch++;                                     // the push
    if (async) l.push_recorded(l.slot());
    l.raycast_ahead(epoch);
    l.enqueued();
    return may;
  }
  bool collect()             // tsd_scan_collect
  {
    if (!l.collect_due()) return false;
    l.collect();
    return true;
  }
  bool scan(bool have_scan = true) { return submit(have_scan) == ScanLedger::Submit::ok && collect(); }
};

static void fresh_state()
{
  ScanLedger l;
  EXPECT(l.may_stage());
  EXPECT(l.may_submit(false) == ScanLedger::Submit::no_scan);
  EXPECT(l.may_submit(true) == ScanLedger::Submit::ok);
  EXPECT(!l.collect_due() && !l.split_in_flight() && !l.in_flight());
  EXPECT(l.scan_from_host());
  EXPECT(!l.raycast_stands(0));
  EXPECT(l.slot() == 0);
  for (int b = 0; b < ScanLedger::kBuffers; b++) EXPECT(!l.side_write(b));
  PreLedger p;
  EXPECT(!p.take());
  EXPECT(!p.result_readable(false));
  EXPECT(p.inputs_ready() == PreLedger::Inputs::copy_now);
}

static void four_scans_use_slots_0_1_2_0()
{
  for (int bar = 0; bar < 2; bar++) {
    Sensor s; s.bar = bar != 0;
    const int want[4] = {0, 1, 2, 0};
    for (int k = 0; k < 4; k++) {
      EXPECT(s.scan());
      EXPECT(s.slot == want[k]);
      EXPECT(s.from_host);                       // a scan that came with the submit: its registration reads what the host wrote
      EXPECT(!s.wait_push && !s.side_wait);      // strict order: no push event anywhere
      EXPECT(s.cast == (k == 0));                // every scan but the first finds its ray cast enqueued ahead
      if (bar) EXPECT(!s.wait_copy);             // no pinned copy at all
    }
  }
}

static void pinned_copy_is_asked_for_once()
{
  Sensor s;                                      // pinned buffers
  const bool want[4] = {false, false, false, true};
  for (int k = 0; k < 4; k++) { EXPECT(s.scan()); EXPECT(s.wait_copy == want[k]); EXPECT(s.slot == (k % 3)); }
  // the fourth scan's own copy out of buffer 0 is recorded again; seen once, a host write with no copy in between asks no more
  ScanLedger l;
  l.host_write(false); l.copy_recorded(0); l.device_staged();
  l.drop_staged(false);
  ScanLedger::HostWrite w = l.host_write(false);
  EXPECT(w.slot == 0 && w.wait_copy);
  l.drop_staged(false);
  w = l.host_write(false);
  EXPECT(w.slot == 0 && !w.wait_copy);
}

static void pushes_are_recorded_per_slot_under_asynchronous_mapping()
{
  {                                              // the host writes the device buffers: it has to see the buffer's push done itself
    Sensor s; s.bar = true; s.async = true;
    for (int k = 0; k < 3; k++) { EXPECT(s.scan()); EXPECT(s.slot == k && !s.wait_push && !s.side_wait); }
    for (int k = 3; k < 7; k++) {
      EXPECT(s.scan());
      EXPECT(s.slot == k % 3 && s.wait_push);    // the push of scan k-3, which read this buffer
      EXPECT(!s.side_wait);                      // ... and the side stream needs no wait of its own after that
      EXPECT(!s.wait_copy);
    }
  }
  {                                              // pinned buffers: the host write does not ask, the side stream's write does
    Sensor s; s.async = true;
    for (int k = 0; k < 3; k++) { EXPECT(s.scan()); EXPECT(!s.wait_push && !s.side_wait); }
    EXPECT(s.scan());
    EXPECT(s.slot == 0 && !s.wait_push && s.wait_copy && s.side_wait);
    // the host saw nothing complete: buffer 1's push is still outstanding for the next scan, and the host's shortcut settles it
    EXPECT(s.l.side_write(1));
    s.host_sees_push = true;
    EXPECT(s.scan());
    EXPECT(s.slot == 1 && !s.wait_push && !s.side_wait);
    // (scan 4's own push is recorded on buffer 1 again)
    EXPECT(s.l.side_write(1));
    s.l.push_seen_done(1);
    EXPECT(!s.l.side_write(1));
    EXPECT(s.l.side_write(2) && s.l.side_write(0));      // per buffer: scan 2's and scan 3's pushes
  }
  {                                              // strict order records none
    Sensor s; s.bar = true;
    for (int k = 0; k < 6; k++) { EXPECT(s.scan()); EXPECT(!s.wait_push && !s.side_wait); }
  }
  {                                              // switched off again: what was recorded is still looked at, nothing new is recorded
    Sensor s; s.bar = true; s.async = true;
    for (int k = 0; k < 3; k++) EXPECT(s.scan());
    s.async = false; s.l.raycast_void();         // tsd_sensor_set_async_mapping(0)
    for (int k = 3; k < 6; k++) { EXPECT(s.scan()); EXPECT(s.wait_push); }
    for (int k = 6; k < 9; k++) { EXPECT(s.scan()); EXPECT(!s.wait_push); }
  }
}

static void a_scan_staged_ahead_is_submitted_from_its_slot()
{
  for (int bar = 0; bar < 2; bar++) {
    Sensor s; s.bar = bar != 0;
    EXPECT(s.scan());                            // slot 0
    EXPECT(s.stage());
    EXPECT(s.slot == 1);
    EXPECT(!s.l.may_stage());
    EXPECT(s.submit(false) == ScanLedger::Submit::ok);
    EXPECT(s.slot == 1 && !s.from_host && !s.tables_seen);     // copy and tables went out with the stage
    EXPECT(s.l.may_stage());
    EXPECT(s.collect());
    EXPECT(s.scan());
    EXPECT(s.slot == 2);                         // the rotation advanced once for the staged scan
    EXPECT(s.from_host);
  }
}

static void a_decoy_staged_and_dropped_after_every_scan()
{
  for (int bar = 0; bar < 2; bar++) {
    Sensor s; s.bar = bar != 0; s.async = true;
    for (int k = 0; k < 6; k++) {
      EXPECT(s.scan());                          // the real scan: drops the decoy staged after the previous one
      EXPECT(s.slot == k % 3);
      EXPECT(s.from_host);                       // the dropped scan's device half does not count for the new one
      EXPECT(s.tables_seen == (bar && k > 0));   // host-written buffer + the decoy's tables were enqueued
      EXPECT(s.stage());                         // the decoy
      EXPECT(s.slot == (k + 1) % 3);
    }
  }
  // a dropped scan whose device half was never enqueued: nothing on the device reads the buffer
  ScanLedger l;
  l.host_write(true);
  EXPECT(!l.drop_staged(true).need_tables_seen);
  EXPECT(l.may_stage());
  EXPECT(l.host_write(true).slot == 0);
  l.device_staged();
  EXPECT(l.drop_staged(true).need_tables_seen);
  EXPECT(l.host_write(true).slot == 0);
  l.device_staged();
  EXPECT(!l.drop_staged(false).need_tables_seen);
}

static void refusals()
{
  Sensor s;
  EXPECT(!s.collect());                                                  // collect without a submit
  EXPECT(s.submit(false) == ScanLedger::Submit::no_scan);                // nothing given, nothing staged
  EXPECT(s.l.slot() == 0 && s.l.may_stage() && !s.l.in_flight());        // ... and nothing moved
  EXPECT(s.stage());
  EXPECT(!s.stage());                                                    // staging twice
  EXPECT(s.slot == 0);
  EXPECT(s.submit(false) == ScanLedger::Submit::ok);
  EXPECT(s.submit(true) == ScanLedger::Submit::not_collected);           // submitting twice, with ...
  EXPECT(s.submit(false) == ScanLedger::Submit::not_collected);          // ... and without a scan
  EXPECT(s.stage());                                                     // (staging ahead of the collect is the point of staging)
  EXPECT(s.slot == 1);
  EXPECT(s.collect());
  EXPECT(!s.collect());
}

static void the_ray_cast_ahead()
{
  Sensor s; s.bar = true;
  EXPECT(s.scan());
  EXPECT(s.cast);                                // the first scan casts itself
  EXPECT(s.epoch == 1);
  EXPECT(s.l.raycast_stands(1));
  EXPECT(!s.l.raycast_stands(2) && !s.l.raycast_stands(0));      // only at the same epoch
  EXPECT(s.scan());
  EXPECT(!s.cast);
  s.epoch++;                                     // something wrote the grid (tsd_push, a footprint, another sensor's scan ..)
  EXPECT(s.scan());
  EXPECT(s.cast);
  // consumed by a submit: between ScanLedger::submit and the next raycast_ahead nothing stands
  ScanLedger l;
  l.raycast_ahead(7);
  EXPECT(l.raycast_stands(7));
  l.host_write(true);
  l.submit();
  EXPECT(!l.raycast_stands(7));
  l.raycast_ahead(8); l.enqueued();
  EXPECT(l.raycast_stands(8));
  l.raycast_void();                              // tsd_sensor_set_async_mapping
  EXPECT(!l.raycast_stands(8));
  l.raycast_ahead(8);
  l.collect();
  l.split_begin();                               // tsd_scan_begin, and every sensor of a tsd_batch_begin
  EXPECT(!l.raycast_stands(8));
  l.split_end();
  EXPECT(!l.raycast_stands(8));
}

static void in_flight()
{
  Sensor s;
  EXPECT(s.submit(true) == ScanLedger::Submit::ok);
  EXPECT(s.l.in_flight() && s.l.collect_due() && !s.l.split_in_flight());
  EXPECT(s.collect());
  EXPECT(!s.l.in_flight());
  s.l.split_begin();                             // a split scan, or a batched one
  EXPECT(s.l.in_flight() && s.l.split_in_flight() && !s.l.collect_due());
  s.l.split_end();
  EXPECT(!s.l.in_flight() && !s.l.split_in_flight());
  EXPECT(s.stage());
  EXPECT(!s.l.in_flight());                      // a staged scan is not in flight
}

// ---- PreLedger.  A layout here: total 1000 bytes, inputs 200, header at 800, result at 900.
static void armed_between_scans()
{
  PreLedger p;
  PreLedger::MayArm m = p.may_arm(false, 1000, 200, 0);
  EXPECT(!m.refused && !m.sync_prev_copy);
  EXPECT(p.arm(false, true, false) == PreLedger::Arm::direct);
  EXPECT(p.inputs_ready() == PreLedger::Inputs::ready);
  PreLedger q;
  EXPECT(q.arm(false, false, false) == PreLedger::Arm::side_copy);
  EXPECT(q.inputs_ready() == PreLedger::Inputs::wait_copy_event);
  // between scans a larger layout is fine, whatever ran before
  EXPECT(q.take()); q.launched_single(800, 900);
  m = q.may_arm(false, 5000, 2000, 1000);
  EXPECT(!m.refused && m.sync_prev_copy);
}

static void copy_at_submit()
{
  PreLedger p;
  EXPECT(p.arm(false, true, true) == PreLedger::Arm::at_submit);         // (never direct, even where the host could store)
  EXPECT(p.inputs_ready() == PreLedger::Inputs::copy_now);
  EXPECT(!p.may_arm(false, 1000, 200, 1000).sync_prev_copy);
  EXPECT(p.take());
  p.launched_single(800, 900);
  EXPECT(p.arm(true, true, true) == PreLedger::Arm::refuse_copy_main);   // a scan in flight
  EXPECT(!p.take());                                                     // nothing was armed by the refused call
  PreLedger q;
  EXPECT(q.arm(true, false, true) == PreLedger::Arm::refuse_copy_main);
}

static void armed_ahead_of_a_collect()
{
  for (int visible = 0; visible < 2; visible++) {
    PreLedger p;
    p.arm(false, visible != 0, false);
    EXPECT(p.take());
    p.launched_single(800, 900);                 // the scan in flight ran a pre-registration
    EXPECT(!p.may_arm(true, 1000, 200, 1000).refused);
    EXPECT(p.may_arm(true, 1001, 200, 1000).refused);          // needs new buffers
    EXPECT(p.may_arm(true, 1000, 801, 1000).refused);          // inputs reach into the in-flight header
    EXPECT(!p.may_arm(true, 1000, 800, 1000).refused);         // ... end right in front of it
    EXPECT(p.may_arm(true, 1000, 200, 1000).sync_prev_copy == (visible == 0));
    EXPECT(p.arm(true, visible != 0, false) == PreLedger::Arm::side_copy_behind_done);   // never direct
    EXPECT(p.inputs_ready() == PreLedger::Inputs::wait_copy_event);
  }
  // the in-flight scan ran none: nothing of it in the buffers, nothing to order the copy behind
  PreLedger p;
  EXPECT(!p.take());
  EXPECT(!p.may_arm(true, 1000, 200, 0).refused);
  EXPECT(p.arm(true, true, false) == PreLedger::Arm::side_copy);
}

static void rearmed_without_a_submit()
{
  PreLedger p;
  EXPECT(p.arm(false, false, false) == PreLedger::Arm::side_copy);
  PreLedger::MayArm m = p.may_arm(false, 1000, 200, 1000);
  EXPECT(m.sync_prev_copy && !m.refused);        // nothing the host has seen is ordered behind that copy
  EXPECT(p.arm(false, false, false) == PreLedger::Arm::side_copy);
  EXPECT(p.take());
  EXPECT(!p.take());                             // one submit uses it up, however often it was armed
  PreLedger q;
  EXPECT(q.arm(false, true, false) == PreLedger::Arm::direct);
  EXPECT(!q.may_arm(false, 1000, 200, 1000).sync_prev_copy);     // the host stored it: no copy to see done
  // armed ahead, then re-armed ahead: the first ahead-copy is synchronised, the second still goes behind the done event
  PreLedger r;
  r.arm(false, true, false); EXPECT(r.take()); r.launched_single(800, 900);
  EXPECT(r.arm(true, true, false) == PreLedger::Arm::side_copy_behind_done);
  EXPECT(r.may_arm(true, 1000, 200, 1000).sync_prev_copy);
  EXPECT(r.arm(true, true, false) == PreLedger::Arm::side_copy_behind_done);
}

static void take_in_a_submit_and_in_a_batch()
{
  PreLedger p;
  p.arm(false, true, false);
  EXPECT(p.take());                              // tsd_scan_submit
  p.launched_single(800, 900);
  EXPECT(!p.result_readable(true));              // submitted, not collected
  EXPECT(p.result_readable(false));
  EXPECT(!p.take());                             // the next scan has none
  EXPECT(!p.result_readable(false));
  // a batch of three robots, the middle one not armed (and with a result from its previous scan)
  PreLedger r[3];
  r[1].arm(false, true, false); EXPECT(r[1].take()); r[1].launched_single(800, 900);
  r[0].arm(false, false, false); r[2].arm(false, true, false);
  const bool want[3] = {true, false, true};
  for (int i = 0; i < 3; i++) EXPECT(r[i].take() == want[i]);
  for (int i = 0; i < 3; i++) if (want[i]) r[i].launched_batch(800, 900);
  for (int i = 0; i < 3; i++) EXPECT(r[i].result_readable(false) == want[i]);
}

static void no_done_event_after_a_batched_launch()
{
  PreLedger p;
  p.arm(false, true, false); EXPECT(p.take()); p.launched_single(800, 900);
  EXPECT(p.arm(true, true, false) == PreLedger::Arm::side_copy_behind_done);
  EXPECT(p.take()); p.launched_batch(800, 900);
  EXPECT(p.arm(true, true, false) == PreLedger::Arm::side_copy);
  EXPECT(p.take()); p.launched_single(800, 900);
  EXPECT(p.arm(true, true, false) == PreLedger::Arm::side_copy_behind_done);
}

static void result_offsets_are_the_launch_s()
{
  PreLedger p;
  p.arm(false, true, false); EXPECT(p.take()); p.launched_single(800, 900);
  EXPECT(p.res_off_hdr() == 800 && p.res_off_res() == 900);
  // re-armed ahead of the collect with a smaller layout (header at 640, result at 700): the collected scan's records are where its
  // own launch put them
  EXPECT(!p.may_arm(true, 760, 160, 1000).refused);
  p.arm(true, true, false);
  EXPECT(p.result_readable(false));
  EXPECT(p.res_off_hdr() == 800 && p.res_off_res() == 900);
  EXPECT(p.take()); p.launched_single(640, 700);
  EXPECT(p.res_off_hdr() == 640 && p.res_off_res() == 700);
  // ... and the refusal is measured against them: inputs of 700 bytes would now reach into the header at 640
  EXPECT(p.may_arm(true, 1000, 700, 1000).refused);
  EXPECT(p.take() == false);
  EXPECT(!p.may_arm(true, 1000, 700, 1000).refused);     // the scan in flight has no pre-registration any more
  p.arm(false, true, false); EXPECT(p.take()); p.launched_batch(512, 576);
  EXPECT(p.res_off_hdr() == 512 && p.res_off_res() == 576);
}

static int failures = 0;
static void run(const char* name, void (*f)())
{
  bad = 0;
  f();
  if (bad) { std::printf("FAIL %s\n", name); failures++; }
  else std::printf("ok %s\n", name);
}
#define RUN(f) run(#f, f)

int main()
{
  RUN(fresh_state);
  RUN(four_scans_use_slots_0_1_2_0);
  RUN(pinned_copy_is_asked_for_once);
  RUN(pushes_are_recorded_per_slot_under_asynchronous_mapping);
  RUN(a_scan_staged_ahead_is_submitted_from_its_slot);
  RUN(a_decoy_staged_and_dropped_after_every_scan);
  RUN(refusals);
  RUN(the_ray_cast_ahead);
  RUN(in_flight);
  RUN(armed_between_scans);
  RUN(copy_at_submit);
  RUN(armed_ahead_of_a_collect);
  RUN(rearmed_without_a_submit);
  RUN(take_in_a_submit_and_in_a_batch);
  RUN(no_done_event_after_a_batched_launch);
  RUN(result_offsets_are_the_launch_s);
  if (failures) { std::printf("scan_ledger: %d case(s) FAILED\n", failures); return 1; }
  std::printf("scan_ledger: all cases ok\n");
  return 0;
}
