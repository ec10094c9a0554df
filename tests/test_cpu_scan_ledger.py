"""A sensor's scan slots and pre-registration arming on the CPU, under sanitizers (csrc/scan_ledger.hpp).

tests/scan_ledger_check.cpp includes nothing but the two ledgers' header -- plain host logic, no HIP -- and walks them through the
ledger calls of the scan entry points, in the entry points' order: which buffer a scan goes into, which events are asked for before it
is rewritten, what is refused, when the ray cast ahead stands, how a pre-registration is armed and where its result is read.  The
expectations are written out by hand.  Built with -fsanitize=address,undefined and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fresh_state", "four_scans_use_slots_0_1_2_0", "pinned_copy_is_asked_for_once",
         "pushes_are_recorded_per_slot_under_asynchronous_mapping", "a_scan_staged_ahead_is_submitted_from_its_slot",
         "a_decoy_staged_and_dropped_after_every_scan", "refusals", "the_ray_cast_ahead", "in_flight",
         "armed_between_scans", "copy_at_submit", "armed_ahead_of_a_collect", "rearmed_without_a_submit",
         "take_in_a_submit_and_in_a_batch", "no_done_event_after_a_batched_launch", "result_offsets_are_the_launch_s"]


def test_scan_ledger_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join(str(tmp_path), "scan_ledger_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "scan_ledger_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    for c in CASES:
        assert f"ok {c}" in r.stdout, out[-2000:]
    assert "scan_ledger: all cases ok" in r.stdout
