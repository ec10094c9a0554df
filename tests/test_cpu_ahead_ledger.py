"""A localiser's look-ahead bookkeeping on the CPU, under sanitizers (csrc/host/ahead_ledger.hpp; DESIGN, the facade).

tests/ahead_ledger_check.cpp includes nothing but the ledger's header -- plain host logic, no ROS shim, no device ABI -- and walks it
through the ledger calls of ThreadLocalize's fused path, in that path's order: when a scan that came is the staged one, what a dropped
staged scan takes along (its arming) and what it leaves (its draws), which drawStreams() call's draws an arming carries, what a
concurrent entry and a re-seat leave alone.  The expectations are written out by hand.  Built with -fsanitize=address,undefined and
run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fresh_state", "staged_and_accepted", "staged_and_dropped", "empty_readings_with_the_same_stamp", "armed_ahead_and_accepted",
         "armed_ahead_and_dropped", "draws_taken_ahead_with_nothing_staged", "a_draws_vector_of_another_size",
         "submitted_needs_draws_in_all_four_combinations", "concurrent_entry", "reseated_with_an_armed_scan", "capacity_refused_sticks"]


def test_ahead_ledger_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join(str(tmp_path), "ahead_ledger_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc", "host"),
                        os.path.join(ROOT, "tests", "ahead_ledger_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    for c in CASES:
        assert f"ok {c}" in r.stdout, out[-2000:]
    assert "ahead_ledger: all cases ok" in r.stdout
