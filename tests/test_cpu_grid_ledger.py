"""The grid's write ledger on the CPU, under sanitizers (csrc/grid_ledger.hpp).

tests/grid_ledger_check.cpp includes nothing but the ledger's header -- plain host arithmetic, no HIP -- and walks it through tables of
calls whose expected launch windows, frame boxes, windowed / full decisions and epoch moves are written out by hand.  Built with
-fsanitize=address,undefined and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fresh_ledger", "windows_of_three_pushes", "footprint_widens_the_next_window_once",
         "frame_box_is_everything_since_the_last_enqueued_frame", "frame_box_survives_a_lost_frame", "wholesale_rewrites",
         "fallbacks_return_the_whole_map", "image_switched_on_after_map_only_frames", "epoch_rows"]


def test_grid_ledger_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join(str(tmp_path), "grid_ledger_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-misleading-indentation",
                        "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "grid_ledger_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    for c in CASES:
        assert f"ok {c}" in r.stdout, out[-2000:]
    assert "grid_ledger: all cases ok" in r.stdout
