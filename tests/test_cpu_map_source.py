"""The map products' rule on the CPU, under sanitizers (csrc/map_source_rule.hpp).

tests/map_source_check.cpp includes nothing but the rule's header -- plain host logic, no HIP -- and puts it through every combination
of what it reads: the frame's flags, sides at and above the limit, the cost map's states, a caller's sides and strides, a fetch's
ranges up to INT_MAX, the seed list.  What each must return is written out by hand there.  Built with -fsanitize=address,undefined
and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["frame_map_wrong", "caller_map_wrong", "fetch_range_wrong", "map_seeds"]


def test_map_source_rule_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join(str(tmp_path), "map_source_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-I" + os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "map_source_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    for c in CASES:
        assert f"ok {c}" in r.stdout, out[-2000:]
    assert "map_source: all cases ok" in r.stdout
