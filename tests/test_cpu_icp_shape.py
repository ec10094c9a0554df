"""The registration's launch decision on the CPU, under sanitizers (csrc/icp_shape.hpp).

tests/icp_shape_check.cpp includes nothing but that header -- plain host arithmetic, no HIP -- and walks icp_shape_for, icp_helpers and
icp_with_shape through rows written out by hand: which kernel instantiation, how many threads, which capacity, how many helper
workgroups and which error a point count gets.  The LDS bytes, the halves of the slot array and the shapes that do not fit 160 KiB
come from tests/golden/icp_shapes.txt, recorded from the arithmetic before it moved into the header.  Built with
-fsanitize=address,undefined and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fused_closed_form", "fused_point_to_line", "forced_shapes", "direct_mode", "batch", "helpers_limit"]


def test_icp_shape_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join(str(tmp_path), "icp_shape_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "icp_shape_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "icp_shapes.txt")], env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    print(r.stdout)
    assert "Sanitizer" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    for c in CASES:
        assert f"ok {c}" in r.stdout, out[-2000:]
    assert "icp_shape: all cases ok" in r.stdout
