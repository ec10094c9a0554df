"""A context's frontier scratch serves one call at a time (include/tsd_hip.h), and two of the facade's workers meet on member 0's
context: its own ThreadGrid (publish_frontiers, ThreadGrid::frontiers) and a ThreadGridGroup that labels its merged map there.
tests/frontier_lock.cpp drives the facade's own sources (csrc/host) against tests/stub_tsd_hip.c and stand-ins for the calls of the two
workers, which count every overlap of two frontier calls on one context and every fetch of a result another thread replaced; three
threads run the three paths against each other.  Built with -fsanitize=thread, so a missing lock order shows as well."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ohm_tsd_slam_amd", "csrc", "host")


def _no_aslr():
    """one process without address-space randomisation where setarch offers it (GCC 11's ThreadSanitizer needs it on kernels with
    32 bits of mmap randomisation), else nothing"""
    s = shutil.which("setarch")
    if s and subprocess.run([s, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        return [s, platform.machine(), "-R"]
    return []


def test_frontier_calls_on_one_context_exclude_each_other(tmp_path):
    if not (shutil.which("g++") and shutil.which("gcc")):
        pytest.skip("no host compiler")
    common = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=thread"]
    stub = str(tmp_path / "stub.o")
    subprocess.run(["gcc", "-c", *common, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stub_tsd_hip.c"), "-o", stub],
                   check=True, capture_output=True, text=True)
    exe = str(tmp_path / "frontier_lock")
    srcs = [os.path.join(ROOT, "tests", "frontier_lock.cpp")] + [os.path.join(HOST, f) for f in
                                                                 ("obvision/obvious.cpp", "ThreadSLAM.cpp", "ThreadGrid.cpp", "ThreadGridGroup.cpp")]
    r = subprocess.run(["g++", "-std=c++17", *common, "-pthread", "-DOHM_TSD_SLAM_NO_ROS", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tests"), *srcs, stub, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66 second_deadlock_stack=1")
    r = subprocess.run(_no_aslr() + [exe], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ok" in r.stdout and "WARNING: ThreadSanitizer" not in out, out[-3000:]
