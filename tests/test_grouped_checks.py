"""The grouped 3x3 conv's index math under AddressSanitizer +
UndefinedBehaviorSanitizer: csrc/tests/grouped_checks.cpp drives the
__host__ __device__ functions of csrc/grouped_math.h the way
conv3x3_grouped.hip does (channel-block-to-K-slot map for every group size and
C up to 2048, halo / border geometry of both strides for H, W = 1 .. 20).
A stand-alone host program, built and run as tests/test_host_checks.py builds
host_checks.cpp; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "-distributed-machine-learning-system_amd", "csrc", "tests", "grouped_checks.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_grouped_index_math_under_asan_ubsan(tmp_path):
    exe = tmp_path / "grouped_checks"
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", SRC, "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
