"""resize_crop_u8's host math under AddressSanitizer + UndefinedBehaviorSanitizer:
csrc/tests/resize_checks.cpp drives csrc/resize_math.h (Pillow's fixed-point
coefficient tables, the band -> input-row ranges, the LDS plan, the staging
slots of an unaligned row) for the tested geometries, a 1 x N strip, upscales
and supports large enough to force the chunked form.  A stand-alone host
program, built and run as tests/test_grouped_checks.py builds grouped_checks.cpp;
no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "-distributed-machine-learning-system_amd", "csrc", "tests", "resize_checks.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_resize_host_math_under_asan_ubsan(tmp_path):
    exe = tmp_path / "resize_checks"
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", SRC, "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
