"""The JPEG entropy decoder's memory safety under host AddressSanitizer +
UndefinedBehaviorSanitizer: csrc/tests/jpeg_checks.cpp (a stand-alone program)
is built together with csrc/runtime/jpeg_entropy.cpp and decodes six small
files, every prefix of each, and each with single bytes replaced.  Host code
only; the program is run directly, with nothing preloaded."""
import os
import shutil
import subprocess

import pytest
from jpeg_cases import encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "-distributed-machine-learning-system_amd", "csrc")
SRCS = [os.path.join(CSRC, "tests", "jpeg_checks.cpp"), os.path.join(CSRC, "runtime", "jpeg_entropy.cpp")]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_jpeg_entropy_decoder_under_asan_ubsan(tmp_path):
    files = [
        encode(38, 30, "420", 50, seed=1),
        encode(54, 22, "422", 95, seed=2),
        encode(17, 9, "444", 75, seed=3),
        encode(70, 46, "420", 75, seed=4, restart_marker_blocks=3),
        encode(24, 24, "444", 75, seed=5, optimize=True),
        encode(33, 19, "grey", 75, seed=6),
    ]
    paths = []
    for i, d in enumerate(files):
        p = tmp_path / f"f{i}.jpg"
        p.write_bytes(d)
        paths.append(str(p))
    exe = tmp_path / "jpeg_checks"
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", *SRCS, "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
    calls = int(r.stdout.split(" decode calls")[0].split()[-1])
    assert calls >= sum(len(d) + len(d) // 7 for d in files)       # every prefix and every 7th byte ran
