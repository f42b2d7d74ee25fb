"""The sub-stream Huffman decode (csrc/jpeg_huff_par.h: one image on many lanes)
and its packer layout against the host decoder, under host AddressSanitizer +
UndefinedBehaviorSanitizer: csrc/tests/jpeg_huff_par_checks.cpp (a stand-alone
program) emulates the kernel's workgroup with virtual threads and decodes eight
small files without restart markers, every prefix of each, and each with every
7th byte replaced by FF, 00 and its value XOR 55, at sub-stream sizes of 32 bits
and the kernel's, with 1, 3 and 64 threads.  Verdicts must agree and
coefficients be identical.  Host code only; the program is run directly, with
nothing preloaded.  Plus the CPU behaviour of ``entropy_on="gpu_parallel"``."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from jpeg_cases import encode, resize_cases
from jpeg_entropy_cases import noise_q100

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "-distributed-machine-learning-system_amd", "csrc")
SRCS = [os.path.join(CSRC, "tests", "jpeg_huff_par_checks.cpp"), os.path.join(CSRC, "runtime", "jpeg_huff_pack.cpp"),
        os.path.join(CSRC, "runtime", "jpeg_entropy.cpp")]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SHARDS = 16


def par_check_files():
    """The eight files of the one-lane core check, the two with restart markers
    replaced by a grey image and a 4:2:2 image with optimised tables."""
    return [
        encode(38, 30, "420", 50, seed=1),
        encode(54, 22, "422", 95, seed=2),
        encode(17, 9, "444", 75, seed=3),
        encode(40, 26, "grey", 90, seed=4),
        encode(24, 24, "444", 75, seed=5, optimize=True),
        encode(33, 19, "grey", 75, seed=6),
        encode(46, 30, "422", 85, seed=7, optimize=True),
        noise_q100(),
    ]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sub_stream_decode_matches_host_decoder_under_asan_ubsan(tmp_path):
    files = par_check_files()
    assert all(b"\xff\xdd" not in d[:d.index(b"\xff\xda")] for d in files)      # no restart interval
    paths = []
    for i, d in enumerate(files):
        p = tmp_path / f"f{i}.jpg"
        p.write_bytes(d)
        paths.append(str(p))
    exe = tmp_path / "jpeg_huff_par_checks"
    cmd = [HIPCC, "--offload-host-only", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", *SRCS, "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    # one pass over every input, spread over SHARDS processes by the program's --shard (the 32-bit
    # sub-streams of the noise file take hundreds of rounds each); the counts of the shards add up
    def shard(i):
        return subprocess.run([str(exe), "--shard", str(i), str(SHARDS), *paths], capture_output=True, text=True,
                              timeout=900, env=env)

    with ThreadPoolExecutor(max_workers=8) as ex:
        runs = list(ex.map(shard, range(SHARDS)))
    tot = {"calls": 0, "ok": 0, "corrupt": 0, "mut_ok": 0, "mut_corrupt": 0, "reached": 0}
    small = seen = cap = 0
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
        assert "0 failure(s)" in r.stdout
        tot["calls"] += int(r.stdout.split(" decode calls")[0].split()[-1])
        tot["ok"] += int(r.stdout.split("both ok ")[1].split(",")[0])
        tot["corrupt"] += int(r.stdout.split("both corrupt in the scan ")[1].split(",")[0])
        m = re.search(r"mutants: both ok (\d+), both corrupt in the scan (\d+)", r.stdout)
        tot["mut_ok"] += int(m.group(1))
        tot["mut_corrupt"] += int(m.group(2))
        m = re.search(r"largest round count at 32 bits (\d+), at (\d+) bits (\d+) \(cap (\d+), reached by (\d+)\)", r.stdout)
        small, seen, cap = max(small, int(m.group(1))), max(seen, int(m.group(3))), int(m.group(4))
        tot["reached"] += int(m.group(5))
    print(tot, f"largest round count at 32 bits {small}, at {m.group(2)} bits {seen}, cap {cap}")
    # every prefix, every 7th byte three ways
    assert tot["calls"] == sum(1 + len(d) + 3 * ((len(d) + 6) // 7) for d in files)
    assert tot["ok"] > len(files) and tot["corrupt"] > 1000           # the comparison saw both outcomes
    assert tot["mut_ok"] > 100 and tot["mut_corrupt"] > 100           # among the mutants too
    assert tot["reached"] == 0 and seen >= 2 and small >= seen        # no input reached the cap at the kernel's size
    assert cap >= 4 * seen                                            # the cap is a safety margin, not a tuning knob


def test_gpu_parallel_is_ignored_on_a_cpu_device():
    from idunno.runtime import jpeg
    from idunno.runtime.data import GpuJpegSource, load_image_u8

    assert jpeg.ENTROPY_ON == ("host", "gpu", "gpu_parallel")
    datas = [d for _, d in resize_cases()[:2]] + [None]
    imgs, info = jpeg.decode_batch(datas, "cpu", entropy_on="gpu_parallel")
    assert info["entropy_on"] == "gpu_parallel" and [r for _, r in info["fallbacks"]] == ["cpu_device"] * 2
    for i, d in enumerate(datas[:2]):
        assert np.array_equal(imgs[i].numpy(), load_image_u8(d))
    assert int(imgs[2].max()) == 0
    host, hinfo = jpeg.decode_batch(datas, "cpu")
    assert hinfo["entropy_on"] == "host" and torch.equal(host, imgs)
    gpu, ginfo = jpeg.decode_batch(datas, "cpu", entropy_on="gpu")
    assert ginfo["entropy_on"] == "gpu" and torch.equal(gpu, imgs)
    assert GpuJpegSource("cpu", root=".", entropy_on="gpu_parallel").entropy_on == "gpu_parallel"
    for bad in ("device", "", "fpga"):
        with pytest.raises(ValueError):
            jpeg.decode_batch(datas, "cpu", entropy_on=bad)


def test_inference_cli_takes_gpu_parallel(monkeypatch):
    from idunno import inference

    seen = []

    def fake(filename, modelname, start, end, **kw):
        seen.append(kw["entropy_on"])
        return [], 0.0

    monkeypatch.setattr(inference, "deeplearning", fake)
    assert inference.main(["alexnet", "0", "0", "--decoder", "gpu", "--entropy", "gpu_parallel"]) == 0
    assert inference.main(["alexnet", "0", "0"]) == 0
    assert seen == ["gpu_parallel", "host"]
    with pytest.raises(SystemExit):
        inference.main(["alexnet", "0", "0", "--entropy", "device"])
    monkeypatch.undo()
    with pytest.raises(ValueError):                 # the real one refuses an unknown form before touching a device
        inference.deeplearning("alexnet", "alexnet", 0, 0, device="cpu", entropy_on="device")
