"""JPEG source throughput: Pillow on Python threads against the native entropy
decoder + HIP kernels.

Generates N (default 2000) Pillow-encoded 500x375 images (4:2:0, quality 90,
seeded) in a temporary directory and, in one process, after a warm-up,
alternating three times, reports images/s of

  * ``JpegSource.get``     8 workers (decode + resize in Pillow, one copy to HBM),
  * ``GpuJpegSource.get``  cold, 8 entropy threads (nothing resident),
  * ``GpuJpegSource.get``  warm (everything resident),

and the cold path's split into entropy decode (host wall time), H2D and the two
kernels (device events).  Then the entropy stage on the host against the
opt-in stage on the device (``entropy_on="gpu"``), cold passes alternating in
the same process: host threads ``--threads`` and 2 (one rank's share when 8
ranks split 16 CPUs), device form at each ``--gpu-chunks`` size; per pass
images/s, entropy time, H2D bytes and time, and host CPU seconds
(``time.process_time``: all threads of the process).  The sub-stream device
form (``entropy_on="gpu_parallel"``, one workgroup per image) runs the same
full passes at each ``--par-chunks`` size, and all four forms (host at
``--threads`` and at 2, ``gpu``, ``gpu_parallel``) answer a small cold query of
each ``--queries`` size (default 64 and 400 images: nothing resident, a fresh
source per query), alternating in that same process after a warm-up of every
form.  The synchronisation rounds the sub-stream kernel needs on these files are
found on the host with the same code (``ops.jpeg_huff_par_rounds``).  Needs a
GPU: without one it exits with an error.

``--progressive`` measures the progressive files instead and nothing else: the
same images encoded with ``progressive=True``, cold ``GpuJpegSource.get`` passes
with ``progressive="fallback"`` (every file through Pillow in ``decode_batch``'s
serial loop) against ``"native"``, for ``entropy_on="host"`` at ``--threads``,
``"gpu"`` and ``"gpu_parallel"``: six arms alternating in one process, ``--reps``
repetitions after a warm-up of every arm, then the cold query of each
``--queries`` size for the same six arms.

``--restart ROWS`` measures restart-interval files instead and nothing else: the
same images encoded with ``restart_marker_rows=ROWS`` (a restart interval of
ROWS MCU rows), cold ``GpuJpegSource.get`` passes with ``restart="lane"`` (one
lane walks the whole stream) against ``"intervals"`` (one lane per restart
interval), for ``entropy_on="gpu"`` and ``"gpu_parallel"``: four arms
alternating in one process, ``--reps`` repetitions after a warm-up of every arm,
then the cold query of each ``--queries`` size for the same four arms.

``--sampling {440,411}`` measures files of that chroma layout instead and nothing
else.  Pillow writes neither, so each file is a Pillow file whose MCUs have the
same block structure with its frame header rewritten to 500x375: a 4:2:2 file
of 375x500 becomes 4:4:0 (luma 1x2), a 4:2:0 file of 256x752 becomes 4:1:1
(luma 4x1, 16 x 47 MCUs either way).  The pictures are scrambled, the work per
file is a photograph's.  Cold ``GpuJpegSource.get`` passes with
``sampling="fallback"`` (every file through Pillow in ``decode_batch``'s serial
loop) against ``"native"``, for ``entropy_on="host"`` at ``--threads``, ``"gpu"``
and ``"gpu_parallel"``: six arms alternating in one process, ``--reps``
repetitions after a warm-up of every arm, then the cold query of each
``--queries`` size for the same six arms.

    python tools/jpeg_bench.py [--images 2000] [--threads 8] [--out profiles/jpeg_bench.log]
    python tools/jpeg_bench.py --progressive --queries 64 --out profiles/jpeg_bench_progressive.log
    python tools/jpeg_bench.py --restart 1 --queries 64,400 --out profiles/jpeg_bench_restart.log
    python tools/jpeg_bench.py --sampling 440 --queries 64 --out profiles/jpeg_bench_sampling.log
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# --sampling: (source width, source height, Pillow subsampling, luma sampling byte) of a 500x375 file
SAMPLING = {"440": (375, 500, 1, 0x12), "411": (256, 752, 2, 0x41)}


def rewrite_frame(path: str, hv: int, w: int, h: int) -> None:
    """The file's SOF0 made to say w x h with the first component sampled ``hv``."""
    with open(path, "rb") as f:
        d = bytearray(f.read())
    pos = 2
    while d[pos + 1] != 0xC0:
        assert d[pos] == 0xFF and d[pos + 1] != 0xDA, "no baseline frame header"
        pos += 2 + ((d[pos + 2] << 8) | d[pos + 3])
    d[pos + 5:pos + 7] = h.to_bytes(2, "big")
    d[pos + 7:pos + 9] = w.to_bytes(2, "big")
    d[pos + 11] = hv
    with open(path, "wb") as f:
        f.write(d)


def make_images(d: str, n: int, seed: int = 0, progressive: bool = False, restart_rows: int = 0,
                sampling: str = "") -> int:
    """Smooth structure plus noise: files of a photograph's size (~40-60 KB), not of flat colour."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    sw, sh, sub, hv = SAMPLING.get(sampling, (500, 375, 2, 0))
    yy, xx = np.mgrid[0:sh, 0:sw]
    total = 0
    for i in range(n):
        ph = rng.uniform(0, 6.28, 6)
        fx, fy = rng.uniform(8, 60, 3), rng.uniform(8, 60, 3)
        a = np.stack([127.5 + 90 * np.sin(xx / fx[c] + ph[c]) * np.cos(yy / fy[c] + ph[3 + c]) for c in range(3)], 2)
        a = np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)
        p = os.path.join(d, f"test_{i}.JPEG")
        kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
        Image.fromarray(a, "RGB").save(p, "JPEG", quality=90, subsampling=sub, progressive=progressive, **kw)
        if sampling:
            rewrite_frame(p, hv, 500, 375)
        total += os.path.getsize(p)
    return total


def progressive_report(a, dev, say) -> None:
    """``--progressive``: fallback against native on progressive files, six arms."""
    import torch

    from idunno.runtime.data import GpuJpegSource

    n = a.images
    arms = [(f"{on:12s} {mode}", on, mode) for on in ("host", "gpu", "gpu_parallel") for mode in ("fallback", "native")]

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        x = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, x

    with tempfile.TemporaryDirectory() as d, torch.cuda.device(dev):
        t0 = time.perf_counter()
        nbytes = make_images(d, n, progressive=True)
        say(f"{n} progressive images 500x375 4:2:0 q90, {nbytes / n / 1024:.1f} KiB each, generated in "
            f"{time.perf_counter() - t0:.1f} s; {torch.cuda.get_device_name(0)}; {a.threads} threads (host form)")

        def source(on, mode):
            return GpuJpegSource(dev, root=d, threads=a.threads, entropy_on=on, progressive=mode)

        def passes(q, label):
            want = None
            for _, on, mode in arms:                                # warm-up of every arm
                src = source(on, mode)
                got = src.get(0, q - 1)
                assert src.fallbacks == (q if mode == "fallback" else 0), (on, mode, src.fallbacks)
                assert src.progressive_images == (0 if mode == "fallback" else q)
                if mode == "native":                                # the three native forms give the same pixels
                    assert want is None or torch.equal(got, want), on
                    want = got
                else:
                    diff = (got.int() - want.int()).abs() if want is not None else None
                    if diff is not None:
                        say(f"{label}: {on} fallback (Pillow) against native over {q} images: max |diff| "
                            f"{int(diff.max())}, mean {float(diff.float().mean()):.4f}")
                del got
            del want
            res = {name: {"s": [], "entropy_s": [], "cpu_s": []} for name, *_ in arms}
            for r in range(a.reps):
                for name, on, mode in arms:
                    src = source(on, mode)
                    c0 = time.process_time()
                    dt, y = timed(lambda: src.get(0, q - 1))
                    cpu = time.process_time() - c0
                    assert src.decoded == q
                    res[name]["s"].append(dt)
                    res[name]["entropy_s"].append(src.seconds["entropy_s"])
                    res[name]["cpu_s"].append(cpu)
                    say(f"{label} rep {r}: {name:24s} {1e3 * dt:10.2f} ms  {q / dt:9.1f} img/s  entropy "
                        f"{1e3 * src.seconds['entropy_s']:9.2f} ms  host CPU {cpu:7.3f} s")
                    del y, src
            return res

        res = passes(n, "full pass")
        say(f"progressive files, cold GpuJpegSource.get of {n} images (entropy: host wall over the decode threads / "
            "device events of the kernels; fallback decodes in Pillow after them):")
        for name, *_ in arms:
            v = [n / s for s in res[name]["s"]]
            say(f"  {name:24s} median {np.median(v):9.1f} img/s  min {min(v):9.1f}  max {max(v):9.1f} | entropy "
                f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms | host CPU {np.median(res[name]['cpu_s']):7.3f} s")
        for q in [int(x) for x in a.queries.split(",") if x]:
            q = min(q, n)
            res = passes(q, f"query {q}")
            say(f"progressive files, cold query of {q} images, GpuJpegSource.get (wall):")
            for name, *_ in arms:
                v = [1e3 * s for s in res[name]["s"]]
                say(f"  {name:24s} median {np.median(v):9.2f} ms  min {min(v):9.2f}  max {max(v):9.2f} | entropy "
                    f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms | host CPU {np.median(res[name]['cpu_s']):7.3f} s")


def sampling_report(a, dev, say) -> None:
    """``--sampling {440,411}``: fallback against native on files of that layout, six arms."""
    import torch

    from idunno.runtime.data import GpuJpegSource

    n = a.images
    layout = {"440": "4:4:0 (luma 1x2)", "411": "4:1:1 (luma 4x1)"}[a.sampling]
    arms = [(f"{on:12s} {mode}", on, mode) for on in ("host", "gpu", "gpu_parallel") for mode in ("fallback", "native")]

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        x = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, x

    with tempfile.TemporaryDirectory() as d, torch.cuda.device(dev):
        t0 = time.perf_counter()
        nbytes = make_images(d, n, sampling=a.sampling)
        say(f"{n} images 500x375 {layout} q90, {nbytes / n / 1024:.1f} KiB each, generated in "
            f"{time.perf_counter() - t0:.1f} s; {torch.cuda.get_device_name(0)}; {a.threads} threads (host form)")

        def source(on, mode):
            return GpuJpegSource(dev, root=d, threads=a.threads, entropy_on=on, sampling=mode)

        def passes(q, label):
            want = None
            for _, on, mode in arms:                                # warm-up of every arm
                src = source(on, mode)
                got = src.get(0, q - 1)
                assert src.fallbacks == (q if mode == "fallback" else 0), (on, mode, src.fallbacks)
                assert src.sampling_images == (0 if mode == "fallback" else q)
                if mode == "native":                                # the three native forms give the same pixels
                    assert want is None or torch.equal(got, want), on
                    want = got
                elif want is not None:
                    diff = (got.int() - want.int()).abs()
                    say(f"{label}: {on} fallback (Pillow) against native over {q} images: max |diff| "
                        f"{int(diff.max())}, mean {float(diff.float().mean()):.4f}")
                del got
            del want
            res = {name: {"s": [], "entropy_s": [], "cpu_s": []} for name, *_ in arms}
            for r in range(a.reps):
                for name, on, mode in arms:
                    src = source(on, mode)
                    c0 = time.process_time()
                    dt, y = timed(lambda: src.get(0, q - 1))
                    cpu = time.process_time() - c0
                    assert src.decoded == q
                    res[name]["s"].append(dt)
                    res[name]["entropy_s"].append(src.seconds["entropy_s"])
                    res[name]["cpu_s"].append(cpu)
                    say(f"{label} rep {r}: {name:24s} {1e3 * dt:10.2f} ms  {q / dt:9.1f} img/s  entropy "
                        f"{1e3 * src.seconds['entropy_s']:9.2f} ms  host CPU {cpu:7.3f} s")
                    del y, src
            return res

        res = passes(n, "full pass")
        say(f"{layout} files, cold GpuJpegSource.get of {n} images (entropy: host wall over the decode threads / "
            "device events of the kernels; fallback decodes in Pillow after them):")
        for name, *_ in arms:
            v = [n / s for s in res[name]["s"]]
            say(f"  {name:24s} median {np.median(v):9.1f} img/s  min {min(v):9.1f}  max {max(v):9.1f} | entropy "
                f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms | host CPU {np.median(res[name]['cpu_s']):7.3f} s")
        for on in ("host", "gpu", "gpu_parallel"):
            fb, nat = (np.median(res[f"{on:12s} {mode}"]["s"]) for mode in ("fallback", "native"))
            say(f"  {on}: fallback / native = {fb / nat:.2f}x (medians)")
        for q in [int(x) for x in a.queries.split(",") if x]:
            q = min(q, n)
            res = passes(q, f"query {q}")
            say(f"{layout} files, cold query of {q} images, GpuJpegSource.get (wall):")
            for name, *_ in arms:
                v = [1e3 * s for s in res[name]["s"]]
                say(f"  {name:24s} median {np.median(v):9.2f} ms  min {min(v):9.2f}  max {max(v):9.2f} | entropy "
                    f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms | host CPU {np.median(res[name]['cpu_s']):7.3f} s")
            for on in ("host", "gpu", "gpu_parallel"):
                fb, nat = (np.median(res[f"{on:12s} {mode}"]["s"]) for mode in ("fallback", "native"))
                say(f"  {on}: fallback / native = {fb / nat:.2f}x (medians)")


def restart_report(a, dev, say) -> None:
    """``--restart ROWS``: one lane per file against one lane per restart interval, four arms."""
    import torch

    from idunno.runtime.data import GpuJpegSource

    n = a.images
    arms = [(f"{on:12s} {mode}", on, mode) for on in ("gpu", "gpu_parallel") for mode in ("lane", "intervals")]

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        x = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, x

    with tempfile.TemporaryDirectory() as d, torch.cuda.device(dev):
        t0 = time.perf_counter()
        nbytes = make_images(d, n, restart_rows=a.restart)
        say(f"{n} images 500x375 4:2:0 q90 with restart_marker_rows={a.restart} "
            f"({-(-24 // a.restart)} restart intervals each), {nbytes / n / 1024:.1f} KiB each, generated in "
            f"{time.perf_counter() - t0:.1f} s; {torch.cuda.get_device_name(0)}")

        def source(on, mode):
            return GpuJpegSource(dev, root=d, threads=a.threads, entropy_on=on, restart=mode)

        def passes(q, label):
            want = GpuJpegSource(dev, root=d, threads=a.threads).get(0, q - 1)      # the host form
            for _, on, mode in arms:                                # warm-up of every arm; the outputs must agree
                src = source(on, mode)
                assert torch.equal(src.get(0, q - 1), want), (on, mode)
                assert src.fallbacks == 0 and src.restart_images == (q if mode == "intervals" else 0), (on, mode)
            del want
            res = {name: {"s": [], "entropy_s": [], "cpu_s": []} for name, *_ in arms}
            for r in range(a.reps):
                for name, on, mode in arms:
                    src = source(on, mode)
                    c0 = time.process_time()
                    dt, y = timed(lambda: src.get(0, q - 1))
                    cpu = time.process_time() - c0
                    assert src.decoded == q and src.fallbacks == 0
                    res[name]["s"].append(dt)
                    res[name]["entropy_s"].append(src.seconds["entropy_s"])
                    res[name]["cpu_s"].append(cpu)
                    say(f"{label} rep {r}: {name:24s} {1e3 * dt:10.2f} ms  {q / dt:9.1f} img/s  entropy "
                        f"{1e3 * src.seconds['entropy_s']:9.2f} ms  host CPU {cpu:7.3f} s")
                    del y, src
            return res

        res = passes(n, "full pass")
        say(f"restart-interval files, cold GpuJpegSource.get of {n} images (entropy: device events of the kernels):")
        for name, *_ in arms:
            v = [n / s for s in res[name]["s"]]
            say(f"  {name:24s} median {np.median(v):9.1f} img/s  min {min(v):9.1f}  max {max(v):9.1f} | entropy "
                f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms | host CPU {np.median(res[name]['cpu_s']):7.3f} s")
        for q in [int(x) for x in a.queries.split(",") if x]:
            q = min(q, n)
            res = passes(q, f"query {q}")
            say(f"restart-interval files, cold query of {q} images, GpuJpegSource.get (wall):")
            for name, *_ in arms:
                v = [1e3 * s for s in res[name]["s"]]
                say(f"  {name:24s} median {np.median(v):9.2f} ms  min {min(v):9.2f}  max {max(v):9.2f} | entropy "
                    f"{1e3 * np.median(res[name]['entropy_s']):9.2f} ms ({1e6 * np.median(res[name]['entropy_s']) / q:7.1f} "
                    f"us/image) | host CPU {np.median(res[name]['cpu_s']):7.3f} s")
            for on in ("gpu", "gpu_parallel"):
                lane, iv = (np.median(res[f"{on:12s} {mode}"]["s"]) for mode in ("lane", "intervals"))
                say(f"  {on}: lane / intervals = {lane / iv:.2f}x (medians)")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpu-chunks", default="256,1024,2048", help="GpuJpegSource.CHUNK_GPU values of the device entropy rows")
    ap.add_argument("--par-chunks", default="64,256,1024", help="GpuJpegSource.CHUNK_GPU_PARALLEL values of the sub-stream rows")
    ap.add_argument("--queries", default="64,400", help="sizes of the small cold queries")
    ap.add_argument("--entropy-only", action="store_true", help="only the host / device entropy comparison")
    ap.add_argument("--progressive", action="store_true",
                    help="measure progressive files only: progressive='fallback' against 'native' in the three forms")
    ap.add_argument("--restart", type=int, default=0, metavar="ROWS", nargs="?", const=1,
                    help="measure restart-interval files only (restart_marker_rows=ROWS, default 1): restart='lane' "
                         "against 'intervals' in the two device forms")
    ap.add_argument("--sampling", default=None, choices=sorted(SAMPLING),
                    help="measure 4:4:0 (440) or 4:1:1 (411) files only: sampling='fallback' against 'native' in the "
                         "three forms")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        print("jpeg_bench: no GPU: this tool measures the GPU decode path and has no fallback", file=sys.stderr)
        return 2
    from idunno import ops
    from idunno.runtime.data import GpuJpegSource, JpegSource

    ops.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    n = a.images
    if a.progressive or a.restart or a.sampling:
        if a.restart < 0 or (a.progressive and a.restart):
            ap.error("--restart takes a positive number of MCU rows and does not combine with --progressive")
        if a.sampling and (a.progressive or a.restart):
            ap.error("--sampling does not combine with --progressive or --restart")
        (sampling_report if a.sampling else progressive_report if a.progressive else restart_report)(a, dev, say)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    with tempfile.TemporaryDirectory() as d, torch.cuda.device(dev):
        t0 = time.perf_counter()
        nbytes = make_images(d, n)
        say(f"{n} images 500x375 4:2:0 q90, {nbytes / n / 1024:.1f} KiB each, generated in {time.perf_counter() - t0:.1f} s; "
            f"{torch.cuda.get_device_name(0)}; {a.threads} threads")
        pil = JpegSource(dev, root=d, workers=a.threads)

        def timed(f):
            torch.cuda.synchronize()
            t = time.perf_counter()
            x = f()
            torch.cuda.synchronize()
            return time.perf_counter() - t, x

        # warm-up: page cache, code objects, pinned buffers, thread pools
        w = min(n, 64)
        timed(lambda: pil.get(0, w - 1))
        timed(lambda: GpuJpegSource(dev, root=d, threads=a.threads).get(0, w - 1))
        if not a.entropy_only:
            rates = {"pil": [], "cold": [], "warm": []}
            split = {"entropy_s": [], "h2d_s": [], "idct_s": [], "resize_s": []}
            ref = None
            for r in range(a.reps):
                dt, x = timed(lambda: pil.get(0, n - 1))
                rates["pil"].append(n / dt)
                gpu = GpuJpegSource(dev, root=d, threads=a.threads)
                dt, y = timed(lambda: gpu.get(0, n - 1))
                rates["cold"].append(n / dt)
                for k in split:
                    split[k].append(gpu.seconds[k])
                assert gpu.decoded == n and gpu.fallbacks == 0
                dt, z = timed(lambda: gpu.get(0, n - 1))
                rates["warm"].append(n / dt)
                assert gpu.decoded == n and torch.equal(y, z)
                if ref is None:
                    diff = (x.int() - y.int()).abs()
                    ref = (int(diff.max()), float(diff.float().mean()))
                say(f"rep {r}: JpegSource {rates['pil'][-1]:9.1f} img/s | GpuJpegSource cold {rates['cold'][-1]:9.1f} img/s | "
                    f"warm {rates['warm'][-1]:12.1f} img/s")
                del x, y, z, gpu
            say(f"GPU output vs Pillow output over {n} images: max |diff| {ref[0]}, mean {ref[1]:.4f}")
            for k, name in (("pil", "JpegSource.get (Pillow, threads)"), ("cold", "GpuJpegSource.get cold"),
                            ("warm", "GpuJpegSource.get warm")):
                v = rates[k]
                say(f"{name:34s} median {np.median(v):12.1f} img/s  min {min(v):12.1f}  max {max(v):12.1f}  "
                    f"spread {100 * (max(v) - min(v)) / np.median(v):.1f} %")
            say(f"cold / Pillow = {np.median(rates['cold']) / np.median(rates['pil']):.2f}x (medians)")
            for k, name in (("entropy_s", "entropy decode (host, wall)"), ("h2d_s", "H2D of coefficients (events)"),
                            ("idct_s", "jpeg_idct_kernel (events)"), ("resize_s", "jpeg_resize_crop_kernel (events)")):
                v = split[k]
                say(f"  cold split: {name:34s} median {1e3 * np.median(v):9.2f} ms  ({1e6 * np.median(v) / n:8.2f} us/image)")
            # bytes the kernels move per image: 500x375 4:2:0 = 32x24 MCUs of 6 blocks
            blocks = 32 * 24 * 6
            idct_b = blocks * (128 + 64)
            say(f"  jpeg_idct_kernel: {blocks} blocks/image, {idct_b} B/image read+written -> "
                f"{n * idct_b / np.median(split['idct_s']) / 1e9:.1f} GB/s")
            say(f"  jpeg_resize_crop_kernel: {224 * 224 * 3} B/image written -> "
                f"{n * 224 * 224 * 3 / np.median(split['resize_s']) / 1e9:.2f} GB/s of output")
        # ---- entropy stage: host threads against the device kernel, same process, alternating ----
        forms = [(f"host, {a.threads} threads", "host", a.threads, None), ("host, 2 threads", "host", 2, None)]
        forms += [(f"gpu, chunk {c}", "gpu", a.threads, int(c)) for c in a.gpu_chunks.split(",") if c]
        forms += [(f"gpu_parallel, chunk {c}", "gpu_parallel", a.threads, int(c)) for c in a.par_chunks.split(",") if c]

        def source(on, threads, chunk):
            src = GpuJpegSource(dev, root=d, threads=threads, entropy_on=on)
            if chunk is not None:
                src.CHUNK_GPU = src.CHUNK_GPU_PARALLEL = chunk
            return src

        want = source("host", a.threads, None).get(0, n - 1)
        for _, on, threads, chunk in forms:                     # warm-up of every form; the outputs must agree
            got = source(on, threads, chunk).get(0, n - 1)
            assert torch.equal(got, want), (on, threads, chunk)
            del got
        del want
        res = {name: {"rate": [], "entropy_s": [], "h2d_s": [], "h2d_b": [], "cpu_s": []} for name, *_ in forms}
        for r in range(a.reps):
            for name, on, threads, chunk in forms:
                src = source(on, threads, chunk)
                c0 = time.process_time()
                dt, y = timed(lambda: src.get(0, n - 1))
                cpu = time.process_time() - c0
                assert src.decoded == n and src.fallbacks == 0
                v = res[name]
                v["rate"].append(n / dt)
                v["entropy_s"].append(src.seconds["entropy_s"])
                v["h2d_s"].append(src.seconds["h2d_s"])
                v["h2d_b"].append(src.stager.bytes_staged)
                v["cpu_s"].append(cpu)
                say(f"entropy rep {r}: {name:24s} {n / dt:9.1f} img/s  entropy {1e3 * src.seconds['entropy_s']:8.2f} ms  "
                    f"H2D {src.stager.bytes_staged / 1e6:8.1f} MB in {1e3 * src.seconds['h2d_s']:7.2f} ms  host CPU {cpu:6.3f} s")
                del y, src
        say("entropy stage, cold GpuJpegSource.get (entropy: host wall over the decode threads / device events of the kernel):")
        for name, *_ in forms:
            v = res[name]
            say(f"  {name:24s} median {np.median(v['rate']):9.1f} img/s  min {min(v['rate']):9.1f}  max {max(v['rate']):9.1f} | "
                f"entropy {1e3 * np.median(v['entropy_s']):8.2f} ms ({1e6 * np.median(v['entropy_s']) / n:7.1f} us/image) | "
                f"H2D {np.median(v['h2d_b']) / 1e6:8.1f} MB {1e3 * np.median(v['h2d_s']):7.2f} ms | "
                f"host CPU {np.median(v['cpu_s']):6.3f} s")
        # ---- small cold queries: a fresh source per query, default chunk sizes, forms alternating ----
        qforms = [(f"host, {a.threads} threads", "host", a.threads), ("host, 2 threads", "host", 2),
                  ("gpu", "gpu", a.threads), ("gpu_parallel", "gpu_parallel", a.threads)]
        for q in [int(x) for x in a.queries.split(",") if x]:
            q = min(q, n)
            want = source("host", a.threads, None).get(0, q - 1)
            for _, on, threads in qforms:                           # warm-up of every form at this size
                assert torch.equal(source(on, threads, None).get(0, q - 1), want), (on, threads, q)
            del want
            qres = {name: {"ms": [], "entropy_ms": [], "cpu_s": []} for name, *_ in qforms}
            for r in range(a.reps):
                for name, on, threads in qforms:
                    src = source(on, threads, None)
                    c0 = time.process_time()
                    dt, y = timed(lambda: src.get(0, q - 1))
                    cpu = time.process_time() - c0
                    assert src.decoded == q and src.fallbacks == 0
                    qres[name]["ms"].append(1e3 * dt)
                    qres[name]["entropy_ms"].append(1e3 * src.seconds["entropy_s"])
                    qres[name]["cpu_s"].append(cpu)
                    say(f"query {q} rep {r}: {name:18s} {1e3 * dt:9.2f} ms  entropy {1e3 * src.seconds['entropy_s']:8.2f} ms  "
                        f"host CPU {cpu:6.3f} s")
                    del y, src
            say(f"cold query of {q} images, GpuJpegSource.get (wall; entropy: host wall / device events of the kernels):")
            for name, *_ in qforms:
                v = qres[name]
                say(f"  {name:18s} median {np.median(v['ms']):9.2f} ms  min {min(v['ms']):9.2f}  max {max(v['ms']):9.2f} | "
                    f"entropy {np.median(v['entropy_ms']):8.2f} ms ({1e3 * np.median(v['entropy_ms']) / q:7.1f} us/image) | "
                    f"host CPU {np.median(v['cpu_s']):6.3f} s")
            g, p_ = np.median(qres["gpu"]["ms"]), np.median(qres["gpu_parallel"]["ms"])
            h = np.median(qres[qforms[0][0]]["ms"])
            say(f"  gpu / gpu_parallel = {g / p_:.2f}x, host {a.threads} threads / gpu_parallel = {h / p_:.2f}x (medians)")
        # ---- synchronisation rounds of the sub-stream kernel on these files (host emulation, same code) ----
        datas = [open(os.path.join(d, f"test_{i}.JPEG"), "rb").read() for i in range(n)]
        rounds = np.asarray(ops.jpeg_huff_par_rounds(datas))
        say(f"sub-stream kernel: {ops.JPEG_PAR_SUB_BITS} bits per sub-stream, {ops.JPEG_PAR_THREADS} threads per image, "
            f"round cap {ops.JPEG_PAR_MAX_ROUNDS}; rounds over {n} files: min {rounds.min()}  median {int(np.median(rounds))}  "
            f"max {rounds.max()}  (0 = not converged: {int((rounds == 0).sum())} files)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
