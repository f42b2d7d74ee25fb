#!/usr/bin/env python3
"""Event-timed ``ops.resize_crop_u8`` against a device copy of the same byte count, in one
process, alternating (what docs/KERNELS.md "resize_crop_u8" quotes).

Nominal bytes of the kernel = the whole input batch + the output batch; the copy moves the
same total (reads half of it, writes half of it).  The kernel reads less than the nominal
input (only the rows and columns the crop's taps touch, band halos twice), so its share of
the copy rate is a figure of merit for the whole operation, not a bandwidth.

usage: python tools/resize_u8_bench.py [--images 2000] [--hw 375,500] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--hw", default="375,500")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("resize_u8_bench: no GPU: this tool measures the GPU kernel and has no fallback", file=sys.stderr)
        return 2
    from idunno import ops

    ops.load()
    dev = torch.device("cuda")
    h, w = (int(v) for v in a.hw.split(","))
    gen = torch.Generator(device=dev).manual_seed(1234)
    img = torch.randint(0, 256, (a.images, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty(a.images, 224, 224, 3, dtype=torch.uint8, device=dev)
    nominal = img.numel() + out.numel()
    src = torch.empty(nominal // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    runs = {"resize_crop_u8": lambda: ops.resize_crop_u8(img, 256, 224, out=out), "copy": lambda: dst.copy_(src)}
    res = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            run()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            res[name].append(t0.elapsed_time(t1) / a.iters)
    plan = ops.load().resize_u8_plan(h, w, 256, 224)
    lines = [f"{a.images} images {h}x{w} -> 256 / 224 on {torch.cuda.get_device_name(0)}; nominal {nominal / 1e6:.1f} MB "
             f"(input {img.numel() / 1e6:.1f} + output {out.numel() / 1e6:.1f}); band {plan['band']} x {plan['nbands']} "
             f"workgroups per image, {plan['lds_bytes']} B LDS"]
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        lines.append(f"{k:15s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  "
                     f"{nominal / med[k] / 1e6:.0f} GB/s nominal  {1e3 * med[k] / a.images:.3f} us/image")
    lines.append(f"resize_crop_u8 runs at {100 * med['copy'] / med['resize_crop_u8']:.1f} % of the copy rate (medians)")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
