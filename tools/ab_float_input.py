#!/usr/bin/env python3
"""Same-process A/B of the two kinds of HipRunner input on the same images: the
uint8 [B,224,224,3] batch (fused uint8 stem) against the normalised float
[B,3,224,224] batch (ops.float_to_* producer + unfused stem).  Each forward is
captured once as a hipGraph; the graphs are timed in interleaved rounds on one
device, like tools/ab_flag.py.

usage: python tools/ab_float_input.py [--model resnet18] [--batch 400] [--dtype fp32]
       python tools/ab_float_input.py --producers    (a few launches of each producer, for a
                                                      `rocprofv3 --kernel-trace --stats` run of its own)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def producers(ops, u, x, iters):
    """The float producers and the uint8 kernels they stand in for, same output bytes."""
    for _ in range(iters):
        ops.preprocess_pack3_split(u, 7, 2, 3)
        ops.float_to_pack3_split(x, 7, 2, 3)
        ops.preprocess_pack3(u, 7, 2, 3)
        ops.float_to_pack3(x, 7, 2, 3)
        ops.preprocess(u)
        ops.float_to_nhwc4(x.half())
        ops.float_to_pack3_split(x.contiguous(memory_format=torch.channels_last), 7, 2, 3)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--producers", action="store_true")
    a = ap.parse_args()
    from idunno import ops
    from idunno.models import HipRunner, build_program
    from idunno.models.reference import preprocess_u8

    ops.load()
    dev = torch.device("cuda")
    u = ops.synth_images(1234, 0, a.batch, dev)
    x = preprocess_u8(u).contiguous()          # NCHW
    if a.producers:
        return producers(ops, u, x, a.iters)
    in_dtype = torch.float16 if a.dtype == "fp16" else torch.float32
    r = HipRunner(build_program(a.model, dtype=a.dtype), dev)
    runs, outs = {}, {}
    for kind, images, dt in (("uint8", u, None), ("float", x.to(in_dtype), in_dtype)):
        sin, runs[kind] = r.capture(a.batch, in_dtype=dt)
        sin.copy_(images)
        cls, prob = runs[kind]()
        torch.cuda.synchronize()
        outs[kind] = (cls.clone(), prob.clone())
    agree = (outs["uint8"][0] == outs["float"][0]).float().mean().item()
    dprob = (outs["uint8"][1] - outs["float"][1]).abs().max().item()
    print(f"top-1 agreement uint8 vs float input {agree:.4f}, max |dprob| {dprob:.2e}", flush=True)
    res = {k: [] for k in runs}
    for _ in range(a.rounds):
        for kind, run in runs.items():
            run()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            res[kind].append(t0.elapsed_time(t1) / a.iters)
    for kind, v in res.items():
        print(f"{kind:5s} input {a.model} {a.dtype} b{a.batch}: median {statistics.median(v):.4f} ms  "
              f"min {min(v):.4f} ms  rounds {[round(t, 4) for t in v]}", flush=True)
    print(f"float / uint8 time: {statistics.median(res['float']) / statistics.median(res['uint8']):.3f}x", flush=True)


if __name__ == "__main__":
    main()
