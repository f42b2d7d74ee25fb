#!/usr/bin/env python3
"""Same-process A/B of a HipRunner attribute (kernel choice is a call argument
the runner passes, never a process-global switch): the whole forward hipGraph
is captured once per value (the attribute is read at capture, so each graph
keeps its setting), then the two graphs are timed in interleaved rounds on one
device (cdna_hip_programming §5.4 rule 24).

usage: python tools/ab_flag.py --attr side_down [--model resnet18] [--batch 400] [--dtype fp32]
       python tools/ab_flag.py --attr astem_form --values 0,1 --model alexnet --batch 500
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attr", required=True, help="HipRunner attribute to switch")
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--values", default=None, help="'a,b' integer values instead of False,True")
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    from idunno import ops
    from idunno.models import HipRunner, build_program

    ops.load()
    dev = torch.device("cuda")
    prog = build_program(a.model, dtype=a.dtype)
    shard = ops.synth_images(1234, 0, a.batch, dev)
    runs, outs, keep = {}, {}, []
    vals = (False, True) if not a.values else tuple(int(v) for v in a.values.split(","))
    for flag in vals:
        r = HipRunner(prog, dev)
        assert hasattr(r, a.attr), f"HipRunner has no attribute {a.attr!r}"
        setattr(r, a.attr, flag)
        keep.append(r)
        _start, run = r.capture_window(shard, a.batch)
        runs[flag] = run
        cls, prob = run()
        torch.cuda.synchronize()
        outs[flag] = (cls.clone(), prob.clone())
    v0, v1 = vals
    agree = (outs[v0][0] == outs[v1][0]).float().mean().item()
    dprob = (outs[v0][1] - outs[v1][1]).abs().max().item()
    print(f"{a.attr}: top-1 agreement off vs on {agree:.4f}, max |dprob| {dprob:.2e}", flush=True)
    res = {k: [] for k in runs}
    for _ in range(a.rounds):
        for flag, run in runs.items():
            run()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            res[flag].append(t0.elapsed_time(t1) / a.iters)
    for flag, v in res.items():
        print(f"{a.attr}({flag!s:5s}) {a.model} b{a.batch}: median {statistics.median(v):.4f} ms  "
              f"min {min(v):.4f} ms  rounds {[round(x, 4) for x in v]}", flush=True)
    off, on = statistics.median(res[v0]), statistics.median(res[v1])
    print(f"on vs off: {100 * (off / on - 1):+.2f}% throughput", flush=True)


if __name__ == "__main__":
    main()
