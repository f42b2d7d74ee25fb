#!/usr/bin/env python3
"""SqueezeNet 1.0 / 1.1 on the Fire, pooled-head and ceil-pool kernels: per launch HBM bytes,
time (median of --reps windows of --iters calls, with the fastest and slowest window) and
achieved GB/s, the whole forward (hipGraph replay and eager) in img/s, in both precisions.
For every distinct Fire shape, fp32 only, the fused launch against the composition the other
ops can run: conv1x1_narrow squeeze, conv1x1_narrow 1x1 expand, conv2d 3x3 on the f32 kernel,
torch.cat; the two arms alternate window by window.  (fp16 has no such baseline: no other
fp16 conv takes 16 .. 64 input channels.)

usage: python tools/bench_squeezenet.py [--batch 400] [--iters 10] [--reps 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, iters):
    """us per call of one window of ``iters`` calls, from device events."""
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) * 1000 / iters


def timeit(fns, iters, reps):
    """(median, min, max) us per call for each of ``fns``, their windows alternating, after two warm-up calls each."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(window(fn, iters))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def launches(p, o, x):
    """(name, HBM bytes, call) per launch after the stem, on real activations, and the Fire modules met."""
    out, fires = [], []
    for i, (k, v) in enumerate(p.features):
        xin = x
        if k == "pool":
            x = o.maxpool2d(xin, *v, ceil_mode=True)
            out.append((f"pool {xin.shape[3]} @{xin.shape[1]}->{x.shape[1]}", xin.nbytes + x.nbytes,
                        lambda xin=xin, v=v: o.maxpool2d(xin, *v, ceil_mode=True)))
        else:
            x = o.fire(xin, v.squeeze.w, v.squeeze.b, v.we, v.be, v.e1)
            wb = v.squeeze.w.nbytes + (v.e1 + 9 * v.e3) * v.s * v.we.element_size()
            name = f"fire {v.squeeze.cin}->{v.s}->{v.e1}+{v.e3} @{xin.shape[1]}"
            fn = lambda xin=xin, v=v: o.fire(xin, v.squeeze.w, v.squeeze.b, v.we, v.be, v.e1)
            out.append((name, xin.nbytes + x.nbytes + wb, fn))
            fires.append((name, v, xin, fn))
    c = p.last
    out.append((f"head {c.cin}->{c.cout} +pool @{x.shape[1]}", x.nbytes + c.w.nbytes + x.shape[0] * c.cout * 4,
                lambda c=c, x=x: o.conv1x1_relu_pool(x, c.w, c.b)))
    return out, fires


def unfused(o, packed, v, xin):
    """The Fire module from the ops that existed before ops.fire (fp32): three convs and a concat."""
    w1, w3 = packed.unpack_fire_weights(v.we, v.e1, v.s)
    p1 = packed.pack_pw_weight(w1.cpu(), "fp32").to(xin.device)
    p3 = packed.pack_conv_weight(w3.cpu(), "fp32")[0].to(xin.device)
    b1, b3 = v.be[:v.e1].contiguous(), v.be[v.e1:].contiguous()

    def fn():
        s = o.conv1x1_narrow(xin, v.squeeze.w, v.squeeze.b, 1)
        return torch.cat([o.conv1x1_narrow(s, p1, b1, 1), o.conv2d(s, p3, b3, 3, 3, 1, 1, True)], dim=3)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from idunno import ops as o
    from idunno.models import HipRunner, compile_model, packed
    from idunno.models import reference as ref

    o.load()
    dev, B = "cuda", a.batch
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    print(f"device {torch.cuda.get_device_name(0)}, batch {B}, median [min .. max] of {a.reps} windows of {a.iters} calls")
    seen = set()
    for name in ("squeezenet1_0", "squeezenet1_1"):
        m = ref.build(name, seed=7)
        for dtype in ("fp16", "fp32"):
            runner = HipRunner(compile_model(m, name, dtype=dtype))
            p, s = runner.p, runner.p.stem
            x0 = o.preprocess(img, f32=dtype == "fp32")
            x = o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)
            per, fires = launches(p, o, x)
            per.insert(0, (f"stem {s.kh}x{s.kw}/2 3->{s.cout} @224->{x.shape[1]}", x0.nbytes + x.nbytes + s.w.nbytes,
                           lambda: o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)))
            print(f"\n## {name} {dtype}: per launch at B = {B}\n\n| launch | MB moved | us | min .. max | GB/s |\n"
                  "|---|---:|---:|---:|---:|")
            tot_us = tot_b = 0.0
            for lname, nbytes, fn in per:
                (us, lo, hi), = timeit([fn], a.iters, a.reps)
                tot_us, tot_b = tot_us + us, tot_b + nbytes
                print(f"| {lname} | {nbytes / 1e6:.1f} | {us:.1f} | {lo:.1f} .. {hi:.1f} | {nbytes / us / 1e3:.0f} |")
            print(f"| sum | {tot_b / 1e6:.1f} | {tot_us:.1f} | | {tot_b / tot_us / 1e3:.0f} |")
            if dtype == "fp32":
                rows = [(n, v, xin, fn) for n, v, xin, fn in fires if n not in seen]
                seen.update(n for n, *_ in rows)
                if rows:
                    print(f"\n## Fire A/B, fp32, B = {B}: shapes first met in {name} (us, median [min .. max])\n\n"
                          "| module | fused ops.fire | narrow + narrow + conv2d + cat | fused / unfused |\n|---|---:|---:|---:|")
                for n, v, xin, fn in rows:
                    base = unfused(o, packed, v, xin)
                    assert (fn().double() - base().double()).abs().max().item() <= 2e-5 * fn().abs().max().item()
                    f, u = timeit([fn, base], a.iters, a.reps)
                    print(f"| {n} | {f[0]:.1f} [{f[1]:.1f} .. {f[2]:.1f}] | {u[0]:.1f} [{u[1]:.1f} .. {u[2]:.1f}] | "
                          f"{f[0] / u[0]:.2f} |")
            del x, x0, per, fires
            sin, replay = runner.capture(B)
            sin.copy_(img)
            (g, glo, ghi), = timeit([replay], a.iters, a.reps)
            (e, elo, ehi), = timeit([lambda: runner.forward(img)], a.iters, a.reps)
            print(f"\n{name} {dtype} whole forward, hipGraph replay: {g / 1e3:.3f} ms [{glo / 1e3:.3f} .. {ghi / 1e3:.3f}] "
                  f"= {B / g * 1e6:.0f} img/s; eager launches: {e / 1e3:.3f} ms [{elo / 1e3:.3f} .. {ehi / 1e3:.3f}] "
                  f"= {B / e * 1e6:.0f} img/s")
            runner.close()


if __name__ == "__main__":
    main()
