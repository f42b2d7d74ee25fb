#!/usr/bin/env python3
"""ShuffleNetV2 x0.5 / x1.0 / x1.5 on the fused shuffle-unit kernel: every launch of the forward timed on real
activations (median of --reps windows of --iters calls, with the fastest and slowest window) with its useful
TFLOP/s and the band plan it ran with, then the whole forward in img/s in both precisions with two arms in the same
process, their windows interleaved: (a) this path as a hipGraph replay (and as eager launches), (b) PyTorch's own
eager forward of the reference module in the same precision on the same card.  The unfused composition on this
project's ops (conv1x1_narrow + conv_dw + a torch shuffle) is not timed here.

usage: python tools/bench_shufflenet.py [--batch 400] [--iters 5] [--reps 5] [--models shufflenet_v2_x1_0,...]
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
    """[(median, min, max) us per call] of each arm after two warm-up calls each; the arms' windows alternate."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(window(fn, iters))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def launches(runner, o, img):
    """(name, useful FLOPs, plan text, call) for every launch of the forward, in order, on real activations."""
    p, s = runner.p, runner.p.stem
    f32 = p.dtype == "fp32"
    B = img.shape[0]
    x0 = o.preprocess(img, f32=f32)
    x1 = o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)
    x = o.maxpool2d(x1, 3, 2, 1)
    out = [(f"stem 3x3/2 3->24 @224->{x1.shape[1]}", B * x1.shape[1] * x1.shape[2] * s.flops_per_out_pixel, "",
            lambda: o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)),
           (f"pool 3/2 @{x1.shape[1]}->{x.shape[1]}", 0, "", lambda: o.maxpool2d(x1, 3, 2, 1))]
    for _, u in p.features:
        pl = o.shuffle_plan(x.shape[1], x.shape[2], u.cin, u.c, u.stride, f32)
        call = lambda u=u, x=x: o.shuffle_unit(x, u.w1, u.b1, u.wd, u.bd, u.w2, u.b2, u.stride, u.wd1, u.bd1, u.wp1,
                                               u.bp1, c=u.c)
        out.append((f"unit s{u.stride} {u.cin}->{u.c} @{x.shape[1]}", B * u.flops(x.shape[1])[0],
                    f"R {pl['R']} x {pl['bands']}, imgs {pl['imgs']}, {pl['lds'] / 1024:.1f} KiB", call))
        x = call()
    c5, fc = p.last, p.fcs[0]
    y = o.conv1x1_narrow(x, c5.w, c5.b, c5.act)
    out.append((f"conv5 {c5.cin}->{c5.cout} @{x.shape[1]}", B * x.shape[1] * x.shape[2] * c5.flops_per_out_pixel, "",
                lambda: o.conv1x1_narrow(x, c5.w, c5.b, c5.act)))
    out.append((f"pool @{x.shape[1]}", 0, "", lambda: o.global_avgpool(y)))
    pooled = o.global_avgpool(y)
    out.append((f"fc {fc.cin}->{fc.cout}", B * fc.flops_per_out_pixel, "",
                lambda: o.linear(pooled, fc.w, fc.b, relu=False, out_f32=True)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="shufflenet_v2_x0_5,shufflenet_v2_x1_0,shufflenet_v2_x1_5")
    a = ap.parse_args()
    from idunno import ops as o
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    o.load()
    dev, B = "cuda", a.batch
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    print(f"device {torch.cuda.get_device_name(0)}, batch {B}, median [min .. max] of {a.reps} windows of {a.iters} calls")
    for name in a.models.split(","):
        m = ref.build(name, seed=7, randomize_bn=True)
        for dtype in ("fp16", "fp32"):
            runner = HipRunner(compile_model(m, name, dtype=dtype))
            per = launches(runner, o, img)
            print(f"\n## {name} {dtype}: per launch at B = {B}\n\n| launch | plan | us | min .. max | useful TFLOP/s |\n"
                  "|---|---|---:|---:|---:|")
            tot = 0.0
            for lname, flops, plan, fn in per:
                (us, lo, hi), = timeit([fn], a.iters, a.reps)
                tot += us
                print(f"| {lname} | {plan} | {us:.1f} | {lo:.1f} .. {hi:.1f} | {flops / us / 1e6:.1f} |")
            print(f"| sum of {len(per)} launches | | {tot:.1f} | | {runner.flops_per_image() * B / tot / 1e6:.1f} |")
            del per
            sin, replay = runner.capture(B)
            sin.copy_(img)
            tdt = torch.float32 if dtype == "fp32" else torch.float16
            tm = ref.build(name, seed=7, randomize_bn=True).to(dev, tdt)
            x = ref.preprocess_u8(img).to(tdt)
            with torch.no_grad():
                (g, glo, ghi), (e, elo, ehi), (t, tlo, thi) = timeit(
                    [replay, lambda: runner.forward(img), lambda: tm(x)], a.iters, a.reps)
            print(f"\n{name} {dtype} (a) whole forward, hipGraph replay: {g / 1e3:.3f} ms [{glo / 1e3:.3f} .. {ghi / 1e3:.3f}] "
                  f"= {B / g * 1e6:.0f} img/s; eager launches: {e / 1e3:.3f} ms [{elo / 1e3:.3f} .. {ehi / 1e3:.3f}] "
                  f"= {B / e * 1e6:.0f} img/s")
            print(f"{name} {dtype} (b) PyTorch eager forward of the reference module: {t / 1e3:.3f} ms "
                  f"[{tlo / 1e3:.3f} .. {thi / 1e3:.3f}] = {B / t * 1e6:.0f} img/s")
            runner.close()
            del runner, sin, replay, tm, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
