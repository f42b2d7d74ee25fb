#!/usr/bin/env python3
"""DenseNet-121 / 169 / 201 on the dense-layer, transition, pool-into and norm5-head kernels: every launch of the
forward timed on real activations (median of --reps windows of --iters calls, with the fastest and slowest window)
with its useful TFLOP/s and the band plan it ran with, the whole forward (hipGraph replay and eager) in img/s, in
both precisions -- and, as the yardstick, PyTorch's own eager forward of the reference module in the same
precision on the same card.

usage: python tools/bench_densenet.py [--batch 400] [--iters 5] [--reps 5] [--models densenet121,...] [--no-torch]
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


def timeit(fn, iters, reps):
    """(median, min, max) us per call after two warm-up calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    t = [window(fn, iters) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def launches(runner, o, img):
    """(name, useful FLOPs, plan text, call) for every launch of the forward, in order, on real activations."""
    p, s = runner.p, runner.p.stem
    f32 = p.dtype == "fp32"
    B = img.shape[0]
    x0 = o.preprocess(img, f32=f32)
    x = o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)
    out = [(f"stem 7x7/2 3->64 @224->{x.shape[1]}", B * x.shape[1] * x.shape[2] * s.flops_per_out_pixel, "",
            lambda: o.conv2d(x0, s.w, s.b, s.kh, s.kw, s.stride, s.pad, True))]
    feats, i, buf, blk = p.features, 0, None, 0
    while i < len(feats):
        n = 0
        while i + n < len(feats) and feats[i + n][0] == "dense":
            n += 1
        c0, blk = feats[i][1].cin, blk + 1
        if buf is None:
            buf = torch.empty((B, x.shape[1] // 2, x.shape[2] // 2, c0 + 32 * n), dtype=x.dtype, device=x.device)
            out.append((f"pool 3/2 into block 1 @{x.shape[1]}->{buf.shape[1]}", 0, "",
                        lambda x=x, buf=buf: o.maxpool2d_into(x, buf, 3, 2, 1)))
            o.maxpool2d_into(x, buf, 3, 2, 1)
        else:
            t, src = feats[i - 1][1], buf
            buf = torch.empty((B, src.shape[1] // 2, src.shape[2] // 2, c0 + 32 * n), dtype=src.dtype, device=src.device)
            out.append((f"transition {t.cin}->{t.cin // 2} @{src.shape[1]}->{buf.shape[1]}",
                        B * buf.shape[1] * buf.shape[2] * t.flops_per_out_pixel, "",
                        lambda t=t, src=src, buf=buf: o.dense_transition(src, t.scale, t.shift, t.w, buf)))
            o.dense_transition(src, t.scale, t.shift, t.w, buf)
        for _, d in feats[i:i + n]:
            pl = o.dense_plan(buf.shape[1], buf.shape[2], d.cin, f32)
            out.append((f"block {blk} layer {d.cin}->128->32 @{buf.shape[1]}",
                        B * buf.shape[1] * buf.shape[2] * d.flops_per_out_pixel,
                        f"R {pl['R']} x {pl['bands']}, kc {pl['kc']}, {pl['lds'] / 1024:.1f} KiB",
                        lambda d=d, buf=buf: o.dense_layer(buf, d.cin, d.scale1, d.shift1, d.w1, d.b1, d.w2)))
            o.dense_layer(buf, d.cin, d.scale1, d.shift1, d.w1, d.b1, d.w2)
        i += n + 1
    fc = p.fcs[0]
    out.append((f"norm5 + pool {buf.shape[3]} @{buf.shape[1]}", 0, "",
                lambda buf=buf: o.bn_relu_avgpool(buf, *p.head_norm)))
    pooled = o.bn_relu_avgpool(buf, *p.head_norm)
    out.append((f"fc {fc.cin}->{fc.cout}", B * fc.flops_per_out_pixel, "",
                lambda: o.linear(pooled, fc.w, fc.b, relu=False, out_f32=True)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="densenet121,densenet169,densenet201")
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch eager yardstick")
    ap.add_argument("--summary", action="store_true", help="one row a (block, H) group instead of one a launch")
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
            tot, groups = 0.0, {}
            for lname, flops, plan, fn in per:
                us, lo, hi = timeit(fn, a.iters, a.reps)
                tot += us
                key = lname.split(" layer ")[0] + (" layers @" + lname.rsplit("@", 1)[1] if " layer " in lname else "")
                g = groups.setdefault(key, [0, 0.0, 0.0, plan])
                g[0], g[1], g[2] = g[0] + 1, g[1] + us, g[2] + flops
                if not a.summary:
                    print(f"| {lname} | {plan} | {us:.1f} | {lo:.1f} .. {hi:.1f} | {flops / us / 1e6:.1f} |")
            if a.summary:
                for key, (n, us, flops, plan) in groups.items():
                    print(f"| {key} x {n} | {plan} | {us:.1f} | | {flops / us / 1e6:.1f} |")
            print(f"| sum of {len(per)} launches | | {tot:.1f} | | {runner.flops_per_image() * B / tot / 1e6:.1f} |")
            del per
            sin, replay = runner.capture(B)
            sin.copy_(img)
            g, glo, ghi = timeit(replay, a.iters, a.reps)
            e, elo, ehi = timeit(lambda: runner.forward(img), a.iters, a.reps)
            print(f"\n{name} {dtype} whole forward, hipGraph replay: {g / 1e3:.3f} ms [{glo / 1e3:.3f} .. {ghi / 1e3:.3f}] "
                  f"= {B / g * 1e6:.0f} img/s; eager launches: {e / 1e3:.3f} ms [{elo / 1e3:.3f} .. {ehi / 1e3:.3f}] "
                  f"= {B / e * 1e6:.0f} img/s")
            runner.close()
            del runner, sin, replay
            torch.cuda.empty_cache()
            if not a.no_torch:
                tdt = torch.float32 if dtype == "fp32" else torch.float16
                tm = ref.build(name, seed=7, randomize_bn=True).to(dev, tdt)
                x = ref.preprocess_u8(img).to(tdt)
                with torch.no_grad():
                    t, tlo, thi = timeit(lambda: tm(x), a.iters, a.reps)
                print(f"{name} {dtype} PyTorch eager forward of the reference module (yardstick): {t / 1e3:.3f} ms "
                      f"[{tlo / 1e3:.3f} .. {thi / 1e3:.3f}] = {B / t * 1e6:.0f} img/s")
                del tm, x
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
