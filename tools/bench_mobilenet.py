#!/usr/bin/env python3
"""MobileNetV2 / V3 on the depthwise / narrow 1x1 / SE kernels: per-layer bytes, time and
GB/s, the whole forward (hipGraph replay and eager) in img/s, and for information torch's
own eager forward of the reference module on the same card in the same process.  Both
precisions.  For MobileNetV3 also the two same-process A/Bs of its SE layers: the squeeze
fused into the depthwise launch against depthwise + global_avgpool, and the one-launch SE
gate against two narrow 1x1 launches.

usage: python tools/bench_mobilenet.py [--model mobilenet_v2] [--batch 400] [--iters 20]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters):
    """us per call from device events, after two warm-up calls."""
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    fn()
    torch.cuda.synchronize()
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) * 1000 / iters


def layers(prog, o, x):
    """(name, bytes moved, call) per launch of the forward after the stem, on real activations,
    and per SE layer (name, fused-squeeze arm, unfused arm, one-launch gate arm, two-launch arm)."""
    out, se = [], []
    v3 = prog.kind == "mobilenet_v3"
    for i, mb in enumerate(prog.mblocks):
        y, scale = x, None
        if mb.expand is not None:
            c, xin = mb.expand, y
            y = o.conv1x1_narrow(xin, c.w, c.b, c.act)
            out.append((f"b{i + 1} expand {c.cin}->{c.cout} @{xin.shape[1]}", xin.nbytes + y.nbytes + c.w.nbytes,
                        lambda c=c, xin=xin: o.conv1x1_narrow(xin, c.w, c.b, c.act)))
        c, xin = mb.dw, y
        if not v3:
            y = o.conv3x3_dw(xin, c.w, c.b, c.stride, c.act, clamp_in=i == 0)
            fn = lambda c=c, xin=xin, i=i: o.conv3x3_dw(xin, c.w, c.b, c.stride, c.act, clamp_in=i == 0)
        else:
            ain = 3 if i == 0 else 0
            mean = torch.empty(xin.shape[0], c.cout, dtype=xin.dtype, device=xin.device) if mb.se else None
            y = o.conv_dw(xin, c.w, c.b, c.kh, c.stride, c.act, act_in=ain, pool=mean)
            fn = lambda c=c, xin=xin, ain=ain, mean=mean: o.conv_dw(xin, c.w, c.b, c.kh, c.stride, c.act, act_in=ain,
                                                                    pool=mean)
        out.append((f"b{i + 1} dw{c.kh} {c.cin} s{c.stride} @{xin.shape[1]}" + (" +squeeze" if mb.se else ""),
                    xin.nbytes + y.nbytes + c.w.nbytes, fn))
        if mb.se:
            f1, f2 = mb.se
            scale = o.se_excite(mean, f1.w, f1.b, f2.w, f2.b)
            gate = lambda f1=f1, f2=f2, mean=mean: o.se_excite(mean, f1.w, f1.b, f2.w, f2.b)
            out.append((f"b{i + 1} se {f1.cin}->{f1.cout}->{f2.cout}", mean.nbytes * 2 + f1.w.nbytes + f2.w.nbytes, gate))

            def unfused(c=c, xin=xin, ain=ain):
                return o.global_avgpool(o.conv_dw(xin, c.w, c.b, c.kh, c.stride, c.act, act_in=ain))

            def two(f1=f1, f2=f2, mean=mean):
                h = o.conv1x1_narrow(mean.view(-1, 1, 1, f1.cin), f1.w, f1.b, f1.act)
                return o.conv1x1_narrow(h, f2.w, f2.b, f2.act)

            se.append((f"b{i + 1} {c.cin} k{c.kh} s{c.stride} @{xin.shape[1]}", fn, unfused, gate, two))
        c, xin, res = mb.project, y, x if mb.residual else None
        kw = dict(in_scale=scale, res_act=3 if i == 0 and res is not None else 0) if v3 else {}
        x = o.conv1x1_narrow(xin, c.w, c.b, c.act, residual=res, **kw)
        out.append((f"b{i + 1} project {c.cin}->{c.cout} @{xin.shape[1]}" + (" +res" if res is not None else "") +
                    (" *gate" if scale is not None else ""),
                    xin.nbytes + x.nbytes * (2 if res is not None else 1) + c.w.nbytes,
                    lambda c=c, xin=xin, res=res, kw=kw: o.conv1x1_narrow(xin, c.w, c.b, c.act, residual=res, **kw)))
    c = prog.last
    out.append((f"last {c.cin}->{c.cout} @{x.shape[1]}", x.nbytes + x.nbytes // c.cin * c.cout + c.w.nbytes,
                lambda c=c, x=x: o.conv1x1_narrow(x, c.w, c.b, c.act)))
    return out, se


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mobilenet_v2")
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from idunno import ops as o
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    o.load()
    dev, B, name = "cuda", a.batch, ref.canonical(a.model)
    m = ref.build(name, seed=7, randomize_bn=True)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    small = img[:3].cpu()
    with torch.no_grad():
        r64 = m.double()(ref.preprocess_u8(small).double())
    m.float()
    print(f"{name}: device {torch.cuda.get_device_name(0)}, batch {B}, {a.iters} timed calls per figure")
    for dtype, tdt in (("fp16", torch.float16), ("fp32", torch.float32)):
        prog = compile_model(m, name, dtype=dtype)
        runner = HipRunner(prog)
        p, s = runner.p, runner.p.stem
        x = o.conv2d(o.preprocess(img, f32=dtype == "fp32"), s.w, s.b, s.kh, s.kw, s.stride, s.pad, p.kind == "mobilenet")
        print(f"\n## {name} {dtype}: per launch at B = {B}\n\n| layer | MB moved | us | GB/s |\n|---|---:|---:|---:|")
        tot_us = tot_b = 0.0
        per_launch, se = layers(p, o, x)
        for lname, nbytes, fn in per_launch:
            us = timeit(fn, a.iters)
            tot_us, tot_b = tot_us + us, tot_b + nbytes
            print(f"| {lname} | {nbytes / 1e6:.1f} | {us:.1f} | {nbytes / us / 1e3:.0f} |")
        print(f"| sum | {tot_b / 1e6:.1f} | {tot_us:.1f} | {tot_b / tot_us / 1e3:.0f} |")
        if se:
            print(f"\n## {name} {dtype}: SE A/Bs at B = {B} (us)\n\n| SE layer | dw+squeeze | dw, avgpool | se_excite | "
                  "two narrow 1x1 |\n|---|---:|---:|---:|---:|")
            sums = [0.0] * 4
            for lname, *arms in se:
                us = [timeit(fn, a.iters) for fn in arms]
                sums = [t + u for t, u in zip(sums, us)]
                print(f"| {lname} | " + " | ".join(f"{u:.1f}" for u in us) + " |")
            print("| sum | " + " | ".join(f"{u:.1f}" for u in sums) + " |")
        del x, per_launch, se
        sin, replay = runner.capture(B)
        sin.copy_(img)
        us = timeit(replay, a.iters)
        print(f"\n{dtype} whole forward, hipGraph replay: {us / 1e3:.3f} ms = {B / us * 1e6:.0f} img/s")
        us = timeit(lambda: runner.forward(img), a.iters)
        print(f"{dtype} whole forward, eager launches: {us / 1e3:.3f} ms = {B / us * 1e6:.0f} img/s")
        # information only: torch's eager forward of the reference module (channels_last, MIOpen)
        mt = ref.build(name, seed=7, randomize_bn=True).to(dev, tdt).to(memory_format=torch.channels_last)
        xt = ref.preprocess_u8(img).to(tdt).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            t0 = time.time()
            us = timeit(lambda: mt(xt), a.iters)
            print(f"{dtype} torch eager forward of the reference module: {us / 1e3:.3f} ms = {B / us * 1e6:.0f} img/s "
                  f"(timed in {time.time() - t0:.1f} s)")
            et = (mt(xt[:3]).double().cpu() - r64).abs().max().item()
        eh = (runner.logits(img[:3]).double().cpu() - r64).abs().max().item()
        print(f"{dtype} logit error vs the fp64 module at B = 3 (logit scale {r64.abs().max().item():.3e}): "
              f"HIP {eh:.3e}, torch {et:.3e}")
        runner.close()


if __name__ == "__main__":
    main()
