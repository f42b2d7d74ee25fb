#!/usr/bin/env python3
"""MobileNetV2 on the depthwise / narrow 1x1 kernels: per-layer bytes, time and GB/s, the
whole forward (hipGraph replay) in img/s, and for information torch's own eager forward of
the reference module on the same card in the same process.  Both precisions.

usage: python tools/bench_mobilenet.py [--batch 400] [--iters 20]
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
    """(name, bytes moved, call) per launch of the forward after the stem, on real activations."""
    out = []
    for i, mb in enumerate(prog.mblocks):
        y = x
        if mb.expand is not None:
            c, xin = mb.expand, y
            y = o.conv1x1_narrow(xin, c.w, c.b, c.act)
            out.append((f"b{i + 1} expand {c.cin}->{c.cout} @{xin.shape[1]}", xin.nbytes + y.nbytes + c.w.nbytes,
                        lambda c=c, xin=xin: o.conv1x1_narrow(xin, c.w, c.b, c.act)))
        c, xin = mb.dw, y
        y = o.conv3x3_dw(xin, c.w, c.b, c.stride, c.act, clamp_in=i == 0)
        out.append((f"b{i + 1} dw {c.cin} s{c.stride} @{xin.shape[1]}", xin.nbytes + y.nbytes + c.w.nbytes,
                    lambda c=c, xin=xin, i=i: o.conv3x3_dw(xin, c.w, c.b, c.stride, c.act, clamp_in=i == 0)))
        c, xin, res = mb.project, y, x if mb.residual else None
        x = o.conv1x1_narrow(xin, c.w, c.b, c.act, residual=res)
        out.append((f"b{i + 1} project {c.cin}->{c.cout} @{xin.shape[1]}" + (" +res" if res is not None else ""),
                    xin.nbytes + x.nbytes * (2 if res is not None else 1) + c.w.nbytes,
                    lambda c=c, xin=xin, res=res: o.conv1x1_narrow(xin, c.w, c.b, c.act, residual=res)))
    c = prog.last
    out.append((f"last {c.cin}->{c.cout} @{x.shape[1]}", x.nbytes + x.nbytes // c.cin * c.cout + c.w.nbytes,
                lambda c=c, x=x: o.conv1x1_narrow(x, c.w, c.b, c.act)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from idunno import ops as o
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    o.load()
    dev, B = "cuda", a.batch
    m = ref.build("mobilenet_v2", seed=7, randomize_bn=True)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev)
    small = img[:3].cpu()
    with torch.no_grad():
        r64 = m.double()(ref.preprocess_u8(small).double())
    m.float()
    print(f"device {torch.cuda.get_device_name(0)}, batch {B}, {a.iters} timed calls per figure")
    for dtype, tdt in (("fp16", torch.float16), ("fp32", torch.float32)):
        prog = compile_model(m, "mobilenet_v2", dtype=dtype)
        runner = HipRunner(prog)
        p, s = runner.p, runner.p.stem
        x = o.conv2d(o.preprocess(img, f32=dtype == "fp32"), s.w, s.b, s.kh, s.kw, s.stride, s.pad, True)
        print(f"\n## {dtype}: per launch at B = {B}\n\n| layer | MB moved | us | GB/s |\n|---|---:|---:|---:|")
        tot_us = tot_b = 0.0
        for name, nbytes, fn in layers(p, o, x):
            us = timeit(fn, a.iters)
            tot_us, tot_b = tot_us + us, tot_b + nbytes
            print(f"| {name} | {nbytes / 1e6:.1f} | {us:.1f} | {nbytes / us / 1e3:.0f} |")
        print(f"| sum | {tot_b / 1e6:.1f} | {tot_us:.1f} | {tot_b / tot_us / 1e3:.0f} |")
        del x
        sin, replay = runner.capture(B)
        sin.copy_(img)
        us = timeit(replay, a.iters)
        print(f"\n{dtype} whole forward, hipGraph replay: {us / 1e3:.3f} ms = {B / us * 1e6:.0f} img/s")
        us = timeit(lambda: runner.forward(img), a.iters)
        print(f"{dtype} whole forward, eager launches: {us / 1e3:.3f} ms = {B / us * 1e6:.0f} img/s")
        # information only: torch's eager forward of the reference module (channels_last, MIOpen)
        mt = ref.build("mobilenet_v2", seed=7, randomize_bn=True).to(dev, tdt).to(memory_format=torch.channels_last)
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
