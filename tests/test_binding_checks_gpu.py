"""Every binding rejects malformed operands before it launches anything.

Table-driven: each entry of CASES builds one minimal valid call of a binding of
``idunno._C``.  The call is made once (it must be accepted), then one operand at
a time is mutated -- a CPU tensor, a wrong dtype, a non-contiguous tensor, a
wrong rank, each documented shape mismatch, a bad ``out`` / residual -- and the
binding must raise RuntimeError.  Rejections launch nothing.

Operand flags: "R" the binding bounds the operand's numel, not its rank (a
reshaped tensor is the same memory: no rank mutation); "C" a one-element
tensor (always contiguous: no stride mutation).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H16, F32, U8, I32, I64 = torch.float16, torch.float32, torch.uint8, torch.int32, torch.int64
WRONG = {H16: F32, F32: H16, U8: torch.int8, I64: I32, I32: I64, torch.int16: I32}


def z(*shape, dt=H16):
    return torch.zeros(shape, dtype=dt, device=DEV)


class Call:
    def __init__(self, fn, kw, operands, shapes, extra=(), wrong=None, cleanup=None, pos=()):
        self.fn, self.kw, self.operands, self.shapes = fn, kw, operands, shapes
        self.pos = pos                    # arguments of a binding without keyword names, in order
        self.extra = list(extra)          # (label, keyword overrides) that must be rejected too
        self.wrong = wrong or {}          # operand -> wrong dtype, where the default one is also accepted
        self.cleanup = cleanup

    def run(self, **over):
        try:
            kw = {**self.kw, **over}
            return self.fn(*[kw.pop(n) for n in self.pos], **kw)
        finally:
            if self.cleanup:
                self.cleanup()


def grow(t, d):
    shape = list(t.shape)
    shape[d] += 1
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def mutations(c, other_device=None):
    """(label, keyword overrides) per operand; with other_device only the move to that device."""
    for name, flags in c.operands.items():
        t = c.kw[name]
        if other_device is not None:
            yield f"{name} on {other_device}", {name: t.to(other_device)}
            continue
        yield f"{name} on the CPU", {name: t.cpu()}
        yield f"{name} wrong dtype", {name: t.to(c.wrong.get(name, WRONG[t.dtype]))}
        if "C" not in flags:
            yield f"{name} non-contiguous", {name: torch.stack([t, t], -1)[..., 0]}
        if "R" not in flags:
            yield f"{name} wrong rank", {name: t.unsqueeze(0)}
    if other_device is None:
        for name, d in c.shapes:
            yield f"{name} dim {d} + 1", {name: grow(c.kw[name], d)}
        yield from c.extra


def all_dims(name, rank):
    return [(name, d) for d in range(rank)]


# ---- the table: name -> builder(ext) -> Call ---------------------------------------------------
def _conv(fn_name, dt, cin, k, **more):
    """64 -> 64 channels at [1, 8, 8]: cin = 64, or 2C = 128 halfs a pixel for the split layout (in and out)."""
    def build(ext):
        kw = dict(x=z(1, 8, 8, cin, dt=dt), w=z(64, k * k * cin, dt=dt), bias=z(64, dt=F32),
                  res=z(1, 8, 8, cin, dt=dt), KH=k, KW=k, stride=1, pad=k // 2, relu=True,
                  out=z(1, 8, 8, cin, dt=dt), **more)
        ops = dict(x="", w="", bias="", res="", out="")
        shapes = [("x", 1), ("x", 3), ("w", 0), ("w", 1), ("bias", 0)] + all_dims("res", 4) + all_dims("out", 4)
        return Call(getattr(ext, fn_name), kw, ops, shapes, extra=[("stride 0", dict(stride=0))])
    return build


def _first_ok(pred, ranges):
    """Smallest argument tuple (by sum, then lexicographic) the binding's own predicate accepts."""
    for args in sorted(itertools.product(*ranges), key=lambda a: (sum(a), a)):
        if pred(*args, 64):
            return args
    raise AssertionError("the predicate accepts no shape in range")


def _dual(split):
    def build(ext):
        c64 = range(64, 513, 64)
        K1, K2, Cout = _first_ok(ext.conv1x1_dual_split_ok if split else ext.conv1x1_dual_ok, (c64, c64, c64))
        m = 2 if split else 1
        kw = dict(x1=z(1, 8, 8, m * K1), x2=z(1, 8, 8, m * K2), w=z(Cout, m * (K1 + K2)), bias=z(Cout, dt=F32),
                  stride=1, relu=True)
        if split:
            kw["acc_scale"] = 1.0
        shapes = all_dims("x1", 4) + all_dims("x2", 4) + [("w", 0), ("w", 1), ("bias", 0)]
        return Call(ext.conv1x1_dual_split if split else ext.conv1x1_dual, kw, dict(x1="", x2="", w="", bias=""),
                    shapes, extra=[("stride 0", dict(stride=0)), ("stride 2", dict(stride=2))])
    return build


def _fused_next(dual):
    def build(ext):
        c64 = range(64, 513, 64)
        K1, K2, N, N2 = _first_ok(ext.conv1x1_fused_next_ok, (c64, c64 if dual else (0,), c64, c64))
        kw = dict(x1=z(1, 8, 8, K1), x2=z(1, 8, 8, K2) if dual else None, w=z(N, K1 + K2), bias=z(N, dt=F32),
                  res=None if dual else z(1, 8, 8, N), w2=z(N2, N), b2=z(N2, dt=F32), stride=1, relu=True)
        other = "x2" if dual else "res"
        shapes = all_dims("x1", 4) + all_dims(other, 4) + [("w", 0), ("w", 1), ("bias", 0), ("w2", 0), ("w2", 1),
                                                            ("b2", 0)]
        extra = [("residual next to x2", dict(res=z(1, 8, 8, N)))] if dual else []
        return Call(ext.conv1x1_fused_next, kw, {"x1": "", other: "", "w": "", "bias": "R", "w2": "", "b2": "R"},
                    shapes, extra)
    return build


def _split_dual(ext):
    kw = dict(x=z(1, 8, 8, 128), w=z(256, 9 * 128), bias=z(256, dt=F32), KH=3, KW=3, stride=2, pad=1, relu=True,
              acc_scale=1.0, acc_scale2=1.0, nsplit=128, center_only=True, tile=36)
    return Call(ext.conv2d_split_dual, kw, dict(x="", w="", bias=""), [("x", 3), ("w", 0), ("w", 1), ("bias", 0)],
                extra=[("nsplit 0", dict(nsplit=0)), ("nsplit 48", dict(nsplit=48)), ("nsplit = Cout", dict(nsplit=256))])


def _split_tail(ext):
    kw = dict(y=z(1, 7, 7, 256), x2=z(1, 14, 14, 128), w=z(128, 9 * 256 + 128), bias=z(128, dt=F32), acc_scale=1.0,
              stride2=2, relu=True)
    return Call(ext.conv2d_split_tail, kw, dict(y="", x2="", w="", bias=""),
                all_dims("y", 4) + all_dims("x2", 4) + [("w", 0), ("w", 1), ("bias", 0)],
                extra=[("stride2 1", dict(stride2=1)), ("a tile without a K tail", dict(tile=27))])


def _band(split):
    def build(ext):
        m = 2 if split else 1
        kw = dict(x=z(1, 7, 7, m * 64), w=z(128, 9 * m * 64), bias=z(128, dt=F32), res=z(1, 7, 7, m * 128), relu=True)
        shapes = [("x", 1), ("x", 3), ("w", 0), ("w", 1), ("bias", 0)] + all_dims("res", 4)
        return Call(ext.conv3x3_band_split if split else ext.conv3x3_band_f16, kw, dict(x="", w="", bias="R", res=""),
                    shapes)
    return build


def _linear(fn_name, dt, kmul, split):
    def build(ext):
        K, N = 2 * kmul, 64                 # two slices of the smallest K slice the split rule allows
        kw = dict(x=z(4, K, dt=dt), w=z(N, K, dt=dt), bias=z(N, dt=F32), relu=True, splits=2)
        if fn_name != "linear_f32_splitk":
            kw["out_f32"] = False
        if split:
            kw["acc_scale"] = 1.0
        return Call(getattr(ext, fn_name), kw, dict(x="", w="", bias=""), [("x", 1), ("w", 0), ("w", 1), ("bias", 0)],
                    extra=[("splits 0", dict(splits=0)), ("splits that do not divide K", dict(splits=4))])
    return build


def _exact_stem(fn_name, hw, wk, ps, form):
    def build(ext):
        kw = dict(img=z(2, *hw, 3, dt=U8), w=z(2, 64, wk * 32), bias=z(64, dt=F32), psum=z(ps, ps, 64, dt=F32),
                  acc_scale=1.0, start=z(1, dt=I64), batch=1)
        extra = [("batch beyond the shard", dict(batch=3)), ("window part out of range", dict(sub=1)),
                 ("image smaller than the kernel", dict(img=z(2, 5, 5, 3, dt=U8)))]
        if form:
            extra += [("form 2", dict(form=2)), ("form -2", dict(form=-2))]
        shapes = [("img", 3), ("w", 0), ("w", 1), ("w", 2), ("bias", 0), ("psum", 0), ("start", 0)]
        return Call(getattr(ext, fn_name), kw, dict(img="", w="", bias="R", psum="R", start="RC"), shapes, extra)
    return build


def _stem_fused(ext):
    kw = dict(img=z(2, 37, 37, 3, dt=U8), w=z(64, 7 * 32), bias=z(64, dt=F32), start=z(1, dt=I64), batch=1)
    return Call(ext.stem_fused, kw, dict(img="", w="", bias="R", start="RC"),
                [("img", 3), ("w", 0), ("w", 1), ("bias", 0), ("start", 0)],
                extra=[("batch beyond the shard", dict(batch=3)), ("image smaller than the kernel",
                                                                     dict(img=z(2, 5, 5, 3, dt=U8)))])


def _image(fn_name, **more):
    def build(ext):
        kw = dict(img=z(2, 16, 16, 3, dt=U8), start=z(1, dt=I64), batch=1, **more)
        extra = [("batch beyond the shard", dict(batch=3))]
        if "KW" in more:
            extra.append(("KW below 5", dict(KW=3)))
        return Call(getattr(ext, fn_name), kw, dict(img="", start="RC"), [("img", 3), ("start", 0)], extra)
    return build


def _resize_crop(ext):
    return Call(ext.resize_crop, dict(img=z(1, 16, 16, 3, dt=U8), resize=8, crop=8), dict(img=""), [("img", 3)],
                extra=[("crop larger than the resized image", dict(crop=9))], pos=("img", "resize", "crop"))


def _pack3(split):
    def build(ext):
        KH = KW = 11
        img = z(1, 31, 23, 3, dt=U8)
        if split:
            x3 = ext.preprocess_pack3_split(img, KW, 4, 2)
            kpad = (KH * ((3 * KW + 7) // 8) + 3) // 4 * 64
            kw = dict(x3=x3, w=z(64, kpad), acc_scale=1.0)
        else:
            x3 = ext.preprocess_pack3(img, KW, 4, 2)
            kpad = (KH * ((3 * KW + 3) // 4) + 3) // 4 * 16
            kw = dict(x3=x3, w=z(64, kpad, dt=F32))
        kw.update(bias=z(64, dt=F32), W=23, KH=KH, KW=KW, stride=4, pad=2, relu=True)
        return Call(ext.conv2d_pack3_split if split else ext.conv2d_pack3, kw, dict(x3="", w="", bias=""),
                    [("x3", 2), ("x3", 3), ("w", 0), ("w", 1), ("bias", 0)], extra=[("another width", dict(W=24))])
    return build


def _wino(ext):
    hw = next(h for h in range(8, 57, 2) if ext.wino_supported(h, h, 64, 64))
    kw = dict(x=z(1, hw, hw, 64, dt=F32), u=z(16, 64, 64, dt=F32), bias=z(64, dt=F32), res=z(1, hw, hw, 64, dt=F32),
              relu=True)
    return Call(ext.conv2d_wino_f32, kw, dict(x="", u="", bias="", res=""),
                [("x", 3), ("u", 0), ("u", 1), ("u", 2), ("bias", 0)] + all_dims("res", 4))


def _maxpool(ext):
    kw = dict(x=z(1, 8, 8, 64), k=3, s=2, pad=1, out=z(1, 4, 4, 64))
    return Call(ext.maxpool2d_nhwc, kw, dict(x="", out=""), [("x", 1), ("x", 3)] + all_dims("out", 4),
                extra=[("pad above k / 2", dict(pad=2))])


def _maxpool_split(ext):
    kw = dict(x=z(1, 8, 8, 64, dt=F32), k=3, s=2, pad=1, out=z(1, 4, 4, 128))
    return Call(ext.maxpool2d_split, kw, dict(x="", out=""), [("x", 1), ("x", 3)] + all_dims("out", 4))


def _softmax(ext):
    kw = dict(logits=z(4, 16, dt=F32), packed=z(4, 2, dt=I32), ovf=z(1, dt=I32))
    return Call(ext.softmax_top1, kw, dict(logits="", packed="", ovf="RC"), [("packed", 1)],
                extra=[("packed shorter than the rows", dict(packed=z(3, 2, dt=I32)))])


def _split_guard(ext):
    return Call(ext.set_split_guard, dict(flag=z(1, dt=I32)), dict(flag="RC"), [],
                cleanup=lambda: ext.set_split_guard(None))


def _one(fn_name, shape, dt, shapes, flags="R", wrong=None):
    return lambda ext: Call(getattr(ext, fn_name), dict(x=z(*shape, dt=dt)), dict(x=flags), shapes, wrong=wrong,
                            pos=("x",))


CASES = {
    "conv2d_nhwc-1x1": _conv("conv2d_nhwc", H16, 64, 1),
    "conv2d_nhwc-3x3": _conv("conv2d_nhwc", H16, 64, 3),
    "conv2d_nhwc_f32-1x1": _conv("conv2d_nhwc_f32", F32, 64, 1),
    "conv2d_nhwc_f32-3x3": _conv("conv2d_nhwc_f32", F32, 64, 3),
    "conv2d_split-1x1": _conv("conv2d_split", H16, 128, 1, acc_scale=1.0),
    "conv2d_split-3x3": _conv("conv2d_split", H16, 128, 3, acc_scale=1.0),
    "conv2d_split_dual": _split_dual,
    "conv2d_split_tail": _split_tail,
    "conv1x1_dual": _dual(False),
    "conv1x1_dual_split": _dual(True),
    "conv1x1_fused_next-res": _fused_next(False),
    "conv1x1_fused_next-dual": _fused_next(True),
    "conv3x3_band_f16": _band(False),
    "conv3x3_band_split": _band(True),
    "linear_splitk": _linear("linear_splitk", H16, 64, False),
    "linear_split": _linear("linear_split", H16, 64, True),
    "linear_f32_splitk": _linear("linear_f32_splitk", F32, 16, False),
    "conv2d_wino_f32": _wino,
    "conv2d_pack3": _pack3(False),
    "conv2d_pack3_split": _pack3(True),
    "alex_stem_split": _exact_stem("alex_stem_split", (31, 23), 17, 12, True),
    "alex_stem_u8_f16": _exact_stem("alex_stem_u8_f16", (31, 23), 17, 12, True),
    "stem_split": _exact_stem("stem_split", (37, 37), 7, 8, False),
    "stem_u8_f16": _exact_stem("stem_u8_f16", (37, 37), 7, 8, False),
    "stem_fused": _stem_fused,
    "preprocess": _image("preprocess"),
    "preprocess_pack3": _image("preprocess_pack3", KW=7, stride=2, pad=3),
    "preprocess_pack3_split": _image("preprocess_pack3_split", KW=7, stride=2, pad=3),
    "resize_crop": _resize_crop,
    "maxpool2d_nhwc": _maxpool,
    "maxpool2d_split": _maxpool_split,
    "global_avgpool_nhwc": _one("global_avgpool_nhwc", (1, 8, 8, 64), H16, [("x", 3)], flags="",
                                wrong={"x": torch.float64}),
    "softmax_top1": _softmax,
    "split_from_f32": _one("split_from_f32", (1, 8, 8, 64), F32, [("x", 3)]),
    "f32_from_split": _one("f32_from_split", (1, 8, 8, 128), H16, [("x", 3)]),
    "jpeg_entropy_zero": _one("jpeg_entropy_zero", (128,), torch.int16, []),
    "set_split_guard": _split_guard,
}


@pytest.fixture(scope="module")
def ext():
    from idunno import ops

    return ops.load()


def _accepted(c, over):
    try:
        c.run(**over)
    except RuntimeError:
        return False
    return True


@pytest.mark.parametrize("name", list(CASES))
def test_binding_accepts_valid_and_rejects_malformed(ext, name):
    c = CASES[name](ext)
    c.run()                               # the minimal valid call is accepted
    torch.cuda.synchronize()
    wrongly = [label for label, over in mutations(c) if _accepted(c, over)]
    assert not wrongly, f"{name} accepted: {wrongly}"


def test_binding_rejects_operands_on_another_device(ext):
    """Every operand of every binding, moved to device 1 in turn (this includes the w / bias /
    res of conv2d_nhwc, every operand of conv1x1_fused_next, and the w / bias of stem_fused and
    linear_splitk, which used to go unchecked)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs to put an operand on another device")
    wrongly = []
    for name, build in CASES.items():
        c = build(ext)
        if len(c.operands) < 2:           # a lone operand has no other to disagree with (and "must be on the
            continue                      # current device" is not a rule of the bindings)
        wrongly += [f"{name}: {label}" for label, over in mutations(c, "cuda:1") if _accepted(c, over)]
    assert not wrongly, wrongly
