"""Inference programs: reference modules -> BN-folded, MFMA-packed op lists.

``compile_model(module)`` turns an eval-mode ResNet / AlexNet into a flat list
of ops whose weights are laid out for the gfx950 implicit-GEMM kernel:

  * BatchNorm folded into the preceding conv: w' = w * g/sqrt(v+eps),
    b' = beta - mean * g/sqrt(v+eps)  ("BN folded into conv
    weights/bias at load time")
  * conv weights [Cout, Cin, KH, KW] -> [Cout, KH, KW, Cin] fp16 (K contiguous)
  * RGB stems (Cin = 3) -> [Cout, KH, ceil(KW/8)*8, 4] (one K-stage per kh row;
    fp32 programs: ceil(KW/4)*4 taps)
  * fp32 programs (dtype "fp32", the reference's precision) keep fp32 weights;
    their 3x3/stride-1 convs also carry the Winograd F(2x2,3x3) filter
    transform U = G g G^T [16, Cout, Cin] (conv_wino_f32.hip)
  * grouped 3x3 convs (ResNeXt) -> channel-block-local [Cout, 9 * CB] weights
    (pack_grouped_weight / pack_grouped_split_weight), never a dense expansion
  * AlexNet fc6 columns permuted from NCHW-flatten to NHWC-flatten order
  * dropout elided (identity in eval), AdaptiveAvgPool(6,6) elided at 224 input

The same program runs on two executors: ``runner.HipRunner`` (the real path,
HIP kernels, fp16 activations / fp32 accumulation, or all-fp32 for dtype
"fp32") and ``emulate`` (fp32 torch
re-execution of the *packed* weights — used on CPU to test folding/packing
without a GPU).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, fields, replace

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import reference as ref


@dataclass
class Conv:
    w: torch.Tensor          # packed [Cout, Kpad] fp16 (fp32 for dtype "fp32" programs)
    b: torch.Tensor          # [Cout] fp32
    cin: int
    cout: int
    kh: int
    kw: int
    stride: int
    pad: int
    relu: bool
    small: bool = False      # RGB stem packing
    wino: torch.Tensor | None = None   # fp32 3x3/s1: Winograd U = G g G^T [16, Cout, Cin]
    p3: torch.Tensor | None = None     # RGB stem on packed rows (pack_conv_weight_p3)
    sw: torch.Tensor | None = None     # fp32 programs: split-fp16 weights (pack_split_weight)
    s_scale: float = 1.0               # accumulator scale of ``sw`` / ``sp3`` (2^-e)
    sp3: torch.Tensor | None = None    # fp32 RGB stems: split-fp16 packed-row weights (pack_split_weight_p3)
    fs: torch.Tensor | None = None     # fp32 ResNet 7x7/2 stem: fused split stem weights (pack_stem_split)
    fs_bias: torch.Tensor | None = None  # ... its bias (with the normalisation shift folded in)
    fs_psum: torch.Tensor | None = None  # ... its border-correction prefix sums [8, 8, 64]
    fs_scale: float = 1.0              # ... its accumulator scale 2^-e
    # grouped 3x3 conv (ResNeXt): ``w`` is the block-local fp16 form (pack_grouped_weight) in fp16
    # programs and the plain fp32 [Cout, Cin/groups, 3, 3] weight in fp32 programs, whose ``sw`` is
    # the block-local split form (pack_grouped_split_weight); cin / cout stay the full widths
    groups: int = 1

    def to(self, device):
        vals = {f.name: getattr(self, f.name) for f in fields(self)}
        return replace(self, **{k: v.to(device) for k, v in vals.items() if isinstance(v, torch.Tensor)})

    @property
    def flops_per_out_pixel(self) -> int:
        return 2 * self.cin * self.kh * self.kw * self.cout // self.groups


@dataclass
class Block:
    """Residual block: convs in order; the last conv fuses +identity and ReLU."""
    convs: list
    down: Conv | None = None

    def to(self, device):
        return replace(self, convs=[c.to(device) for c in self.convs], down=self.down.to(device) if self.down else None)


@dataclass
class Program:
    name: str
    kind: str                 # "resnet" | "alexnet"
    stem: Conv | None = None  # resnet
    blocks: list = field(default_factory=list)
    features: list = field(default_factory=list)  # alexnet: ("conv", Conv) | ("pool", (k, s, p))
    fcs: list = field(default_factory=list)       # list[Conv] as 1x1 convs (last -> fp32 logits)
    num_classes: int = 1000
    dtype: str = "fp16"       # activation / weight precision: "fp16" | "fp32" (reference precision)

    def to(self, device):
        return replace(self, stem=self.stem.to(device) if self.stem else None,
                       blocks=[b.to(device) for b in self.blocks],
                       features=[(k, v.to(device) if k == "conv" else v) for k, v in self.features],
                       fcs=[f.to(device) for f in self.fcs])

    def param_bytes(self) -> int:
        tot = 0
        for c in self.all_convs():
            tot += c.w.numel() * c.w.element_size() + c.b.numel() * 4
        return tot

    def all_convs(self):
        if self.stem is not None:
            yield self.stem
        for b in self.blocks:
            yield from b.convs
            if b.down is not None:
                yield b.down
        for k, v in self.features:
            if k == "conv":
                yield v
        yield from self.fcs


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------

def fold_bn_f64(w: torch.Tensor, b: torch.Tensor | None, bn: nn.BatchNorm2d | None):
    """Fold an eval-mode BatchNorm into the preceding conv's (w, b), fp64 result."""
    w = w.detach().double()
    b = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.detach().double()
    if bn is None:
        return w, b
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = w * scale.view(-1, 1, 1, 1)
    b = (b - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
    return w, b


def fold_bn(w: torch.Tensor, b: torch.Tensor | None, bn: nn.BatchNorm2d | None):
    """Fold an eval-mode BatchNorm into the preceding conv's (w, b), in fp64."""
    w, b = fold_bn_f64(w, b, bn)
    return w.float(), b.float()


DTYPES = ("fp16", "fp32")


def pack_conv_weight(w: torch.Tensor, dtype: str = "fp16") -> tuple[torch.Tensor, bool]:
    """[Cout, Cin, KH, KW] fp32 -> packed [Cout, Kpad], small flag.

    fp16: small (Cin <= 4) rows are 8 taps x 4 channels (K stage of the f16
    kernels); big rows (kh, kw, c) with Cin % 64 == 0.
    fp32: small rows are 4 taps x 4 channels (one BK=16 stage of conv_f32.hip);
    big rows (kh, kw, c) with Cin % 16 == 0."""
    cout, cin, kh, kw = w.shape
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
    taps, mult, dt = (4, 16, torch.float32) if dtype == "fp32" else (8, 64, torch.float16)
    if cin <= 4:
        nsub = (kw + taps - 1) // taps
        p = torch.zeros(cout, kh, nsub * taps, 4, dtype=torch.float32)
        p[:, :, :kw, :cin] = w.permute(0, 2, 3, 1)
        return p.reshape(cout, kh * nsub * taps * 4).to(dt).contiguous(), True
    if cin % mult != 0:
        raise ValueError(f"Cin={cin} unsupported (need 3/4 or a multiple of {mult})")
    return w.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).to(dt).contiguous(), False


def _p3_rows(w: torch.Tensor, e: int, stage: int, dtype: torch.dtype) -> torch.Tensor:
    """[Cout, 3, KH, KW] -> [Cout, K] rows in ``dtype``: K = (kh, f) with
    f = 3*kw + c over cpk = ceil(3*KW/e) chunks of e elements per kernel row
    (f >= 3*KW: zero), zero-padded to whole stages of ``stage`` elements."""
    cout, cin, kh, kw = w.shape
    if cin != 3 or kw < 5:
        raise ValueError("packed-row stems take 3 input channels and KW >= 5")
    cpk = (3 * kw + e - 1) // e
    k = kh * cpk * e
    rows = torch.zeros(cout, kh, e * cpk, dtype=dtype)
    rows[:, :, :3 * kw] = w.to(dtype).permute(0, 2, 3, 1).reshape(cout, kh, 3 * kw)
    flat = torch.zeros(cout, -(-k // stage) * stage, dtype=dtype)
    flat[:, :k] = rows.reshape(cout, -1)
    return flat


def pack_conv_weight_p3(w: torch.Tensor, dtype: str = "fp32") -> torch.Tensor:
    """[Cout, 3, KH, KW] -> packed-row stem weights: K = (kh, f) with
    f = 3*kw + c over cpk = ceil(3*KW/E) 16-byte chunks per kernel row
    (E = 4 fp32 / 8 fp16 elements; f >= 3*KW: zero), the order in which
    preprocess_pack3 lays a kernel row's pixels out; padded to whole K stages
    (16 fp32 = conv_f32.hip mode 2, 64 fp16 = conv_glds pack3)."""
    e, stage = (4, 16) if dtype == "fp32" else (8, 64)
    p = _p3_rows(w, e, stage, torch.float32)
    return p.contiguous() if dtype == "fp32" else p.half().contiguous()


def pack3_eligible(cin: int, kw: int, stride: int = 2, dtype: str = "fp32") -> bool:
    """fp32: any stride (<= 4 row copies); fp16 (8 halfs per chunk): stride
    even (2 or 4 row copies)."""
    return cin == 3 and kw >= 5 and (dtype == "fp32" or stride % 2 == 0)


def unpack_conv_weight(c: Conv) -> torch.Tensor:
    """Inverse of pack_conv_weight -> fp32 [Cout, Cin, KH, KW] (a grouped conv:
    [Cout, Cin / groups, 3, 3], its fp32 copy in fp32 programs)."""
    if c.groups > 1:
        return c.w.float().contiguous() if c.w.dim() == 4 else unpack_grouped_weight(c)
    w = c.w.float()
    if c.small:
        tpr = 4 if c.w.dtype == torch.float32 else 8        # taps per K row (see pack_conv_weight)
        nsub = (c.kw + tpr - 1) // tpr
        return w.view(c.cout, c.kh, nsub * tpr, 4)[:, :, :c.kw, :c.cin].permute(0, 3, 1, 2).contiguous()
    return w.view(c.cout, c.kh, c.kw, c.cin).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------
# split fp16: fp32-accurate values as (hi, lo) half pairs (conv_glds SPLIT)
# ---------------------------------------------------------------------------
# A value v is carried as hi = fp16(v), lo = fp16(v - hi) (22 significant bits);
# a pixel of C channels is 2C halfs laid out [hi x32][lo x32] per 32 channels.
# The conv sums hi*hi + hi*lo + lo*hi on the f16 MFMA in f32.  Weights are
# pre-scaled by 2^e so that max |w| ~ 2^14 (their lo parts stay normal halfs);
# the kernel multiplies the accumulator by 2^-e.  On ResNet18 this is as
# accurate as fp32 (CPU emulation: 1.2e-7 relative logit error vs fp64, fp32
# itself 2.7e-7; tests/test_split.py).

SPLIT_BLOCK = 32


def split_eligible(cin: int, cout: int) -> bool:
    return cin % SPLIT_BLOCK == 0 and cout % SPLIT_BLOCK == 0


def _hi_lo(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """hi = fp16(x), lo = fp16(x - hi), the difference in x's own precision."""
    hi = x.half()
    return hi, (x - hi.to(x.dtype)).half()


def to_split(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., C] -> split half [..., 2C] (C % 32 == 0)."""
    c = x.shape[-1]
    hi, lo = _hi_lo(x.float())
    blk = (*x.shape[:-1], c // SPLIT_BLOCK, 1, SPLIT_BLOCK)
    return torch.cat([hi.reshape(blk), lo.reshape(blk)], dim=-2).reshape(*x.shape[:-1], 2 * c)


def from_split(xs: torch.Tensor) -> torch.Tensor:
    """split half [..., 2C] -> fp32 [..., C] (hi + lo in f32)."""
    c = xs.shape[-1] // 2
    v = xs.float().reshape(*xs.shape[:-1], c // SPLIT_BLOCK, 2, SPLIT_BLOCK)
    return (v[..., 0, :] + v[..., 1, :]).reshape(*xs.shape[:-1], c)


def pack_split_weight(w: torch.Tensor, e: int | None = None) -> tuple[torch.Tensor, float]:
    """[Cout, Cin, KH, KW] -> (split weights [Cout, KH*KW*2*Cin] half, acc_scale).

    K order (kh, kw, 32-channel block, hi|lo, channel); the weights are scaled
    by 2^e (e from max |w|, so the largest is in [2^13, 2^14)) in fp64 before
    the split, acc_scale = 2^-e undoes it exactly in the epilogue.  ``e``
    forces the exponent (parts of one GEMM share one: pack_split_tail_weight)."""
    cout, cin, kh, kw = w.shape
    if cin % SPLIT_BLOCK:
        raise ValueError(f"split weights need Cin % {SPLIT_BLOCK} == 0, got {cin}")
    if e is None:
        e = _split_scale(w)
    hi, lo = _hi_lo(w.double().permute(0, 2, 3, 1) * (2.0 ** e))
    blk = (cout, kh, kw, cin // SPLIT_BLOCK, 1, SPLIT_BLOCK)
    packed = torch.cat([hi.reshape(blk), lo.reshape(blk)], dim=4).reshape(cout, kh * kw * 2 * cin)
    return packed.contiguous(), 2.0 ** -e


def _split_scale(w: torch.Tensor) -> int:
    mx = float(w.abs().max())
    return 0 if mx == 0.0 else 14 - math.ceil(math.log2(mx))


def pack_split_tail_weight(w2: torch.Tensor, wd: torch.Tensor) -> tuple[torch.Tensor, float]:
    """Weights of ops.conv2d_split_tail: [Cout, C, 3, 3] and the 1x1 downsample
    [Cout, Cx, 1, 1] -> ([Cout, 9*2C + 2Cx] split half, acc_scale).  Each part is
    packed as pack_split_weight does, with ONE exponent from the max |w| over
    both (the GEMM has one accumulator scale), the tail's K after the nine taps."""
    if wd.shape[0] != w2.shape[0] or tuple(wd.shape[2:]) != (1, 1) or tuple(w2.shape[2:]) != (3, 3):
        raise ValueError("tail weights: [Cout, C, 3, 3] and [Cout, Cx, 1, 1]")
    e = _split_scale(torch.cat([w2.flatten(), wd.flatten()]))
    s2, scale = pack_split_weight(w2, e)
    sd, _ = pack_split_weight(wd, e)
    return torch.cat([s2, sd], dim=1).contiguous(), scale


def pack_split_weight_p3(w: torch.Tensor) -> tuple[torch.Tensor, float]:
    """RGB stem [Cout, 3, KH, KW] -> split-fp16 packed-row weights (conv_glds
    P3+SPLIT): K = (kh, f = 3*kw + c) over cpk = ceil(3*KW/8) 8-half chunks per
    kernel row (preprocess_pack3_split's order), padded to whole stages of 32
    K elements, each stage [hi x32][lo x32]; scaled by 2^e like pack_split_weight."""
    flat = _p3_rows(w, 8, 32, torch.float64)
    cout, nk = flat.shape[0], flat.shape[1] // 32
    e = _split_scale(w)
    hi, lo = _hi_lo(flat * (2.0 ** e))
    packed = torch.cat([hi.reshape(cout, nk, 1, 32), lo.reshape(cout, nk, 1, 32)], dim=2).reshape(cout, nk * 64)
    return packed.contiguous(), 2.0 ** -e


def _pack_stem_u8(w: torch.Tensor, b: torch.Tensor | None, layout):
    """The exact-u8 stems' normalisation fold: (fs, scale, bias, psum) as the
    two stem packers document them.  ``layout`` maps w' = w * s_c
    [Cout, 3, KH, KW] fp64 to the kernel's [Cout, K] order (zeros in K's gaps)."""
    cout, _, kh, kw = w.shape
    w = w.double()
    mean = torch.tensor(ref.IMAGENET_MEAN, dtype=torch.float64)
    std = torch.tensor(ref.IMAGENET_STD, dtype=torch.float64)
    ws = w * (1.0 / (255.0 * std)).view(1, 3, 1, 1)
    e = _split_scale(ws)
    hi, lo = _hi_lo(layout(ws) * (2.0 ** e))
    corr = (w * (-mean / std).view(1, 3, 1, 1)).sum(dim=1)            # [Cout, KH, KW]
    ps = torch.zeros(kh + 1, kw + 1, cout, dtype=torch.float64)
    ps[1:, 1:] = corr.permute(1, 2, 0).cumsum(0).cumsum(1)
    bias = (torch.zeros(cout, dtype=torch.float64) if b is None else b.double()) + ps[kh, kw]
    return torch.stack([hi, lo]).contiguous(), 2.0 ** -e, bias.float().contiguous(), ps.float().contiguous()


def pack_stem_split(w: torch.Tensor, b: torch.Tensor | None = None):
    """ResNet stem [64, 3, 7, 7] (+ bias [64]) -> operands of the fused split stem
    (stem_fused.hip stem_split_kernel, exact-u8 form):

      fs     [2, 64, 7*32] half: hi and lo of w' = w * s_c, s_c = 1/(255 std_c),
             per kernel row 8 taps x 4 channels (tap 7, channel 3 zero), scaled
             by 2^e like pack_split_weight;
      scale  2^-e;
      bias   [64] f32: b + sum over all taps of w * c_c, c_c = -mean_c / std_c
             (the normalisation's shift for a pixel whose taps are all inside);
      psum   [8, 8, 64] f32: 2D prefix sums over (kh, kw) of sum_c w * c_c, from
             which the kernel corrects border pixels (zero padding in x, not u).

    conv(normalise(u)) = conv(w', u) + sum_{valid taps} w * c: u <= 255 is
    exact in fp16, so the B operand needs no lo part."""
    cout, cin, kh, kw = w.shape
    if (cout, cin, kh, kw) != (64, 3, 7, 7):
        raise ValueError("the fused split stem takes a [64, 3, 7, 7] conv")

    def layout(ws):
        p = torch.zeros(cout, kh, 8, 4, dtype=torch.float64)
        p[:, :, :kw, :cin] = ws.permute(0, 2, 3, 1)
        return p.reshape(cout, kh * 32)
    return _pack_stem_u8(w, b, layout)


def alex_stem_k_index(kh: int, kw: int) -> tuple[int, int]:
    """(K step, slot of 8-k group base) of tap (kh, kw) in the fused AlexNet stem's
    K layout (alex_stem.hip): step kh holds taps 0..7 of row kh as 8 x 4 channels;
    tail step 11 + t holds taps 8, 9 (k 0..7) and 10 (k 8..11) of row 2t, and the
    same of row 2t + 1 at k 16..27.  Returns (step, k of channel 0)."""
    if kw < 8:
        return kh, 4 * kw
    t, second = divmod(kh, 2)
    base = 16 * second
    return 11 + t, base + (4 * (kw - 8) if kw < 10 else 8)


def pack_alex_stem_split(w: torch.Tensor, b: torch.Tensor | None = None):
    """AlexNet conv1 [64, 3, 11, 11] (+ bias) -> operands of the fused split
    AlexNet stem (alex_stem.hip alex_stem_split_kernel, exact-u8 form):

      fs     [2, 64, 17*32] half: hi and lo of w' = w * s_c, s_c = 1/(255 std_c),
             in the kernel's K layout (alex_stem_k_index), scaled by 2^e;
      scale  2^-e;
      bias   [64] f32: b + sum over all taps of w * c_c, c_c = -mean_c / std_c;
      psum   [12, 12, 64] f32: 2D prefix sums over (kh, kw) of sum_c w * c_c (border
             outputs get their in-image taps' sum from it)."""
    cout, cin, kh, kw = w.shape
    if (cout, cin, kh, kw) != (64, 3, 11, 11):
        raise ValueError("the fused split AlexNet stem takes a [64, 3, 11, 11] conv")

    def layout(ws):
        p = torch.zeros(cout, 17, 32, dtype=torch.float64)
        for i in range(kh):
            for j in range(kw):
                st, k0 = alex_stem_k_index(i, j)
                p[:, st, k0:k0 + 3] = ws[:, :, i, j]
        return p.reshape(cout, 17 * 32)
    return _pack_stem_u8(w, b, layout)


def unpack_split_weight(c: "Conv") -> torch.Tensor:
    """Inverse of pack_split_weight -> fp32 [Cout, Cin, KH, KW] (hi + lo, unscaled)."""
    v = c.sw.double().reshape(c.cout, c.kh, c.kw, c.cin // SPLIT_BLOCK, 2, SPLIT_BLOCK)
    w = (v[..., 0, :] + v[..., 1, :]).reshape(c.cout, c.kh, c.kw, c.cin) * c.s_scale
    return w.permute(0, 3, 1, 2).float().contiguous()


# ---------------------------------------------------------------------------
# grouped 3x3 convs (ResNeXt): channel-block-local weights (conv3x3_grouped.hip)
# ---------------------------------------------------------------------------
# With Cg = Cin / groups = Cout / groups and CB = max(16, Cg), output channels
# [CB j, CB j + CB) read input channels of the same range only (groups are
# contiguous and Cg divides CB): per block a small dense [CB outputs, 9 taps, CB
# inputs] weight.  For Cg < 16 the slots outside an output's own group are zero
# (75 % zeros at Cg 4, 50 % at Cg 8; the kernel is bandwidth-bound).

GROUPED_CG = (4, 8, 16, 32, 64)


def grouped_block(cg: int) -> int:
    """Channel block CB of a grouped conv with ``cg`` channels per group."""
    if cg not in GROUPED_CG:
        raise ValueError(f"grouped conv: {cg} channels per group unsupported (need one of {GROUPED_CG})")
    return max(16, cg)


def _grouped_shape(w: torch.Tensor, groups: int) -> tuple[int, int, int]:
    """(Cout, Cg, CB) of a grouped 3x3 weight [Cout, Cg, 3, 3], checked."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"grouped conv weights must be [Cout, Cin/groups, 3, 3], got {tuple(w.shape)}")
    cout, cg = w.shape[0], w.shape[1]
    if groups < 2 or cout % groups or cout // groups != cg:
        raise ValueError(f"grouped conv: Cout={cout}, groups={groups} and {cg} input channels per group do not "
                         "describe a conv with Cin = Cout")
    if cg not in GROUPED_CG:
        raise ValueError(f"grouped conv: Cout={cout} / groups={groups} = {cg} channels per group unsupported "
                         f"(need one of {GROUPED_CG})")
    return cout, cg, grouped_block(cg)


def _grouped_rows(w: torch.Tensor, groups: int) -> torch.Tensor:
    """[Cout, Cg, 3, 3] -> block-local rows [Cout, 9 * CB] in w's dtype."""
    cout, cg, cb = _grouped_shape(w, groups)
    rows = torch.zeros(cout, 9, cb, dtype=w.dtype)
    slot = (torch.arange(cout) % cb) // cg * cg             # first slot of each output's own group
    idx = slot.view(-1, 1) + torch.arange(cg).view(1, -1)   # [Cout, Cg]
    rows.scatter_(2, idx.view(cout, 1, cg).expand(cout, 9, cg), w.permute(0, 2, 3, 1).reshape(cout, 9, cg))
    return rows.reshape(cout, 9 * cb)


def pack_grouped_weight(w: torch.Tensor, groups: int, dtype: str = "fp16") -> torch.Tensor:
    """[Cout, Cg, 3, 3] fp32/fp64 -> block-local fp16 weights [Cout, 9 * CB].

    Row ``co`` is the K axis of the block's GEMM: k = tap * CB + ci with
    tap = 3 kh + kw and ci the input channel within co's channel block
    (input channel CB * (co // CB) + ci); slot ci holds w[co, ci % Cg, kh, kw]
    where ci // Cg == (co % CB) // Cg, zero elsewhere.  The kernel reads it in
    K-steps of 32 (CB 16: two taps a step, the tenth tap absent)."""
    if dtype != "fp16":
        raise ValueError("grouped weights are fp16 (fp32 programs carry pack_grouped_split_weight)")
    return _grouped_rows(w.float(), groups).half().contiguous()


def pack_grouped_split_weight(w: torch.Tensor, groups: int) -> tuple[torch.Tensor, float]:
    """[Cout, Cg, 3, 3] -> (split block-local weights [Cout, 2 * 9 * CB] half,
    acc_scale): each row is [hi 9 CB | lo 9 CB] of pack_grouped_weight's row,
    scaled by 2^e (one exponent per conv) exactly as pack_split_weight does."""
    e = _split_scale(w)
    hi, lo = _hi_lo(_grouped_rows(w.double(), groups) * (2.0 ** e))
    return torch.cat([hi, lo], dim=1).contiguous(), 2.0 ** -e


def unpack_grouped_weight(c: "Conv") -> torch.Tensor:
    """Inverse of pack_grouped_weight (``c.w`` fp16 rows) and of
    pack_grouped_split_weight (``c.sw``, preferred when present: hi + lo,
    unscaled) -> fp32 [Cout, Cg, 3, 3]."""
    cg = c.cin // c.groups
    cb = grouped_block(cg)
    if c.sw is not None:
        rows = (c.sw[:, :9 * cb].double() + c.sw[:, 9 * cb:].double()) * c.s_scale
    else:
        rows = c.w.double()
    slot = (torch.arange(c.cout, device=rows.device) % cb) // cg * cg
    idx = slot.view(-1, 1) + torch.arange(cg, device=rows.device).view(1, -1)
    w = rows.reshape(c.cout, 9, cb).gather(2, idx.view(c.cout, 1, cg).expand(c.cout, 9, cg))
    return w.reshape(c.cout, 3, 3, cg).permute(0, 3, 1, 2).float().contiguous()


def expand_grouped_weight(w: torch.Tensor, groups: int) -> torch.Tensor:
    """[Cout, Cg, 3, 3] -> the dense block-diagonal [Cout, Cin, 3, 3] (w's dtype)
    that computes the same conv without ``groups``: groups x the weights."""
    cout, cg = w.shape[0], w.shape[1]
    if cout % groups or cout // groups != cg:
        raise ValueError(f"grouped conv: Cout={cout}, groups={groups}, {cg} channels per group")
    dense = torch.zeros(cout, cout, *w.shape[2:], dtype=w.dtype, device=w.device)
    for g in range(groups):
        dense[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return dense


# Winograd F(2x2, 3x3) filter transform (Lavin & Gray): U = G g G^T
WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def wino_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> U [16, Cout, Cin] fp32, U[4i+j] = (G g G^T)[i][j],
    computed in fp64 and rounded once (conv_wino_f32.hip's A operand)."""
    assert w.shape[2:] == (3, 3)
    u = torch.einsum("ia,ocab,jb->ijoc", WINO_G, w.double(), WINO_G)
    return u.reshape(16, w.shape[0], w.shape[1]).float().contiguous()


def wino_eligible(cin: int, cout: int, kh: int, kw: int, stride: int, pad: int) -> bool:
    return kh == 3 and kw == 3 and stride == 1 and pad == 1 and cin % 16 == 0 and cout % 32 == 0


def make_conv(conv: nn.Conv2d, bn: nn.BatchNorm2d | None, relu: bool, dtype: str = "fp16") -> Conv:
    w64, b64 = fold_bn_f64(conv.weight, conv.bias, bn)      # folded once; the fp32 pair is its rounding
    w, b = w64.float(), b64.float()
    cin, cout, (kh, kw), stride, pad = conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride[0], \
        conv.padding[0]
    f32 = dtype == "fp32"
    if conv.groups > 1:
        # block-local weights only: never pack_conv_weight (Cin / groups is no multiple of 64) and no
        # dense expansion here (resnext101_32x8d's would be 1.4 GB in fp32; runner.py builds one lazily
        # per conv where a path needs it)
        if (kh, kw, pad) != (3, 3, 1) or stride not in (1, 2) or cin != cout:
            raise ValueError(f"grouped convs are 3x3 pad-1 stride-1/2 with Cin = Cout, got {tuple(conv.weight.shape)} "
                             f"stride {stride} pad {pad} groups {conv.groups}")
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
        c = Conv(w=w.contiguous() if f32 else pack_grouped_weight(w, conv.groups), b=b.contiguous(), cin=cin,
                 cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, relu=relu, groups=conv.groups)
        if f32:
            c.sw, c.s_scale = pack_grouped_split_weight(w64, conv.groups)
        return c
    pw, small = pack_conv_weight(w, dtype)
    c = Conv(w=pw, b=b.contiguous(), cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad, relu=relu, small=small)
    if f32 and split_eligible(cin, cout):
        c.sw, c.s_scale = pack_split_weight(w64)
    if f32 and wino_eligible(cin, cout, kh, kw, stride, pad):
        c.wino = wino_weight(w)
    if pack3_eligible(cin, kw, stride, dtype):
        c.p3 = pack_conv_weight_p3(w, dtype)
    if f32 and pack3_eligible(cin, kw, stride, "fp16") and cout % 64 == 0:
        c.sp3, c.s_scale = pack_split_weight_p3(w64)
    if tuple(conv.weight.shape) == (64, 3, 7, 7) and stride == 2 and pad == 3:
        # the exact-u8 stem: split (fp32 programs) or its hi parts alone (fp16, ops.stem_u8_f16)
        c.fs, c.fs_scale, c.fs_bias, c.fs_psum = pack_stem_split(w64, b64)
    elif tuple(conv.weight.shape) == (64, 3, 11, 11) and stride == 4 and pad == 2:
        # the fused AlexNet stem: split (ops.alex_stem_split) or its hi parts alone
        # (fp16 programs, ops.alex_stem_u8_f16)
        c.fs, c.fs_scale, c.fs_bias, c.fs_psum = pack_alex_stem_split(w64, b64)
    return c


def make_fc(lin: nn.Linear, relu: bool, perm: torch.Tensor | None = None, dtype: str = "fp16") -> Conv:
    w = lin.weight.detach().float()
    if perm is not None:
        w = w[:, perm]
    k = w.shape[1]
    if k % 64 != 0:
        raise ValueError(f"FC in_features={k} must be a multiple of 64")
    sw, s_scale = None, 1.0
    if dtype == "fp32" and k % SPLIT_BLOCK == 0:
        w64 = lin.weight.detach().double()
        if perm is not None:
            w64 = w64[:, perm]
        sw, s_scale = pack_split_weight(w64.reshape(w.shape[0], k, 1, 1))
    return Conv((w if dtype == "fp32" else w.half()).contiguous(), lin.bias.detach().float().contiguous(), k, w.shape[0], 1, 1, 1,
                0, relu, False, sw=sw, s_scale=s_scale)


def compile_model(m: nn.Module, name: str, dtype: str = "fp16") -> Program:
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
    m = m.eval()
    dt = dtype
    if isinstance(m, ref.ResNet):
        p = Program(name, "resnet", stem=make_conv(m.conv1, m.bn1, True, dt), dtype=dt)
        for li in range(1, 5):
            for blk in getattr(m, f"layer{li}"):
                down = make_conv(blk.downsample[0], blk.downsample[1], False, dt) if blk.downsample else None
                if isinstance(blk, ref.BasicBlock):
                    convs = [make_conv(blk.conv1, blk.bn1, True, dt), make_conv(blk.conv2, blk.bn2, True, dt)]
                else:
                    convs = [make_conv(blk.conv1, blk.bn1, True, dt), make_conv(blk.conv2, blk.bn2, True, dt),
                             make_conv(blk.conv3, blk.bn3, True, dt)]
                p.blocks.append(Block(convs, down))
        p.fcs = [make_fc(m.fc, False, dtype=dt)]
        p.num_classes = m.fc.out_features
        return p
    if isinstance(m, ref.AlexNet):
        p = Program(name, "alexnet", dtype=dt)
        mods = list(m.features)
        i = 0
        while i < len(mods):
            mod = mods[i]
            if isinstance(mod, nn.Conv2d):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                p.features.append(("conv", make_conv(mod, None, relu, dt)))
                i += 2 if relu else 1
                continue
            if isinstance(mod, nn.MaxPool2d):
                p.features.append(("pool", (mod.kernel_size, mod.stride, mod.padding)))
            i += 1
        # NCHW flatten (c, h, w) -> our NHWC flatten (h, w, c)
        c, hw = 256, 36
        perm = torch.arange(c * hw).view(c, hw).t().reshape(-1)
        lins = [mm for mm in m.classifier if isinstance(mm, nn.Linear)]
        p.fcs = [make_fc(lins[0], True, perm, dt), make_fc(lins[1], True, dtype=dt),
                 make_fc(lins[2], False, dtype=dt)]
        p.num_classes = lins[2].out_features
        return p
    raise TypeError(f"cannot compile {type(m).__name__}")


def build_program(name: str, seed: int = 0, randomize_bn: bool = False, dtype: str = "fp16",
                  weights=None) -> Program:
    """Program of the named architecture.  ``weights`` (a checkpoint path or a
    state dict, see ``models.checkpoint``) supplies the parameters; without it
    they are random-init from ``seed`` (which ``weights`` makes irrelevant)."""
    name = ref.canonical(name)
    if weights is not None:
        from .checkpoint import load_model

        return compile_model(load_model(name, weights), name, dtype)
    return compile_model(ref.build(name, seed=seed, randomize_bn=randomize_bn), name, dtype)


# ---------------------------------------------------------------------------
# fp32 torch emulation of a packed program (CPU-testable)
# ---------------------------------------------------------------------------

def _emu_conv(c: Conv, x: torch.Tensor, res: torch.Tensor | None = None) -> torch.Tensor:
    y = F.conv2d(x, unpack_conv_weight(c).to(x.device), c.b.to(x.device), c.stride, c.pad, groups=c.groups)
    if res is not None:
        y = y + res
    return F.relu(y) if c.relu else y


@torch.no_grad()
def emulate(p: Program, img_u8: torch.Tensor) -> torch.Tensor:
    """fp32 logits of the packed program on NCHW torch ops."""
    x = ref.preprocess_u8(img_u8)
    if p.kind == "resnet":
        x = F.max_pool2d(_emu_conv(p.stem, x), 3, 2, 1)
        for blk in p.blocks:
            idt = x if blk.down is None else _emu_conv(blk.down, x)
            y = x
            for c in blk.convs[:-1]:
                y = _emu_conv(c, y)
            x = _emu_conv(blk.convs[-1], y, idt)
        x = x.mean(dim=(2, 3))
    else:
        for k, v in p.features:
            x = _emu_conv(v, x) if k == "conv" else F.max_pool2d(x, *v)
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    for fc in p.fcs:
        x = F.linear(x, fc.w.float().to(x.device), fc.b.to(x.device))
        if fc.relu:
            x = F.relu(x)
    return x


def program_flops(p: Program, hw: int = 224) -> float:
    """Analytic forward FLOPs per image (2*MAC, convs + FCs)."""
    tot = 0.0

    def out_hw(h, c):
        return (h + 2 * c.pad - c.kh) // c.stride + 1

    if p.kind == "resnet":
        h = out_hw(hw, p.stem)
        tot += h * h * p.stem.flops_per_out_pixel
        h = (h + 2 - 3) // 2 + 1
        for blk in p.blocks:
            hin = h
            for c in blk.convs:
                h = out_hw(h, c)
                tot += h * h * c.flops_per_out_pixel
            if blk.down is not None:
                hd = out_hw(hin, blk.down)
                tot += hd * hd * blk.down.flops_per_out_pixel
    else:
        h = hw
        for k, v in p.features:
            if k == "conv":
                h = out_hw(h, v)
                tot += h * h * v.flops_per_out_pixel
            else:
                kk, s, pp = v
                h = (h + 2 * pp - kk) // s + 1
    for fc in p.fcs:
        tot += fc.flops_per_out_pixel
    return tot

