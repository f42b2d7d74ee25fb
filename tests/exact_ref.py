"""Bit-exact oracle for the fp16 and f32-MFMA conv / FC kernels.

The test data are small dyadic rationals: every product x*w and every partial
sum of a conv is an integer multiple of one unit q, and the sum of the terms'
magnitudes stays below 2^24 * q.  Under those two conditions fp32 accumulation
is exact in ANY order (any tile shape, K split, MFMA shape; Winograd too, whose
transforms only add and halve), so the one correct output is the float64
reference rounded once, and the comparison is ``torch.equal``.

Plain torch on the CPU, float64 throughout; tensors are NCHW / OIHW here and
``nhwc`` turns them into the kernels' layout.  Shared by test_exact_cpu.py
(which proves that the oracle discriminates) and the two GPU files.

The split-fp16 kernels have their own section at the end: the oracle of their
arithmetic contract (hi*hi + hi*lo + lo*hi, no lo*lo) on NON-CANONICAL
activation pairs, shared by test_exact_split_cpu.py and test_exact_split_gpu.py.
"""
import functools
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

TWO24 = float(2 ** 24)


def case_seed(*key) -> int:
    """A fixed seed per case tuple (no global RNG, no dependence on test order)."""
    return zlib.crc32(repr(key).encode())


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def _unit(t) -> float:
    """Largest power of two q such that every element of ``t`` is an integer multiple of q."""
    if t is None or t.numel() == 0 or not bool(t.any()):
        return float(2 ** 8)
    s = t * 2.0 ** 40
    v = s.long()
    assert torch.equal(v.double(), s), "data is not on a dyadic grid of at most 40 fractional bits"
    low = v & -v                                # lowest set bit of each element
    return min(float(low[low != 0].min().item()) * 2.0 ** -40, float(2 ** 8))


def grid_conv_case(B, H, W, Cin, Cout, k, stride, pad, res, seed, *, coarse=False):
    """x [B,Cin,H,W] in {-4..4}; w [Cout,Cin,k,k] in {-128..128}/4096; bias in
    {-1024..1024}/4096; residual (or None) in multiples of 1/1024 in [-2, 2].
    ``coarse``: w in {-8..8}/64, bias in {-16..16}/64, residual in multiples of 1/64
    in [-2, 2] -- every output is then a multiple of 1/64 and, below 32 in magnitude,
    fp16-representable (the first stage of conv1x1_fused_next, whose stored fp16
    output feeds the second GEMM).  All float64; x, w and the residual are fp16 values."""
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).double()

    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = ints(-4, 4, B, Cin, H, W)
    if coarse:
        w = ints(-8, 8, Cout, Cin, k, k) / 64
        bias = ints(-16, 16, Cout) / 64
        r = ints(-128, 128, B, Cout, Ho, Wo) / 64 if res else None
    else:
        w = ints(-128, 128, Cout, Cin, k, k) / 4096
        bias = ints(-1024, 1024, Cout) / 4096
        r = ints(-2048, 2048, B, Cout, Ho, Wo) / 1024 if res else None
    for t in (x, w, r):
        assert t is None or torch.equal(t.half().double(), t), "operand is not an fp16 value"
    assert torch.equal(bias.float().double(), bias)
    return x, w, bias, r


def dual_input(y, x, stride):
    """The A operand of a [y | x] GEMM: x gathered at ``stride``, channels concatenated."""
    return torch.cat([y, x[:, :, ::stride, ::stride]], 1)


# Winograd F(2x2, 3x3) (Lavin & Gray): Y = A^T [(G g G^T) . (B^T d B)] A
_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
_BT = torch.tensor([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_AT = torch.tensor([[1.0, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_u(w):
    """G g G^T in float64: [16, Cout, Cin], U[4i+j] = (G g G^T)[i][j]."""
    u = torch.einsum("ia,ocab,jb->ijoc", _G, w.double(), _G)
    return u.reshape(16, w.shape[0], w.shape[1])


def _wino_terms(x, w):
    """(U, V) of the 3x3 / stride 1 / pad 1 conv: U [16,Cout,Cin], V [B,Cin,16,T]
    over the 2x2 output tiles (odd sizes padded with zeros)."""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1 + W % 2, 1, 1 + H % 2))
    d = F.unfold(xp, 4, stride=2).reshape(B, C, 4, 4, -1)
    v = torch.einsum("ia,bcajt,kj->bcikt", _BT, d, _BT).reshape(B, C, 16, -1)
    return wino_u(w), v


def wino_emulate(x, w, dtype=torch.float32):
    """F(2x2,3x3) in ``dtype`` arithmetic (transforms, channel sums, output transform):
    [B,Cout,H,W] without bias.  fp32 here against the float64 direct conv shows that
    the Winograd route is exact on the grid."""
    B, C, H, W = x.shape
    u64, v64 = _wino_terms(x, w)
    u, v = u64.to(dtype), v64.to(dtype)
    assert torch.equal(u.double(), u64) and torch.equal(v.double(), v64)
    m = torch.einsum("koc,bckt->bokt", u, v).reshape(B, -1, 4, 4, v.shape[-1])
    at = _AT.to(dtype)
    y = torch.einsum("pi,boijt,qj->bopqt", at, m, at)                       # [B,Cout,2,2,T]
    th, tw = (H + 1) // 2, (W + 1) // 2
    y = y.reshape(B, -1, 2, 2, th, tw).permute(0, 1, 4, 2, 5, 3).reshape(B, -1, 2 * th, 2 * tw)
    return y[:, :, :H, :W]


_memo = {}


def _conv_parts(x, w, stride, pad, wino, groups=1):
    """(conv(x, w), bound on the magnitudes any summation order can reach, the
    products' unit), float64.
    One entry is kept, keyed by the operands' storage, so the ReLU / residual
    variants of one case share one reference."""
    key = (x.data_ptr(), w.data_ptr(), tuple(x.shape), tuple(w.shape), stride, pad, wino, groups)
    if _memo.get("key") != key:
        acc = F.conv2d(x, w, None, stride, pad, groups=groups)
        mag = F.conv2d(x.abs(), w.abs(), None, stride, pad, groups=groups).max().item()
        if wino:
            assert w.shape[2:] == (3, 3) and stride == 1 and pad == 1
            u, v = _wino_terms(x, w)
            m = torch.einsum("koc,bckt->bokt", u.abs(), v.abs())            # sum over Cin of |U||V|
            m = m.reshape(x.shape[0], -1, 4, 4, v.shape[-1])
            mag = max(mag, torch.einsum("pi,boijt,qj->bopqt", _AT.abs(), m, _AT.abs()).max().item())
        _memo.clear()
        _memo.update(key=key, x=x, w=w, acc=acc, mag=mag, q=_unit(x) * _unit(w) * (0.25 if wino else 1.0))
    return _memo["acc"], _memo["mag"], _memo["q"]


def exact_conv(x, w, bias, stride, pad, relu, residual=None, *, wino=False, groups=1):
    """(ref64 [B,Cout,Ho,Wo], unit q, headroom).  Every term and partial sum of
    the conv is a multiple of q; headroom = max(conv(|x|,|w|) + |bias| + |res|) /
    (2^24 q) < 1 (asserted) proves that fp32 accumulation in any order is exact,
    so a case that fails it is wrong, not flaky.  ``wino``: q shrinks by the 1/4
    of G g G^T, and the bound is |U|.|V| summed over Cin through the output
    transform.  Dual [y | x] GEMMs and linear layers are 1x1 convs here
    (``dual_input``; [M,K,1,1]); ``groups`` as in F.conv2d."""
    acc, mag, q = _conv_parts(x, w, stride, pad, wino, groups)
    q = min(q, _unit(bias), _unit(residual))
    ref = acc + bias.view(1, -1, 1, 1)
    extra = bias.abs().view(1, -1, 1, 1)
    if residual is not None:
        ref = ref + residual
        extra = extra + residual.abs()
    # the elementwise maximum of conv(|x|,|w|) + |bias| + |res| is at most mag + max(extra)
    headroom = (mag + extra.max().item()) / (TWO24 * q)
    assert headroom < 1, f"case is not order-independent: headroom {headroom:.3f} (unit 2^{torch.tensor(q).log2().item():.0f})"
    s = ref / q
    assert torch.equal(s, torch.round(s))
    if relu:
        ref = F.relu(ref)
    return ref, q, headroom


def expect_f16(ref64):
    """One round-to-nearest-even of the exact result."""
    return ref64.half()


def expect_f32(ref64):
    """The exact result as fp32: lossless on the grid (asserted)."""
    y = ref64.float()
    assert torch.equal(y.double(), ref64), "exact result does not fit fp32"
    return y


def _ordinal(t):
    """Sign-magnitude bit pattern -> a monotone integer (adjacent floats differ by 1)."""
    bits = t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).long()
    mask = 0x7FFF if t.dtype == torch.float16 else 0x7FFFFFFF
    return torch.where(bits < 0, -(bits & mask), bits)


def f16_other_neighbour(ref64):
    """(h, o): h = ref64.half(), o = the fp16 value on the other side of ref64
    (o = h where ref64 is representable)."""
    h = ref64.half()
    hd = h.double()
    bits = h.contiguous().view(torch.int16)
    step = torch.where(hd.abs() < ref64.abs(), 1, -1).to(torch.int16)      # magnitude up / down
    # h == 0 < |ref|: the neighbour carries ref's sign
    zero = (hd == 0) & (ref64 != 0)
    o = (bits + step).view(torch.float16)
    o = torch.where(zero, torch.copysign(torch.full_like(hd, 2.0 ** -24), ref64).half(), o)
    return h, torch.where(hd == ref64, h, o)


def f16_stats(ref64):
    """(fraction of values that are not fp16-representable, fraction that are exact ties)."""
    h, o = f16_other_neighbour(ref64)
    inexact = h.double() != ref64
    tie = inexact & ((h.double() - ref64).abs() == (o.double() - ref64).abs())
    return inexact.double().mean().item(), tie.double().mean().item()


def assert_bits(y, expect, ref64=None, split=False):
    """torch.equal on CPU copies of NHWC tensors.  On failure: the number of
    differing elements, the first few NHWC indices with got / want / the float64
    value, and whether every difference is within one ulp of the output type
    (a rounding fault) or not (an arithmetic fault).

    ``split``: both tensors are in the split layout [.., 2C] (``ref64`` is the
    value, [.., C]).  The report then names the plane (hi or lo), the channel
    and the pixel of each difference, counts the differing halfs per plane, and
    says whether all of them are within one fp16 ulp of the lo plane (the lo
    rounding) or not (the arithmetic, or the hi half)."""
    y = y.detach().cpu()
    expect = expect.detach().cpu()
    assert y.dtype == expect.dtype and y.shape == expect.shape, (y.dtype, expect.dtype, y.shape, expect.shape)
    if torch.equal(y, expect):
        return
    bad = ~(y == expect)                       # NaNs differ
    idx = bad.nonzero()
    finite = bool(torch.isfinite(y[bad]).all())
    ulps = (_ordinal(y) - _ordinal(expect)).abs()[bad]
    within = finite and int(ulps.max()) <= 1
    name = "fp16" if y.dtype == torch.float16 else "fp32"
    if split:
        assert y.dtype == torch.float16 and y.shape[-1] % 64 == 0, "not a split tensor"
        hi_bad, lo_bad = split_planes(bad)
        n_hi, n_lo = int(hi_bad.sum()), int(lo_bad.sum())
        lo_only = within and n_hi == 0
        lines = [f"{idx.shape[0]} of {y.numel()} halfs differ ({n_hi} in the hi plane, {n_lo} in the lo plane) at "
                 f"{int((hi_bad | lo_bad).sum())} of {hi_bad.numel()} outputs; "
                 + ("all within one fp16 ulp of the lo plane (the lo rounding)" if lo_only else
                    f"NOT all within one fp16 ulp of the lo plane (max {int(ulps.max())} ulps"
                    f"{'' if finite else ', non-finite values'})")]
        for i in idx[:8].tolist():
            *pix, j = i
            c = j // 64 * 32 + j % 32
            plane = "lo" if j % 64 >= 32 else "hi"
            exact = "" if ref64 is None else f" exact value {ref64[(*pix, c)].item():.10g}"
            lines.append(f"  {plane} plane, channel {c}, pixel (b, h, w) {pix}: got {y[tuple(i)].item():.10g} "
                         f"want {expect[tuple(i)].item():.10g}{exact}")
        raise AssertionError("\n".join(lines))
    lines = [f"{idx.shape[0]} of {y.numel()} elements differ; "
             + (f"all within one {name} ulp (a rounding fault)" if within else
                f"NOT all within one {name} ulp (an arithmetic fault; max {int(ulps.max())} ulps"
                f"{'' if finite else ', non-finite values'})")]
    for i in idx[:8].tolist():
        t = tuple(i)
        exact = "" if ref64 is None else f" exact {ref64[t].item():.10g}"
        lines.append(f"  NHWC{list(t)}: got {y[t].item():.10g} want {expect[t].item():.10g}{exact}")
    raise AssertionError("\n".join(lines))


# ---------------------------------------------------------------------------
# cases: what the GPU files run and test_exact_cpu.py qualifies
# ---------------------------------------------------------------------------

class Case(NamedTuple):
    x: torch.Tensor            # [B,Cin,H,W] float64
    w: torch.Tensor            # [Cout,Cin,k,k]
    bias: torch.Tensor         # [Cout]
    res: torch.Tensor          # [B,Cout,Ho,Wo] (a test may leave it out)
    stride: int
    pad: int
    wino: bool = False
    coarse: bool = False
    groups: int = 1

    def ref(self, relu, use_res):
        """The exact result (NCHW float64) of this case."""
        return exact_conv(self.x, self.w, self.bias, self.stride, self.pad, relu,
                          self.res if use_res else None, wino=self.wino, groups=self.groups)[0]


@functools.lru_cache(maxsize=2)
def conv_case(B, H, W, Cin, Cout, k, stride, pad, coarse=False, wino=False) -> Case:
    seed = case_seed("conv", B, H, W, Cin, Cout, k, stride, pad, coarse)
    x, w, b, r = grid_conv_case(B, H, W, Cin, Cout, k, stride, pad, True, seed, coarse=coarse)
    return Case(x, w, b, r, stride, pad, wino, coarse)


@functools.lru_cache(maxsize=2)
def grouped_case(B, H, W, C, groups, stride) -> Case:
    """A grouped 3x3 pad-1 conv with Cin = Cout = C (conv3x3_grouped.hip; no residual):
    x in {-4..4}, w [C, C/groups, 3, 3] in {-128..128}/256, bias in {-1024..1024}/4096.
    The weights are 16 x grid_conv_case's, so that the short K of a group (36 at
    four channels per group, 4 where only the centre tap is inside) still
    reaches outputs past 1, which fp16 does not hold to the bias' 2^-12."""
    g = torch.Generator().manual_seed(case_seed("grouped", B, H, W, C, groups, stride))
    x = torch.randint(-4, 5, (B, C, H, W), generator=g).double()
    w = torch.randint(-128, 129, (C, C // groups, 3, 3), generator=g).double() / 256
    bias = torch.randint(-1024, 1025, (C,), generator=g).double() / 4096
    assert torch.equal(w.half().double(), w)
    return Case(x, w, bias, None, stride, 1, groups=groups)


def linear_case(M, K, N) -> Case:
    """A linear layer as the 1x1 conv of an [M,K,1,1] input (no residual)."""
    return conv_case(M, 1, 1, K, N, 1, 1, 0)


@functools.lru_cache(maxsize=2)
def dual_case(B, Ho, K1, K2, Cout, stride, coarse=False):
    """(case, y, x, w_y, w_x): the bottleneck tail act([y | x at stride] . [w_y | w_x]^T + bias)
    as ONE 1x1 conv case over the concatenated channels; y [B,K1,Ho,Ho], x [B,K2,H,H]."""
    H = (Ho - 1) * stride + 1 + (stride - 1)
    s1 = case_seed("dual-y", B, Ho, K1, K2, Cout, stride, coarse)
    s2 = case_seed("dual-x", B, Ho, K1, K2, Cout, stride, coarse)
    y, wy, by, r = grid_conv_case(B, Ho, Ho, K1, Cout, 1, 1, 0, True, s1, coarse=coarse)
    x, wx, bx, _ = grid_conv_case(B, H, H, K2, Cout, 1, stride, 0, False, s2, coarse=coarse)
    case = Case(dual_input(y, x, stride), torch.cat([wy, wx], 1), by + bx, r, 1, 0, False, coarse)
    return case, y, x, wy, wx


def parametrize_args(fn, first):
    """The value list of the ``pytest.mark.parametrize`` of test function ``fn``
    whose first argument name is ``first`` (the existing files keep their case
    lists in the decorators)."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0].split(",")[0].strip() == first:
            return list(m.args[1])
    raise KeyError((fn.__name__, first))


# ---------------------------------------------------------------------------
# split-fp16 kernels: the arithmetic contract, bit for bit
# ---------------------------------------------------------------------------
# A split kernel is bilinear in its four planes and computes
#
#     acc = sum x_hi*w_hi + x_hi*w_lo + x_lo*w_hi          (no lo*lo), in f32
#     v   = acc * 2^-e + bias (+ res_hi + res_lo), ReLU
#
# and stores v as fp32, or split: hi = fp16(v), lo = fp16(v - hi).  As above,
# when every term is a multiple of one unit q and the magnitudes sum to less
# than 2^24 q, the f32 result does not depend on the order, and the one correct
# output is the float64 value of that expression.
#
# NON-CANONICAL ACTIVATION PAIRS.  A canonical pair (lo = fp16(v - fp16(v)), so
# |lo| <= ulp(hi)/2) cannot meet the 24-bit window at a real K: hi*hi and lo*hi
# are 11 bits apart before K is summed.  The kernels take the pair as two
# independent planes, so the exact cases feed x_hi = a small integer and x_lo =
# an independent small dyadic value (the residual's planes likewise).  The
# weights go through the real packers and ARE canonical: integers n / 2^11, most
# of them |n| <= 64 (lo = 0), a few "wide" odd |n| in [2049, 16383] whose fp16 hi
# leaves a non-zero lo.  The tolerance tests on randn data (test_split.py,
# test_split_tail.py, test_band.py, test_grouped_gpu.py) keep covering
# canonical pairs.
#
# The split store rounds only the 24th bit of v (hi and lo hold 11 bits and a
# sign each), so it is exercised by outputs past half the window: output
# channels n % 8 == 1 / 5 carry a bias of +- SPLIT_BIG, which puts |v| in
# [2^23 q, 2^24 q); a quarter of those outputs are ties of the lo rounding.

SPLIT_E = 11                 # the packers' exponent for max |n| in (2^13, 2^14)
SPLIT_BIG = 2304.0           # |v| >= 2048 = 2^23 q at q = 2^-12: the lo half drops v's last bit


def split_layout(hi, lo):
    """Planes [.., C] -> the kernels' split layout [.., 2C] half ([hi x32][lo x32]
    per 32 channels); lossless (asserted)."""
    c = hi.shape[-1]
    blk = (*hi.shape[:-1], c // 32, 1, 32)
    t = torch.cat([hi.reshape(blk), lo.reshape(blk)], dim=-2).reshape(*hi.shape[:-1], 2 * c)
    h = t.half()
    assert torch.equal(h.to(t.dtype), t), "plane is not an fp16 value"
    return h


def split_planes(xs):
    """Split layout [.., 2C] -> (hi, lo), each [.., C]."""
    c = xs.shape[-1] // 2
    v = xs.reshape(*xs.shape[:-1], c // 32, 2, 32)
    return v[..., 0, :].reshape(*xs.shape[:-1], c), v[..., 1, :].reshape(*xs.shape[:-1], c)


class SplitPart(NamedTuple):
    """One K range of a split GEMM: conv(x, w) at its own stride / pad."""
    xh: torch.Tensor           # [B,C,H,W] float64
    xl: torch.Tensor
    wh: torch.Tensor           # [Cout,C/groups,k,k] float64: the packer's planes of w * 2^e
    wl: torch.Tensor
    stride: int
    pad: int
    groups: int = 1

    def conv(self, x, w, dtype=torch.float64):
        return F.conv2d(x.to(dtype), w.to(dtype), None, self.stride, self.pad, groups=self.groups)


class SplitCase:
    """Operands of one exact split case.  ``parts`` share one accumulator (the
    two-input kernels are ONE GEMM over the concatenated K); ``w`` are the
    float64 weights as given to the packer, ``sw`` its output, ``scale`` = 2^-e."""

    def __init__(self, parts, scale, bias, res_hi, res_lo, w, sw):
        self.parts, self.scale, self.bias = tuple(parts), scale, bias
        self.res_hi, self.res_lo, self.w, self.sw = res_hi, res_lo, w, sw
        self._terms = None

    def terms(self):
        """(acc, mag): the contract's accumulator in float64 and the sum of its
        terms' magnitudes (fp32 is exact for that sum while it is below 2^24
        units, and past that the headroom assertion fails either way)."""
        if self._terms is None:
            # x_hi*w_hi + x_hi*w_lo as one conv with w_hi + w_lo: the same float64 value (all sums are exact)
            acc = sum(p.conv(p.xh, p.wh + p.wl) + p.conv(p.xl, p.wh) for p in self.parts)
            mag = sum(p.conv(p.xh.abs(), p.wh.abs() + p.wl.abs(), torch.float32)
                      + p.conv(p.xl.abs(), p.wh.abs(), torch.float32) for p in self.parts).double()
            self._terms = (acc, mag)
        return self._terms

    def ref(self, relu, use_res):
        return exact_split_conv(self, relu, use_res)[0]


def split_epilogue(case, acc, relu, use_res, *, bias=None, res_lo=True):
    """v = acc * 2^-e + bias (+ res_hi + res_lo), ReLU; float64."""
    v = acc * case.scale + (case.bias if bias is None else bias).view(1, -1, 1, 1)
    if use_res:
        v = v + case.res_hi + (case.res_lo if res_lo else 0.0)
    return F.relu(v) if relu else v


def exact_split_conv(case, relu, use_res=False):
    """(ref64 [B,Cout,Ho,Wo], unit q, headroom) of the split contract
    sum x_hi*w_hi + x_hi*w_lo + x_lo*w_hi (no lo*lo) through the epilogue.
    Every term is a multiple of q; headroom = max over the outputs of
    (conv(|x_hi|,|w_hi|) + conv(|x_hi|,|w_lo|) + conv(|x_lo|,|w_hi|)) 2^-e + |bias|
    + |res_hi| + |res_lo|, over 2^24 q, and < 1 (asserted): f32 accumulation is
    exact in any order, tile, K split or K concatenation."""
    acc, mag = case.terms()
    q = min(min(_unit(p.xh) * _unit(p.wh), _unit(p.xh) * _unit(p.wl), _unit(p.xl) * _unit(p.wh))
            for p in case.parts) * case.scale
    q = min(q, _unit(case.bias))
    bound = mag * case.scale + case.bias.abs().view(1, -1, 1, 1)
    if use_res:
        q = min(q, _unit(case.res_hi), _unit(case.res_lo))
        bound = bound + case.res_hi.abs() + case.res_lo.abs()
    headroom = bound.max().item() / (TWO24 * q)
    assert headroom < 1, f"case is not order-independent: headroom {headroom:.3f} (unit 2^{torch.tensor(q).log2().item():.0f})"
    ref = split_epilogue(case, acc, False, use_res)
    s = ref / q
    assert torch.equal(s, torch.round(s))
    return (F.relu(ref) if relu else ref), q, headroom


def expect_split(ref64):
    """The split-layout half tensor of the exact result ([.., C] -> [.., 2C]) through
    models.packed.to_split; the result must be an fp32 value (asserted)."""
    from idunno.models.packed import to_split

    return to_split(expect_f32(ref64))


def split_rounding_stats(ref64):
    """(fraction of outputs with v != hi + lo, fraction that are exact ties of the lo rounding)."""
    return f16_stats(ref64 - ref64.half().double())


def split_change_share(a, b):
    """Share of the outputs whose hi or lo half differs between two split tensors."""
    ah, al = split_planes(a)
    bh, bl = split_planes(b)
    return ((ah != bh) | (al != bl)).double().mean().item()


def _split_weight_ints(g, cout, cin_g, k, bs, run):
    """Scaled weights n [cout, cin_g, k, k] (float64 integers).  |n| <= 64, except:
    up to min(K/8, 48) random "wide" weights per output channel, odd |n| in [2049, 16383]
    (an odd n past 2048 is no fp16 value: lo != 0); one wide weight in every K slot
    (tap x ``bs``-channel block) s of every channel n with n % run == s % run, so that
    every run of ``run`` consecutive output channels has a non-zero w_lo in every slot;
    and one odd |n| in [8193, 16383] per channel, which pins the packer's exponent."""
    slots, K = k * k * (cin_g // bs), k * k * cin_g

    def wide(lo, *shape):
        mag = torch.randint(lo, 16384, shape, generator=g) | 1
        return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)

    n = torch.randint(-64, 65, (cout, slots, bs), generator=g)
    flat = n.view(cout, K)
    nw = min(K // 8, 48)
    flat.scatter_(1, torch.randint(0, K, (cout, nw), generator=g), wide(2048, cout, nw))    # (a few coincide)
    forced = (torch.arange(cout).view(-1, 1) % run) == (torch.arange(slots).view(1, -1) % run)
    at = torch.randint(0, bs, (cout, slots, 1), generator=g)
    n.scatter_(2, at, torch.where(forced.unsqueeze(-1), wide(2048, cout, slots, 1), n.gather(2, at)))
    flat.scatter_(1, torch.randint(0, K, (cout, 1), generator=g), wide(8192, cout, 1))
    return n.view(cout, k, k, cin_g).permute(0, 3, 1, 2).contiguous().double()


def _dense_planes(sw, cout, cin, k):
    v = sw.double().reshape(cout, k, k, cin // 32, 2, 32)
    return tuple(v[..., i, :].reshape(cout, k, k, cin).permute(0, 3, 1, 2).contiguous() for i in (0, 1))


def _grouped_planes(sw, cout, cg):
    """pack_grouped_split_weight's rows [hi 9 CB | lo 9 CB] -> planes [cout, cg, 3, 3];
    the slots outside an output's own group hold zeros (asserted)."""
    cb = max(16, cg)
    idx = ((torch.arange(cout) % cb) // cg * cg).view(-1, 1, 1) + torch.arange(cg).view(1, 1, -1)
    out = []
    for rows in (sw[:, :9 * cb], sw[:, 9 * cb:]):
        rows = rows.double().reshape(cout, 9, cb)
        own = rows.gather(2, idx.expand(cout, 9, cg))
        assert own.abs().sum() == rows.abs().sum()
        out.append(own.reshape(cout, 3, 3, cg).permute(0, 3, 1, 2).contiguous())
    return tuple(out)


def _checked(planes, w, scale):
    wh, wl = planes
    assert scale == 2.0 ** -SPLIT_E, scale
    assert torch.equal(wh + wl, w / scale), "the packer's hi + lo does not reproduce w * 2^e"
    return wh, wl


def _split_acts(g, B, C, H, W):
    """x_hi in {-4..4}, x_lo in {-2..2}/2: independent planes (a non-canonical pair)."""
    return (torch.randint(-4, 5, (B, C, H, W), generator=g).double(),
            torch.randint(-2, 3, (B, C, H, W), generator=g).double() / 2)


def _split_bias(g, cout):
    """Multiples of 1/4096 in [-1/4, 1/4]; channels n % 8 == 1 / 5 carry +- SPLIT_BIG on top."""
    n = torch.arange(cout) % 8
    big = torch.where(n == 1, SPLIT_BIG, 0.0) - torch.where(n == 5, SPLIT_BIG, 0.0)
    return torch.randint(-1024, 1025, (cout,), generator=g).double() / 4096 + big.double()


def _split_res(g, *shape):
    """res_hi in multiples of 1/4 in [-2, 2], res_lo in multiples of 2^-10 in [-1/2, 1/2]."""
    return (torch.randint(-8, 9, shape, generator=g).double() / 4,
            torch.randint(-512, 513, shape, generator=g).double() / 1024)


def _out_hw(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=2)
def split_conv_case(B, H, W, Cin, Cout, k, stride, pad, groups=1) -> SplitCase:
    """conv2d_split / conv3x3_band_split / linear_split (``groups`` 1, pack_split_weight)
    and conv3x3_grouped_split (pack_grouped_split_weight; its K slots are tap x group,
    and every output channel has a wide weight in each of its nine)."""
    from idunno.models import packed as P

    g = torch.Generator().manual_seed(case_seed("split-conv", B, H, W, Cin, Cout, k, stride, pad, groups))
    xh, xl = _split_acts(g, B, Cin, H, W)
    cg = Cin // groups
    if groups == 1:
        w = _split_weight_ints(g, Cout, Cin, k, 32, 16) / 2.0 ** SPLIT_E
        sw, scale = P.pack_split_weight(w)
        planes = _dense_planes(sw, Cout, Cin, k)
    else:
        # a wide weight in EVERY tap of every channel: where only the centre tap is inside
        # (a 1 x 1 image) K is one group's few channels, and hi*lo / lo*lo must still be live
        w = _split_weight_ints(g, Cout, cg, k, cg, 1) / 2.0 ** SPLIT_E
        sw, scale = P.pack_grouped_split_weight(w, groups)
        planes = _grouped_planes(sw, Cout, cg)
    wh, wl = _checked(planes, w, scale)
    rh, rl = _split_res(g, B, Cout, _out_hw(H, k, stride, pad), _out_hw(W, k, stride, pad))
    return SplitCase([SplitPart(xh, xl, wh, wl, stride, pad, groups)], scale, _split_bias(g, Cout), rh, rl, (w,), sw)


def split_linear_case(M, K, N) -> SplitCase:
    """linear_split as the 1x1 conv of an [M,K,1,1] input."""
    return split_conv_case(M, 1, 1, K, N, 1, 1, 0)


@functools.lru_cache(maxsize=2)
def split_dual1x1_case(B, Ho, K1, K2, Cout, stride) -> SplitCase:
    """conv1x1_dual_split: act([y | x at stride] . w^T + bias), w packed as ONE
    [Cout, K1 + K2, 1, 1] weight; parts[0] reads y [B,K1,Ho,Ho], parts[1] x [B,K2,H,H]."""
    from idunno.models import packed as P

    g = torch.Generator().manual_seed(case_seed("split-dual1x1", B, Ho, K1, K2, Cout, stride))
    H = (Ho - 1) * stride + 1 + (stride - 1)
    yh, yl = _split_acts(g, B, K1, Ho, Ho)
    xh, xl = _split_acts(g, B, K2, H, H)
    w = _split_weight_ints(g, Cout, K1 + K2, 1, 32, 16) / 2.0 ** SPLIT_E
    sw, scale = P.pack_split_weight(w)
    wh, wl = _checked(_dense_planes(sw, Cout, K1 + K2, 1), w, scale)
    parts = [SplitPart(yh, yl, wh[:, :K1].contiguous(), wl[:, :K1].contiguous(), 1, 0),
             SplitPart(xh, xl, wh[:, K1:].contiguous(), wl[:, K1:].contiguous(), stride, 0)]
    return SplitCase(parts, scale, _split_bias(g, Cout), None, None, (w,), sw)


@functools.lru_cache(maxsize=2)
def split_tail_case(B, Ho, C, Cx, stride2, H2) -> SplitCase:
    """conv2d_split_tail: act(conv3x3(y, W2) + conv1x1/stride2(x, Wd) + bias) as ONE
    accumulator over K = [nine taps of y | x's channels] (pack_split_tail_weight: one
    exponent); parts[0] reads y [B,C,Ho,Ho], parts[1] x [B,Cx,H2,H2]."""
    from idunno.models import packed as P

    g = torch.Generator().manual_seed(case_seed("split-tail", B, Ho, C, Cx, stride2, H2))
    yh, yl = _split_acts(g, B, C, Ho, Ho)
    xh, xl = _split_acts(g, B, Cx, H2, H2)
    w2 = _split_weight_ints(g, C, C, 3, 32, 16) / 2.0 ** SPLIT_E
    wd = _split_weight_ints(g, C, Cx, 1, 32, 16) / 2.0 ** SPLIT_E
    sw, scale = P.pack_split_tail_weight(w2, wd)
    w2h, w2l = _checked(_dense_planes(sw[:, :18 * C], C, C, 3), w2, scale)
    wdh, wdl = _checked(_dense_planes(sw[:, 18 * C:], C, Cx, 1), wd, scale)
    parts = [SplitPart(yh, yl, w2h, w2l, 1, 1), SplitPart(xh, xl, wdh, wdl, stride2, 0)]
    return SplitCase(parts, scale, _split_bias(g, C), None, None, (w2, wd), sw)


@functools.lru_cache(maxsize=2)
def split_down_case(B, H, C, Cout):
    """conv2d_split_dual: (main, down) = the 3x3/2 pad-1 conv and the 1x1/2 conv (its
    centre tap) of ONE input, each with its own weights, exponent and bias: the
    launch's two output ranges and two scales."""
    from idunno.models import packed as P

    g = torch.Generator().manual_seed(case_seed("split-down", B, H, C, Cout))
    xh, xl = _split_acts(g, B, C, H, H)
    cases = []
    for k, pad in ((3, 1), (1, 0)):
        w = _split_weight_ints(g, Cout, C, k, 32, 16) / 2.0 ** SPLIT_E
        sw, scale = P.pack_split_weight(w)
        wh, wl = _checked(_dense_planes(sw, Cout, C, k), w, scale)
        cases.append(SplitCase([SplitPart(xh, xl, wh, wl, 2, pad)], scale, _split_bias(g, Cout), None, None, (w,), sw))
    return tuple(cases)
