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


def _conv_parts(x, w, stride, pad, wino):
    """(conv(x, w), bound on the magnitudes any summation order can reach, the
    products' unit), float64.
    One entry is kept, keyed by the operands' storage, so the ReLU / residual
    variants of one case share one reference."""
    key = (x.data_ptr(), w.data_ptr(), tuple(x.shape), tuple(w.shape), stride, pad, wino)
    if _memo.get("key") != key:
        acc = F.conv2d(x, w, None, stride, pad)
        mag = F.conv2d(x.abs(), w.abs(), None, stride, pad).max().item()
        if wino:
            assert w.shape[2:] == (3, 3) and stride == 1 and pad == 1
            u, v = _wino_terms(x, w)
            m = torch.einsum("koc,bckt->bokt", u.abs(), v.abs())            # sum over Cin of |U||V|
            m = m.reshape(x.shape[0], -1, 4, 4, v.shape[-1])
            mag = max(mag, torch.einsum("pi,boijt,qj->bopqt", _AT.abs(), m, _AT.abs()).max().item())
        _memo.clear()
        _memo.update(key=key, x=x, w=w, acc=acc, mag=mag, q=_unit(x) * _unit(w) * (0.25 if wino else 1.0))
    return _memo["acc"], _memo["mag"], _memo["q"]


def exact_conv(x, w, bias, stride, pad, relu, residual=None, *, wino=False):
    """(ref64 [B,Cout,Ho,Wo], unit q, headroom).  Every term and partial sum of
    the conv is a multiple of q; headroom = max(conv(|x|,|w|) + |bias| + |res|) /
    (2^24 q) < 1 (asserted) proves that fp32 accumulation in any order is exact,
    so a case that fails it is wrong, not flaky.  ``wino``: q shrinks by the 1/4
    of G g G^T, and the bound is |U|.|V| summed over Cin through the output
    transform.  Dual [y | x] GEMMs and linear layers are 1x1 convs here
    (``dual_input``; [M,K,1,1])."""
    acc, mag, q = _conv_parts(x, w, stride, pad, wino)
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


def assert_bits(y, expect, ref64=None):
    """torch.equal on CPU copies of NHWC tensors.  On failure: the number of
    differing elements, the first few NHWC indices with got / want / the float64
    value, and whether every difference is within one ulp of the output type
    (a rounding fault) or not (an arithmetic fault)."""
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

    def ref(self, relu, use_res):
        """The exact result (NCHW float64) of this case."""
        return exact_conv(self.x, self.w, self.bias, self.stride, self.pad, relu,
                          self.res if use_res else None, wino=self.wino)[0]


@functools.lru_cache(maxsize=2)
def conv_case(B, H, W, Cin, Cout, k, stride, pad, coarse=False, wino=False) -> Case:
    seed = case_seed("conv", B, H, W, Cin, Cout, k, stride, pad, coarse)
    x, w, b, r = grid_conv_case(B, H, W, Cin, Cout, k, stride, pad, True, seed, coarse=coarse)
    return Case(x, w, b, r, stride, pad, wino, coarse)


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
