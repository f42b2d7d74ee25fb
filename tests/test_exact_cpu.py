"""The bit-exact oracle (exact_ref.py) qualified on the CPU, for every case the
GPU files test_exact_f16_gpu.py / test_exact_f32_gpu.py run:

* the case is order-independent (headroom < 1, asserted inside ``exact_conv``);
* its outputs exercise fp16 rounding (>= 1 % not representable) and
  ties-to-even (>= 0.1 % exact ties) -- conditions on the data; the coarse first
  stages of conv1x1_fused_next are the stated exception (every output IS an
  fp16 value, so the second stage's input is exact);
* torch's own fp32 conv of the same data equals the float64 reference bit for
  bit, and so does an fp32 emulation of F(2x2,3x3) Winograd, whose filter
  transform ``models.packed.wino_weight`` equals the float64 G g G^T;
* five mutants of the reference are each rejected by ``assert_bits`` and the
  correctly rounded reference is accepted.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import test_exact_f16_gpu as G16
import test_exact_f32_gpu as G32

CASES = dict(G32.cpu_cases())
CASES.update(G16.cpu_cases())          # same id = same data


def _ulp16(v: float) -> float:
    v = abs(v)
    return 2.0 ** -24 if v == 0 else 2.0 ** (max(math.floor(math.log2(v)), -14) - 10)


def _moves_f16(o: float, d: float) -> bool:
    """o -> o + d crosses at least four fp16 ulps of either value: the two roundings
    differ by more than one ulp (an arithmetic fault in assert_bits' report)."""
    return abs(d) >= 4 * max(_ulp16(o), _ulp16(o + d))


def _positions(shape, seed, n=4096):
    g = torch.Generator().manual_seed(seed)
    total = math.prod(shape)
    for f in torch.randint(0, total, (n,), generator=g).tolist():
        idx = []
        for s in reversed(shape):
            idx.append(f % s)
            f //= s
        yield tuple(reversed(idx))


def mutant_missing_product(c, ref):
    """One output without its largest-|x w| product (>= 4 fp16 ulps there, picked so)."""
    k, s, p = c.w.shape[2], c.stride, c.pad
    cg = c.w.shape[1]                                          # input channels of one group (all of them at groups = 1)
    for b, n, oh, ow in _positions(ref.shape, 1):
        c0 = n // (c.w.shape[0] // c.groups) * cg
        patch = F.pad(c.x[b, c0:c0 + cg], (p, p, p, p))[:, oh * s:oh * s + k, ow * s:ow * s + k]
        prods = (patch * c.w[n]).flatten()
        d = -prods[prods.abs().argmax()].item()
        if _moves_f16(ref[b, n, oh, ow].item(), d):
            m = ref.clone()
            m[b, n, oh, ow] += d
            return m
    raise AssertionError("no output whose largest product reaches four fp16 ulps")


def mutant_swapped_bias(c, ref):
    """Bias of channel n applied to channel n ^ 1 at one pixel."""
    pair = c.bias.view(-1, 2)
    n = 2 * int((pair[:, 0] - pair[:, 1]).abs().argmax())
    d = (c.bias[n ^ 1] - c.bias[n]).item()
    for b, _n, oh, ow in _positions(ref.shape, 2):
        if _moves_f16(ref[b, n, oh, ow].item(), d):
            m = ref.clone()
            m[b, n, oh, ow] += d
            return m
    raise AssertionError("no pixel where the neighbour's bias moves the output by four fp16 ulps")


def mutant_residual_after_rounding(c):
    """half(half(acc + b) + r) instead of half(acc + b + r)."""
    return (c.ref(False, False).half().double() + c.res).half()


def mutant_toward_zero(ref):
    h, o = X.f16_other_neighbour(ref)
    return torch.where(h.double().abs() > ref.abs(), o, h)


def mutant_ties_away(ref):
    h, o = X.f16_other_neighbour(ref)
    tie = (h.double() != ref) & ((h.double() - ref).abs() == (o.double() - ref).abs())
    return torch.where(tie & (o.double().abs() > h.double().abs()), o, h)


def _rejected(y, expect, ref, within_one_ulp):
    with pytest.raises(AssertionError) as e:
        X.assert_bits(y, expect, ref)
    msg = str(e.value)
    assert "elements differ" in msg and "got" in msg and "want" in msg and "exact" in msg
    if within_one_ulp is not None:
        assert ("all within one" in msg and "NOT" not in msg) == within_one_ulp, msg


@pytest.mark.parametrize("cid", sorted(CASES))
def test_case_qualifies(cid):
    c = CASES[cid]()
    plain, full = c.ref(False, False), c.ref(False, True)      # pre-ReLU; headroom < 1 asserted inside
    _, q, headroom = X.exact_conv(c.x, c.w, c.bias, c.stride, c.pad, False, c.res, wino=c.wino, groups=c.groups)
    assert headroom < 1

    # fp32 arithmetic is exact on this data, whatever the order: torch's own conv, and Winograd
    y32 = F.conv2d(c.x.float(), c.w.float(), c.bias.float(), c.stride, c.pad, groups=c.groups)
    assert torch.equal(y32.double(), plain)
    if c.wino:
        from idunno.models.packed import wino_weight

        assert torch.equal(wino_weight(c.w.float()).double(), X.wino_u(c.w))
        assert torch.equal(X.wino_emulate(c.x, c.w).double() + c.bias.view(1, -1, 1, 1), plain)

    for ref in (plain, full):
        inexact, ties = X.f16_stats(ref)
        if c.coarse:
            assert inexact == 0 and ref.abs().max().item() < 32
        else:
            assert inexact >= 0.01, (cid, inexact)
            assert ties >= 0.001, (cid, ties)

    # the correctly rounded reference is accepted; the mutants are not
    e16, e32 = X.expect_f16(full), X.expect_f32(full)
    X.assert_bits(e16.clone(), e16, full)
    X.assert_bits(e32.clone(), e32, full)
    for m in (mutant_missing_product(c, full), mutant_swapped_bias(c, full)):
        _rejected(X.expect_f16(m), e16, full, False)
        _rejected(X.expect_f32(m), e32, full, False)
    if c.coarse:
        return                                                 # nothing is rounded: mutants 2-4 are the reference
    if c.res is not None:
        # (more than one ulp where the residual cancels most of the rounded sum)
        _rejected(mutant_residual_after_rounding(c), e16, full, None)
    _rejected(mutant_toward_zero(full), e16, full, True)
    _rejected(mutant_ties_away(full), e16, full, True)


def test_assert_bits_flags_nan_and_dtype():
    a = torch.tensor([1.0, 2.0]).half()
    X.assert_bits(a, a.clone())
    with pytest.raises(AssertionError, match="non-finite"):
        X.assert_bits(torch.tensor([1.0, float("nan")]).half(), a)
    with pytest.raises(AssertionError):
        X.assert_bits(a.float(), a)


def test_rounding_helpers():
    """ties-to-even, the other neighbour and the tie count on hand-made values."""
    ref = torch.tensor([2049.0, 2051.0, -2049.0, 0.5 + 2.0 ** -12, 1.0, 2048.5, 0.0], dtype=torch.float64)
    h, o = X.f16_other_neighbour(ref)
    assert h.tolist() == [2048.0, 2052.0, -2048.0, 0.5, 1.0, 2048.0, 0.0]
    assert o.tolist() == [2050.0, 2050.0, -2050.0, 0.5 + 2.0 ** -11, 1.0, 2050.0, 0.0]
    inexact, ties = X.f16_stats(ref)
    assert inexact == 5 / 7 and ties == 4 / 7
    assert mutant_toward_zero(ref).tolist() == [2048.0, 2050.0, -2048.0, 0.5, 1.0, 2048.0, 0.0]
    assert mutant_ties_away(ref).tolist() == [2050.0, 2052.0, -2050.0, 0.5 + 2.0 ** -11, 1.0, 2048.0, 0.0]
