"""The split oracle (exact_ref.py, split section) qualified on the CPU, for every
case id that test_exact_split_gpu.py runs:

* the case is order-independent (headroom < 1, asserted inside ``exact_split_conv``),
  with and without the residual, and its result is an fp32 value;
* x_lo is non-zero in at least half the elements (the lo*hi term is live), and
  every K slot (tap x 32-channel block; tap x group for the grouped kernel) has a
  non-zero w_lo in every run of 16 consecutive output channels (grouped: in every
  aligned run of min(16, channels per group), i.e. inside one group), so no
  fragment of a K stage can lose its hi*lo MFMA unnoticed;
* the split store is exercised: >= 1 % of the outputs have v != hi + lo and
  >= 0.1 % are exact ties of the lo rounding -- before the ReLU, with and
  without the residual, and after the ReLU;
* fp32 arithmetic gives the contract's terms exactly (torch's own fp32 conv of
  each plane pair equals the float64 one), so the mutants below are exact too;
* eight mutants of the kernel each change >= 25 % of the outputs of the ReLU
  variant (25 % is a condition on the data, not a measurement) and are rejected
  by ``assert_bits``; the correct reference is accepted.
"""
import pytest
import torch

import exact_ref as X
import test_exact_split_gpu as GS
from test_exact_cpu import _positions

CASES = dict(GS.cpu_cases())
MIN_SHARE = 0.25


def _term(case, which, roll=False):
    """One product term of the accumulator over all parts, computed in fp32 and
    proven equal to float64 where that is cheap (the first part)."""
    total = 0.0
    for i, p in enumerate(case.parts):
        x = {"h": p.xh, "l": p.xl}[which[0]]
        w = {"h": p.wh, "l": p.wl}[which[1]]
        if roll:
            x = x.roll(1, dims=1)
        t = p.conv(x, w, torch.float32).double()
        if i == 0 and t.numel() * w[0].numel() <= 2 ** 28:
            assert torch.equal(t, p.conv(x, w))
        total = total + t
    return total


def _wlo_coverage(case):
    """Every run of output channels x every K slot holds a non-zero w_lo."""
    for p in case.parts:
        cout, cg, k, _ = p.wl.shape
        bs, run = (32, 16) if p.groups == 1 else (cg, min(16, cg))
        nz = (p.wl.permute(0, 2, 3, 1).reshape(cout, k * k * (cg // bs), bs) != 0).any(2)      # [cout, slots]
        if p.groups == 1:
            windows = nz.unfold(0, run, 1)                         # every run of 16 consecutive channels
        else:
            windows = nz.reshape(cout // run, run, -1).permute(0, 2, 1)
        if not bool(windows.any(-1).all()):
            return False
    return True


def _one_product_missing(case, ref):
    """One output without its largest |x_hi * w_hi| product."""
    p = case.parts[0]
    cg = p.wh.shape[1]
    for b, n, oh, ow in _positions(ref.shape, 1):
        if ref[b, n, oh, ow] <= 0:
            continue
        c0 = n // (p.wh.shape[0] // p.groups) * cg
        xp = torch.nn.functional.pad(p.xh[b, c0:c0 + cg], (p.pad,) * 4)
        k = p.wh.shape[2]
        prods = (xp[:, oh * p.stride:oh * p.stride + k, ow * p.stride:ow * p.stride + k] * p.wh[n]).flatten()
        d = -prods[prods.abs().argmax()].item() * case.scale
        if d != 0 and ref[b, n, oh, ow] + d > 0:
            m = ref.clone()
            m[b, n, oh, ow] += d
            return m
    raise AssertionError("no positive output with a non-zero product")


def _rejected(y, expect, ref, lo_rounding=None):
    with pytest.raises(AssertionError) as e:
        X.assert_bits(y, expect, ref, split=True)
    msg = str(e.value)
    assert "halfs differ" in msg and " plane, channel " in msg and "pixel (b, h, w)" in msg and "exact value" in msg, msg
    if lo_rounding is not None:
        assert ("all within one fp16 ulp of the lo plane" in msg and "NOT" not in msg) == lo_rounding, msg


@pytest.mark.parametrize("cid", sorted(CASES))
def test_split_case_qualifies(cid):
    c = CASES[cid]()
    has_res = c.res_hi is not None
    plain, q, headroom = X.exact_split_conv(c, False, False)        # headroom < 1 and the grid asserted inside
    assert headroom < 1
    full = plain
    if has_res:
        full, _, headroom = X.exact_split_conv(c, False, True)
        assert headroom < 1
    print(f"{cid}: unit 2^{torch.tensor(q).log2().item():.0f}, headroom {headroom:.3f}")

    for p in c.parts:
        assert (p.xl != 0).double().mean().item() >= 0.5
        for t in (p.xh, p.xl, p.wh, p.wl):
            assert torch.equal(t.half().double(), t)
    assert _wlo_coverage(c)

    relu_full = torch.relu(full)
    for ref in (plain, full, relu_full):
        inexact, ties = X.split_rounding_stats(ref)
        assert inexact >= 0.01, (cid, inexact)
        assert ties >= 0.001, (cid, ties)
    assert 0.4 <= (full > 0).double().mean().item() <= 0.6

    # the contract, term by term, in fp32 == float64
    hh, hl, lh, ll = (_term(c, t) for t in ("hh", "hl", "lh", "ll"))
    acc = c.terms()[0]
    assert torch.equal(hh + hl + lh, acc)

    ref = X.nhwc(relu_full)
    # N = 1000 (the logits layer) has no split form: its kernel stores fp32 only
    split_out = ref.shape[-1] % 32 == 0
    e32 = X.expect_f32(ref)
    X.assert_bits(e32.clone(), e32, ref)
    if split_out:
        expect = X.expect_split(ref)
        X.assert_bits(expect.clone(), expect, ref, split=True)

    def out(a, **kw):
        return X.nhwc(X.split_epilogue(c, a, True, has_res, **kw))

    def share_and_reject(m):
        """The share of outputs that mutant ``m`` changes; it must be rejected in both output forms."""
        with pytest.raises(AssertionError, match="elements differ"):
            X.assert_bits(X.expect_f32(m), e32, ref)
        if not split_out:
            return (X.expect_f32(m) != e32).double().mean().item()
        _rejected(X.expect_split(m), expect, ref)
        return X.split_change_share(X.expect_split(m), expect)

    swapped = c.bias.view(-1, 2).flip(1).reshape(-1)                # bias of channel n at channel n ^ 1
    mutants = {
        "lo*hi dropped": out(acc - lh),
        "hi*lo dropped": out(acc - hl),
        "lo*lo added": out(acc + ll),
        "x_lo of the neighbouring channel": out(acc - lh + _term(c, "lh", roll=True)),
        "bias of channel n ^ 1": out(acc, bias=swapped),
    }
    if has_res:
        mutants["res_lo skipped"] = out(acc, res_lo=False)
    shares = {name: share_and_reject(m) for name, m in mutants.items()}
    # one product missing at one output: one output differs, and is reported
    assert share_and_reject(X.nhwc(_one_product_missing(c, relu_full))) * ref.numel() == pytest.approx(1.0)
    assert min(shares.values()) >= MIN_SHARE, (cid, shares)
    if split_out:
        # the split store with lo = fp16(v) - hi taken in half arithmetic: v is rounded to
        # half BEFORE the subtraction, so what the lo half should carry is lost
        hi = ref.half()
        half_lo = X.split_layout(hi, hi - ref.half())
        shares["lo computed in half"] = X.split_change_share(half_lo, expect)
        assert shares["lo computed in half"] >= MIN_SHARE, (cid, shares)
        _rejected(half_lo, expect, ref)
        # a lo half one ulp off is named as the lo rounding, a hi half is not
        lo_off = expect.clone()
        first_lo = lo_off.view(-1)[32:33]
        first_lo.copy_((first_lo.view(torch.int16) ^ 1).view(torch.float16))
        _rejected(lo_off, expect, ref, lo_rounding=True)
        hi_off = expect.clone()
        first_hi = hi_off.view(-1)[0:1]
        first_hi.copy_((first_hi.view(torch.int16) ^ 1).view(torch.float16))
        _rejected(hi_off, expect, ref, lo_rounding=False)
    print(f"{cid}: smallest mutant share {min(shares.values()):.3f} ({min(shares, key=shares.get)})")


def test_split_layout_roundtrip_and_packed_to_split():
    """split_layout / split_planes are each other's inverse and agree with models.packed.to_split."""
    from idunno.models.packed import from_split, to_split

    g = torch.Generator().manual_seed(3)
    v = torch.randn(2, 3, 5, 96, generator=g) * 7
    s = to_split(v)
    hi, lo = X.split_planes(s)
    assert torch.equal(hi, v.half()) and torch.equal(lo, (v - v.half().float()).half())
    assert torch.equal(X.split_layout(hi, lo), s)
    assert torch.equal(from_split(s), hi.float() + lo.float())


def test_split_rounding_stats_on_hand_made_values():
    """2049 = 2048 + 1 and 100 + 2^-12 are exact; 2049 + 2^-12 = 2050 - (1 - 2^-12) needs a
    12th bit of lo (a tie); past hi = 1 a lo below 2^-14 keeps multiples of 2^-24:
    3 * 2^-25 is a tie, 5 * 2^-26 is inexact and no tie."""
    ref = torch.tensor([2049.0, 100.0 + 2.0 ** -12, 2049.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -25, 1.0 + 5 * 2.0 ** -26],
                       dtype=torch.float64)
    inexact, ties = X.split_rounding_stats(ref)
    assert inexact == 3 / 5 and ties == 2 / 5
