"""Exact cases of the fused layer-1 block, composed from the arithmetic-contract oracle of
exact_ref.py: conv a's exact result, rounded to the split planes as the kernel stores it,
is conv b's input, and x's NON-CANONICAL planes are conv b's residual.

exact_ref.split_conv_case cannot be chained as it is, and the numbers say why: its conv a
result is a multiple of 2^-12 (x_lo unit 1/2 times weight unit 2^-11) and reaches
SPLIT_BIG = 2304 on every eighth channel, so conv b's unit would be 2^-12 * 2^-11 = 2^-23
and its window 2^24 * 2^-23 = 2, while its terms' magnitudes sum to 72 * 2304 * 64 / 2048 =
5184 from the ordinary weights alone: headroom ~2600 where the assertion needs < 1.  The
cases here keep the same operand kinds on coarser grids, and both pass
exact_ref.exact_split_conv's own headroom and integrality assertions (SplitCase.ref):

  "wide_a"  conv a: every second weight in {+-1/2, +-1} and per output channel 24 wide weights
            +-2049/1024 (scaled 8196 = hi 8192 + lo 4): x_hi*w_lo and x_lo*w_hi are live in
            conv a, y is a multiple of 2^-10 with up to 18 significant bits, so y_lo != 0.
            That leaves conv b 6 bits: exact_ref counts a weight plane's unit as at most 2^8
            of the 2^14 scale, so its weights are +-1/64 (scaled 256), one in four, and one
            3/4 that pins the exponent (w_lo = 0): unit 2^-16, window 256.
  "wide_b"  conv a coarse (y a multiple of 1/4, y_lo = 0); conv b +-1/16, one in eight, and 4
            wide weights per output channel: y_hi*w_lo is live in conv b; unit 2^-12, window 4096.

In both the residual is x_hi in {-4..4} plus x_lo in {-2..2}/2, independent planes.  The
+-SPLIT_BIG biases of exact_ref (the split store's 24th-bit rounding) do not fit these
windows; y's store rounds nothing here (y has at most 18 bits), conv b's neither.
"""
import functools

import torch

import exact_ref as X

WIDE = 2049.0 / 1024.0


def _weights(g, step, levels, density_den, nwide=0, pin=0.0):
    """[64, 64, 3, 3] float64: multiples of ``step`` up to ``levels`` steps, one in
    ``density_den`` non-zero; ``nwide`` weights +-WIDE per output channel; ``pin`` (if set)
    one weight of the tensor, which fixes the packer's exponent."""
    w = torch.randint(-levels, levels + 1, (64, 64, 3, 3), generator=g).double() * step
    if density_den > 1:
        w = w * (torch.randint(0, density_den, w.shape, generator=g) == 0)
    flat = w.view(64, -1)
    if nwide:
        at = torch.randint(0, flat.shape[1], (64, nwide), generator=g)
        sign = (torch.randint(0, 2, (64, nwide), generator=g) * 2 - 1).double()
        flat.scatter_(1, at, sign * WIDE)
    if pin:
        flat[7, 300] = pin
    return w


def _packed(w):
    from idunno.models import packed as P

    sw, scale = P.pack_split_weight(w)
    wh, wl = X._dense_planes(sw, 64, 64, 3)
    assert torch.equal(wh + wl, w / scale), "the packer's hi + lo does not reproduce w * 2^e"
    return sw, scale, wh, wl


@functools.lru_cache(maxsize=4)
def block_case(kind, B, H, W):
    """(case_a, case_b, x in the split layout, expected out in the split layout, ref64 NHWC)."""
    g = torch.Generator().manual_seed(X.case_seed("c64-block", kind, B, H, W))
    xh, xl = X._split_acts(g, B, 64, H, W)
    wa = _weights(g, 0.5, 2, 2, 24) if kind == "wide_a" else _weights(g, 0.5, 2, 2)
    wb = _weights(g, 1.0 / 64, 1, 4, pin=0.75) if kind == "wide_a" else _weights(g, 1.0 / 16, 1, 8, 4)
    ba = torch.randint(-8, 9, (64,), generator=g).double() / 4
    bb = torch.randint(-8, 9, (64,), generator=g).double() / 4
    swa, sa, wah, wal = _packed(wa)
    case_a = X.SplitCase([X.SplitPart(xh, xl, wah, wal, 1, 1)], sa, ba, None, None, (wa,), swa)
    y = case_a.ref(True, False)                          # asserts conv a's headroom
    yh, yl = X.split_planes(X.expect_split(X.nhwc(y)))   # NHWC planes, as the kernel stores y
    yh, yl = (t.double().permute(0, 3, 1, 2).contiguous() for t in (yh, yl))
    assert torch.equal(yh + yl, y), "y does not fit its split planes"
    swb, sb, wbh, wbl = _packed(wb)
    case_b = X.SplitCase([X.SplitPart(yh, yl, wbh, wbl, 1, 1)], sb, bb, xh, xl, (wb,), swb)
    ref = X.nhwc(case_b.ref(True, True))                 # asserts conv b's headroom, residual included
    if kind == "wide_a":
        assert bool(wal.any()) and bool(yl.any()) and not bool(wbl.any())
    else:
        assert bool(wbl.any()) and not bool(wal.any())
    return case_a, case_b, X.split_layout(X.nhwc(xh), X.nhwc(xl)), X.expect_split(ref), ref


KINDS = ("wide_a", "wide_b")
SHAPES = [(3, 13, 49), (1, 9, 52), (2, 5, 56)]
