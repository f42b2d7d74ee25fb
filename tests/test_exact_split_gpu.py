"""Bit-exact checks of the split-fp16 conv / FC kernels (exact_ref.py, split section).

A split kernel computes sum x_hi*w_hi + x_hi*w_lo + x_lo*w_hi (no lo*lo) in
f32, then acc * 2^-e + bias (+ res_hi + res_lo), ReLU, and stores fp32 or
hi = fp16(v), lo = fp16(v - hi).  On the grid data of exact_ref.py every f32
accumulation order is exact, so each kernel must return the float64 value of
that expression: ``torch.equal`` on both planes, no tolerance.

The activation and residual pairs are NON-CANONICAL on purpose (x_hi a small
integer, x_lo an independent small dyadic value): a canonical pair cannot fit
fp32's 24-bit window at a real K, and the kernels read the pair as two
independent planes.  The weights go through the real packers.  The tolerance
tests on randn data keep covering canonical pairs; the case lists here are
theirs (imported), so both suites walk the same shapes -- a shape that is only
large is replaced by the small one that reaches the same code.
test_exact_split_cpu.py qualifies every case id of this file on the CPU.
"""
import pathlib
import re

import pytest
import torch

import exact_ref as X
import test_band as TB
import test_grouped_gpu as TG
import test_split as TS
import test_split_tail as TT

DEV = "cuda"
_CSRC = pathlib.Path(TS.P.__file__).resolve().parent.parent / "csrc"


def _table_tiles(fn):
    """The tile ids that dispatch table ``fn`` of conv_glds.hip accepts."""
    text = (_CSRC / "kernels" / "conv_glds.hip").read_text()
    body = text[text.index(f"static bool {fn}("):]
    return sorted({int(t) for t in re.findall(r"case (\d+):", body[:body.index("default:")])})


SPLIT_CASES = TS.SPLIT_CASES                                                      # (B, H, Cin, Cout, k, s, p)
TILES = _table_tiles("glds_dispatch_split")
assert set(TS.SPLIT_TILES) <= set(TILES) and len(TILES) >= 6, TILES
KS_TILES = _table_tiles("glds_dispatch_ks")                                       # the split-K instantiations
TILE_CASE = (3, 13, 128, 192, 3, 1, 1)                                            # M = 507, Cout 192: partial tiles
# every route bit the binding knows (binding_util.cpp), one at a time, and none
ROUTES = [0] + sorted(int(v) for v in re.findall(r"kRoute\w+ = (\d+)", (_CSRC / "binding_util.cpp").read_text()))
assert len(ROUTES) == 8, ROUTES
# the shapes that a route bit re-routes: layer-1 rows, band (W 28 / 7), streaming 1x1 (large and small M)
ROUTE_CASES = [TILE_CASE, (2, 49, 64, 64, 3, 1, 1), (2, 28, 128, 128, 3, 1, 1), (5, 7, 512, 512, 3, 1, 1),
               (6, 56, 64, 128, 1, 1, 0), (2, 14, 256, 512, 1, 2, 0)]
STREAM_CASES = sorted({c[:5] for c in X.parametrize_args(TS.test_conv_split_1x1_stream, "B")})    # (B, H, Cin, Cout, s)
assert len(STREAM_CASES) == 12
# (160, 56, 56) and (40, 56, 56) are only large; (150, 13, 52) is the many-row case
ROWS_CASES = [c for c in X.parametrize_args(TS.test_conv_split_c64_rows, "B") if c[0] < 40 or c[1] < 56]
assert ROWS_CASES == [(2, 56, 56), (3, 13, 49), (1, 9, 52), (150, 13, 52)]
KSPLIT_CASES = X.parametrize_args(TS.test_conv_split_ksplit, "B")                 # (B, H, Cin, Cout, k, s, ks)
DUAL1X1_CASES = X.parametrize_args(TS.test_conv1x1_dual_split, "B")               # (B, Ho, K1, K2, Cout, s)
DOWN_CASES = X.parametrize_args(TS.test_conv_split_dual_downsample, "B")          # (B, H, C, Cout, tile)
TAIL_CASES = TT.TAIL_CASES                                                        # (B, Ho, C, Cx, s2, tile, H2)
BAND_CASES = TB.BAND_CASES                                                        # (B, H, Cin, Cout)
# test_linear_split's (M, K, N) with M 500 cut to 7 / 170 (one partial and two 160-row tiles)
LINEAR_CASES = [(7, 9216, 4096), (170, 4096, 1000), (7, 512, 96), (33, 1024, 256)]
assert [(K, N) for _, K, N in LINEAR_CASES] == [c[1:3] for c in X.parametrize_args(TS.test_linear_split, "M")]
LINEAR_SPLITS = [None, 1, 2, 4, 8]
GROUPED_CASES = TG.CASES                                                          # (B, H, W, C, groups, stride)
SLICE_CASES = [(2, 14, 256, 256, 3, 1, 1), (2, 14, 1024, 256, 1, 1, 0)]


def _conv(B, H, Cin, Cout, k, s, p, W=None):
    return X.split_conv_case(B, H, H if W is None else W, Cin, Cout, k, s, p)


def cpu_cases():
    """(id, thunk -> SplitCase) of every distinct data set the tests below run."""
    cs = {}
    convs = SPLIT_CASES + [TILE_CASE] + ROUTE_CASES + SLICE_CASES
    convs += [(B, H, Cin, Cout, 1, s, 0) for B, H, Cin, Cout, s in STREAM_CASES]
    convs += [(B, H, Cin, Cout, k, s, k // 2) for B, H, Cin, Cout, k, s, _ks in KSPLIT_CASES]
    convs += [(B, H, Cin, Cout, 3, 1, 1) for B, H, Cin, Cout in BAND_CASES]
    for c in convs:
        cs[f"conv{c}"] = lambda a=c: _conv(*a)
    for B, H, W in ROWS_CASES:
        cs[f"rows{(B, H, W)}"] = lambda a=(B, H, 64, 64, 3, 1, 1, W): _conv(*a)
    for c in DUAL1X1_CASES:
        cs[f"dual1x1{c}"] = lambda a=c: X.split_dual1x1_case(*a)
    for B, H, C, Cout, _tile in DOWN_CASES:
        cs[f"down-main{(B, H, C, Cout)}"] = lambda a=(B, H, C, Cout): X.split_down_case(*a)[0]
        cs[f"down-1x1{(B, H, C, Cout)}"] = lambda a=(B, H, C, Cout): X.split_down_case(*a)[1]
    for B, Ho, C, Cx, s2, _tile, H2 in TAIL_CASES:
        cs[f"tail{(B, Ho, C, Cx, s2, H2)}"] = lambda a=(B, Ho, C, Cx, s2, H2): X.split_tail_case(*a)
    for c in LINEAR_CASES:
        cs[f"linear{c}"] = lambda a=c: X.split_linear_case(*a)
    for B, H, W, C, groups, stride in GROUPED_CASES:
        cs[f"grouped{(B, H, W, C, groups, stride)}"] = \
            lambda a=(B, H, W, C, C, 3, stride, 1, groups): X.split_conv_case(*a)
    return sorted(cs.items())


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def guard(ops):
    """The range guard flag around the whole module: no exact case may raise it
    (test_guard_flag_stayed_zero, the module's last test, reads it)."""
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.set_split_guard(flag)
    try:
        yield flag
    finally:
        ops.set_split_guard(None)


def _s(hi, lo):
    """NCHW float64 planes -> the NHWC split layout on the GPU (lossless, asserted)."""
    return None if hi is None else X.split_layout(X.nhwc(hi), X.nhwc(lo)).to(DEV)


def _b(bias):
    return bias.float().to(DEV)


def _variants(case, calls, res=(False, True), relus=(True, False), f32=False):
    """``call(relu, residual in the split layout or None)`` (one, or a dict of
    labelled ones that share the reference) against the exact result, for every
    ReLU / residual combination; all mismatches are reported together."""
    if callable(calls):
        calls = {"": calls}
    fails = []
    r = _s(case.res_hi, case.res_lo) if True in res else None
    for use_res in res:
        for relu in relus:
            ref = X.nhwc(case.ref(relu, use_res))
            expect = X.expect_f32(ref) if f32 else X.expect_split(ref)
            for label, call in calls.items():
                y = call(relu, r if use_res else None)
                try:
                    X.assert_bits(y, expect, ref, split=not f32)
                except AssertionError as e:
                    fails.append(f"{label} residual={use_res} relu={relu} out_f32={f32}: {e}")
    assert not fails, "\n".join(fails)


def _operands(c):
    p = c.parts[0]
    return _s(p.xh, p.xl), c.sw.to(DEV), _b(c.bias)


def _both_outputs(c, call, **kw):
    """``call(relu, r, out_f32)`` into the split layout and into fp32."""
    for f32 in (False, True):
        _variants(c, lambda relu, r: call(relu, r, f32), f32=f32, **kw)


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", SPLIT_CASES)
def test_conv_split_default_tile_exact(ops, B, H, Cin, Cout, k, s, p):
    c = _conv(B, H, Cin, Cout, k, s, p)
    x, w, b = _operands(c)
    _both_outputs(c, lambda relu, r, f32: ops.conv2d_split(x, w, b, c.scale, k, k, s, p, relu, residual=r, out_f32=f32))


@pytest.mark.parametrize("tile", TILES)
def test_conv_split_all_tiles_exact(ops, tile):
    c = _conv(*TILE_CASE)
    x, w, b = _operands(c)
    _both_outputs(c, lambda relu, r, f32: ops.conv2d_split(x, w, b, c.scale, 3, 3, 1, 1, relu, residual=r, out_f32=f32,
                                                         tile=tile))


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", ROUTE_CASES)
def test_conv_split_routes_exact(ops, B, H, Cin, Cout, k, s, p):
    """Whatever kernel a route value selects gives the same bits."""
    c = _conv(B, H, Cin, Cout, k, s, p)
    x, w, b = _operands(c)
    for f32 in (False, True):
        _variants(c, {f"route {rt}": lambda relu, r, rt=rt: ops.conv2d_split(x, w, b, c.scale, k, k, s, p, relu,
                                                                             residual=r, out_f32=f32, route=rt)
                      for rt in ROUTES}, f32=f32)


@pytest.mark.parametrize("B,H,Cin,Cout,s", STREAM_CASES)
def test_conv_split_1x1_stream_exact(ops, B, H, Cin, Cout, s):
    """Tile 80 (conv1x1_stream.hip SPLIT)."""
    c = _conv(B, H, Cin, Cout, 1, s, 0)
    x, w, b = _operands(c)
    _variants(c, lambda relu, r: ops.conv2d_split(x, w, b, c.scale, 1, 1, s, 0, relu, residual=r, tile=80))


@pytest.mark.parametrize("B,H,W", ROWS_CASES)
def test_conv_split_c64_rows_exact(ops, B, H, W):
    """Tile 50 (conv3x3_split.hip): one-row bands, and at B = 150 two-row bands whose
    shares of rows cross images; both workgroup-per-CU forms."""
    c = _conv(B, H, 64, 64, 3, 1, 1, W)
    x, w, b = _operands(c)
    _variants(c, {f"route {rt}": lambda relu, r, rt=rt: ops.conv2d_split(x, w, b, c.scale, 3, 3, 1, 1, relu, residual=r,
                                                                         tile=50, route=rt) for rt in (0, 16)})


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,ks", KSPLIT_CASES)
def test_conv_split_ksplit_exact(ops, B, H, Cin, Cout, k, s, ks):
    """K slices into fp32 partials + one combine (bias, residual, ReLU, re-split)."""
    c = _conv(B, H, Cin, Cout, k, s, k // 2)
    x, w, b = _operands(c)
    _both_outputs(c, lambda relu, r, f32: ops.conv2d_split(x, w, b, c.scale, k, k, s, k // 2, relu, residual=r,
                                                         out_f32=f32, ksplit=ks))


@pytest.mark.parametrize("tile", KS_TILES)
def test_conv_split_ksplit_tiles_exact(ops, tile):
    """Every split-K instantiation (glds_dispatch_ks), three slices of the nine taps."""
    c = _conv(2, 9, 128, 256, 3, 1, 1)
    x, w, b = _operands(c)
    _both_outputs(c, lambda relu, r, f32: ops.conv2d_split(x, w, b, c.scale, 3, 3, 1, 1, relu, residual=r, out_f32=f32,
                                                         tile=tile, ksplit=3))


@pytest.mark.parametrize("B,Ho,K1,K2,Cout,s", DUAL1X1_CASES)
def test_conv1x1_dual_split_exact(ops, B, Ho, K1, K2, Cout, s):
    c = X.split_dual1x1_case(B, Ho, K1, K2, Cout, s)
    y, x = (_s(p.xh, p.xl) for p in c.parts)
    w, b = c.sw.to(DEV), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv1x1_dual_split(y, x, w, b, c.scale, s, relu), res=(False,))


@pytest.mark.parametrize("B,H,C,Cout,tile", DOWN_CASES)
def test_conv_split_dual_downsample_exact(ops, B, H, C, Cout, tile):
    """One launch, two output ranges: the 3x3/2 conv (ReLU, its scale) and the 1x1/2
    downsample on the centre tap (no ReLU, its own scale)."""
    main, down = X.split_down_case(B, H, C, Cout)
    x = _s(main.parts[0].xh, main.parts[0].xl)
    c2 = main.sw.shape[1] // 9
    wd = torch.zeros(2 * Cout, main.sw.shape[1], dtype=torch.float16)
    wd[:Cout] = main.sw
    wd[Cout:, 4 * c2:5 * c2] = down.sw
    wd, b = wd.to(DEV), _b(torch.cat([main.bias, down.bias]))
    down_ref = X.nhwc(down.ref(False, False))
    fails = []
    for relu in (True, False):
        both = ops.conv2d_split_dual(x, wd, b, main.scale, down.scale, Cout, 3, 3, 2, 1, relu, tile=tile)
        main_ref = X.nhwc(main.ref(relu, False))
        for name, got, ref in (("3x3", both[..., :2 * Cout], main_ref), ("1x1", both[..., 2 * Cout:], down_ref)):
            try:
                X.assert_bits(got.contiguous(), X.expect_split(ref), ref, split=True)
            except AssertionError as e:
                fails.append(f"{name} relu={relu}: {e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,Ho,C,Cx,s2,tile,H2", TAIL_CASES)
def test_conv_split_tail_exact(ops, B, Ho, C, Cx, s2, tile, H2):
    """conv3x3(y) + conv1x1/s2(x2) in ONE accumulator."""
    c = X.split_tail_case(B, Ho, C, Cx, s2, H2)
    y, x = (_s(p.xh, p.xl) for p in c.parts)
    w, b = c.sw.to(DEV), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d_split_tail(y, x, w, b, c.scale, s2, relu, tile=tile), res=(False,))


@pytest.mark.parametrize("max_grid", [0, 3])
@pytest.mark.parametrize("B,H,Cin,Cout", BAND_CASES)
def test_conv3x3_band_split_exact(ops, B, H, Cin, Cout, max_grid):
    """conv3x3_band.hip, free and capped persistent grid (a workgroup runs several tiles)."""
    c = _conv(B, H, Cin, Cout, 3, 1, 1)
    x, w, b = _operands(c)
    ext = ops.load()
    _both_outputs(c, lambda relu, r, f32: ext.conv3x3_band_split(x, w, b, r, relu, c.scale, f32, max_grid))


@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
@pytest.mark.parametrize("splits", LINEAR_SPLITS)           # innermost: one case's splits run back to back
def test_linear_split_exact(ops, M, K, N, splits):
    c = X.split_linear_case(M, K, N)
    p = c.parts[0]
    x = X.split_layout(p.xh.view(M, K), p.xl.view(M, K)).to(DEV)
    w, b = c.sw.to(DEV), _b(c.bias)
    for f32 in (False, True) if N % 32 == 0 else (True,):
        _variants(c, lambda relu, r: ops.linear_split(x, w, b, c.scale, relu=relu, out_f32=f32, splits=splits)
                  .view(M, 1, 1, -1), res=(False,), f32=f32)


@pytest.mark.parametrize("case", GROUPED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_grouped_split_exact(ops, case):
    B, H, W, C, groups, stride = case
    c = X.split_conv_case(B, H, W, C, C, 3, stride, 1, groups)
    x, w, b = _operands(c)
    _variants(c, lambda relu, r: ops.conv3x3_grouped_split(x, w, b, c.scale, groups, stride, relu), res=(False,))


@pytest.mark.parametrize("tile", [-1, 36])
@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", SLICE_CASES)
def test_conv_split_into_batch_slice_exact(ops, B, H, Cin, Cout, k, s, p, tile):
    """``out=`` a batch slice of a larger tensor: exact there, nothing written around it."""
    c = _conv(B, H, Cin, Cout, k, s, p)
    x, w, b = _operands(c)
    Ho = (H + 2 * p - k) // s + 1
    big = torch.full((B + 3, Ho, Ho, 2 * Cout), 7.0, dtype=torch.float16, device=DEV)

    def call(relu, r):
        big.fill_(7.0)
        y = ops.conv2d_split(x, w, b, c.scale, k, k, s, p, relu, residual=r, tile=tile, out=big[1:1 + B])
        assert y.data_ptr() == big[1].data_ptr()
        assert bool((big[:1] == 7).all()) and bool((big[1 + B:] == 7).all())
        return big[1:1 + B]

    _variants(c, call)


def test_guard_flag_stayed_zero(guard):
    """Last in the module: no exact case left fp16's range (the largest output is below 4096)."""
    torch.cuda.synchronize()
    assert int(guard.item()) == 0
