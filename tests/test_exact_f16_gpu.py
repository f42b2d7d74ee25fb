"""Bit-exact checks of the fp16 MFMA conv / FC kernels (exact_ref.py).

On dyadic grid data every fp32 accumulation order is exact, so each kernel
must return the float64 reference rounded ONCE to nearest-even (fp16 output)
or the reference itself (fp32 output): ``torch.equal``, no tolerance.  The
case lists are the existing loose tests' own (imported), so every path they
reach is pinned; test_exact_cpu.py qualifies the same cases on the CPU.
"""
import pytest
import torch

import exact_ref as X
import test_band as TB
import test_c64_f16 as TC
import test_grouped_gpu as TG
import test_kernels_gpu as TK

DEV = "cuda"

CONV_CASES = TK.CONV_CASES                                                       # (B, H, Cin, Cout, k, s, p)
TILES = X.parametrize_args(TK.test_conv_all_tiles_with_residual, "tile")
TILE_HS = X.parametrize_args(TK.test_conv_all_tiles_with_residual, "H")
KSPLIT_CASES = X.parametrize_args(TK.test_conv_f16_ksplit, "B")                  # (B, H, Cin, Cout, k, s, ks)
STREAM_CASES = sorted({c[:4] for c in X.parametrize_args(TK.test_conv1x1_stream, "B")})   # (B, H, Cin, Cout)
DUAL_CASES = X.parametrize_args(TK.test_conv1x1_dual, "B")                       # (B, Ho, K1, K2, Cout, s)
FUSED_CASES = X.parametrize_args(TK.test_conv1x1_fused_next, "B")                # (B, H, N2, dual)
C64_CASES = X.parametrize_args(TC.test_conv3x3_c64_f16_vs_fp32, "B")             # (B, H, W)
BAND_CASES = X.parametrize_args(TB.test_band_conv_f16_vs_fp32, "B")              # (B, H, Cin, Cout)
assert BAND_CASES == TB.BAND_CASES + [(3, 14, 512, 256)]
STEM_CASES = [(7, 2, 3, 37), (11, 4, 2, 37)]                                     # (k, s, p, H): every border tap
LINEAR_CASES = [(5, 512, 1000), (7, 9216, 4096), (130, 2048, 1000)]              # (M, K, N): M 130 leaves a partial tile
LINEAR_SPLITS = [None, 1, 2, 4, 8]
SLICE_CASES = [(2, 14, 256, 256, 3, 1, 1), (2, 14, 1024, 256, 1, 1, 0)]
GROUPED_CASES = TG.CASES                                                         # (B, H, W, C, groups, stride)


def tile_case(tile, H):
    return X.conv_case(2, H, H, 128, 256 if tile == 17 else 128, 3, 1, 1)


def fused_first(B, H, dual):
    """First stage of conv1x1_fused_next on the coarse grid: (case, y, x)."""
    if dual:
        case, y, x, _, _ = X.dual_case(B, H, 64, 64, 256, 1, coarse=True)
        return case, y, x
    case = X.conv_case(B, H, H, 64, 256, 1, 1, 0, coarse=True)
    return case, case.x, case.res


def fused_second(B, H, N2, dual, relu):
    """Second stage: the reduce 1x1 of the first stage's (exact, fp16-representable) output."""
    first = fused_first(B, H, dual)[0]
    out = first.ref(relu, not dual)
    assert torch.equal(out.half().double(), out), "first-stage output must be an fp16 value"
    seed = X.case_seed("fused-next", B, H, N2, dual)
    _, w2, b2, _ = X.grid_conv_case(1, 1, 1, 256, N2, 1, 1, 0, False, seed)
    return X.Case(out, w2, b2, None, 1, 0)


def cpu_cases():
    """(id, thunk -> Case) of every distinct data set the tests below run."""
    cs = {}
    for B, H, Cin, Cout, k, s, p in CONV_CASES + SLICE_CASES:
        cs[f"conv{(B, H, Cin, Cout, k, s, p)}"] = lambda a=(B, H, H, Cin, Cout, k, s, p): X.conv_case(*a)
    for H in TILE_HS:
        for tile in (17, 36):
            cs[f"tile{(H, tile)}"] = lambda a=(tile, H): tile_case(*a)
    for B, H, Cin, Cout, k, s, _ks in KSPLIT_CASES:
        cs[f"conv{(B, H, Cin, Cout, k, s, k // 2)}"] = lambda a=(B, H, H, Cin, Cout, k, s, k // 2): X.conv_case(*a)
    for B, H, Cin, Cout in STREAM_CASES:
        for s in (1, 2):
            cs[f"conv{(B, H, Cin, Cout, 1, s, 0)}"] = lambda a=(B, H, H, Cin, Cout, 1, s, 0): X.conv_case(*a)
    for c in DUAL_CASES:
        cs[f"dual{c}"] = lambda a=c: X.dual_case(*a)[0]
    for B, H, N2, dual in FUSED_CASES:
        cs[f"fused-first{(B, H, dual)}"] = lambda a=(B, H, dual): fused_first(*a)[0]
        cs[f"fused-second{(B, H, N2, dual)}"] = lambda a=(B, H, N2, dual): fused_second(*a, True)
    for B, H, W in C64_CASES:
        cs[f"c64{(B, H, W)}"] = lambda a=(B, H, W, 64, 64, 3, 1, 1): X.conv_case(*a)
    for B, H, Cin, Cout in BAND_CASES:
        cs[f"conv{(B, H, Cin, Cout, 3, 1, 1)}"] = lambda a=(B, H, H, Cin, Cout, 3, 1, 1): X.conv_case(*a)
    for k, s, p, H in STEM_CASES:
        cs[f"stem{(k, s, p, H)}"] = lambda a=(2, H, H, 3, 64, k, s, p): X.conv_case(*a)
    for c in LINEAR_CASES:
        cs[f"linear{c}"] = lambda a=c: X.linear_case(*a)
    for c in GROUPED_CASES:
        cs[f"grouped{c}"] = lambda a=c: X.grouped_case(*a)
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


def _h(t):
    """NCHW float64 -> NHWC fp16 on the GPU (lossless: the operands are fp16 values)."""
    return None if t is None else X.nhwc(t).half().to(DEV)


def _pack(w):
    from idunno.models.packed import pack_conv_weight

    pw, small = pack_conv_weight(w.float())      # its .half() is lossless: grid_conv_case asserts w is fp16 data
    assert not small
    return pw.to(DEV)


def _b(bias):
    return bias.float().to(DEV)


def _variants(case, calls, res=(False, True), relus=(True, False), f32=False):
    """``call(relu, residual NHWC fp16 or None)`` (one, or a dict of labelled
    ones that share the reference) against the exact result, for every ReLU /
    residual combination; all mismatches are reported together."""
    if callable(calls):
        calls = {"": calls}
    fails = []
    for use_res in res:
        for relu in relus:
            ref = X.nhwc(case.ref(relu, use_res))
            expect = X.expect_f32(ref) if f32 else X.expect_f16(ref)
            for label, call in calls.items():
                y = call(relu, _h(case.res) if use_res else None)
                try:
                    X.assert_bits(y, expect, ref)
                except AssertionError as e:
                    fails.append(f"{label} residual={use_res} relu={relu} out_f32={f32}: {e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", CONV_CASES)
def test_conv_default_tile_exact(ops, B, H, Cin, Cout, k, s, p):
    c = X.conv_case(B, H, H, Cin, Cout, k, s, p)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, k, k, s, p, relu, residual=r))
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, k, k, s, p, relu, residual=r, out_f32=True), f32=True)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("H", TILE_HS)
def test_conv_all_tiles_exact(ops, tile, H):
    c = tile_case(tile, H)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, 3, 3, 1, 1, relu, residual=r, tile=tile))
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, 3, 3, 1, 1, relu, residual=r, tile=tile, out_f32=True), f32=True)


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,ks", KSPLIT_CASES)
def test_conv_ksplit_exact(ops, B, H, Cin, Cout, k, s, ks):
    """K slices into fp32 partials + one combine: the slices' sums are exact too."""
    c = X.conv_case(B, H, H, Cin, Cout, k, s, k // 2)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, k, k, s, k // 2, relu, residual=r, ksplit=ks))
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, k, k, s, k // 2, relu, residual=r, ksplit=ks, out_f32=True),
              f32=True)


@pytest.mark.parametrize("tile", [-1, 36])
@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", SLICE_CASES)
def test_conv_into_batch_slice_exact(ops, B, H, Cin, Cout, k, s, p, tile):
    """``out=`` a batch slice of a larger tensor: exact there, nothing written around it."""
    c = X.conv_case(B, H, H, Cin, Cout, k, s, p)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    Ho = (H + 2 * p - k) // s + 1
    big = torch.full((B + 3, Ho, Ho, Cout), 7.0, dtype=torch.float16, device=DEV)

    def call(relu, r):
        big.fill_(7.0)
        y = ops.conv2d(x, w, b, k, k, s, p, relu, residual=r, tile=tile, out=big[1:1 + B])
        assert y.data_ptr() == big[1].data_ptr()
        assert bool((big[:1] == 7).all()) and bool((big[1 + B:] == 7).all())
        return big[1:1 + B]

    _variants(c, call)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,Cin,Cout", STREAM_CASES)
def test_conv1x1_stream_exact(ops, B, H, Cin, Cout, stride):
    """Tile 80 (conv1x1_stream.hip) and the implicit-GEMM tile 36 both give the
    once-rounded exact result, so they are EQUAL (test_conv1x1_stream's 2e-3)."""
    c = X.conv_case(B, H, H, Cin, Cout, 1, stride, 0)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    _variants(c, {f"tile {t}": lambda relu, r, t=t: ops.conv2d(x, w, b, 1, 1, stride, 0, relu, residual=r, tile=t)
                  for t in (80, 36)})


@pytest.mark.parametrize("B,Ho,K1,K2,Cout,s", DUAL_CASES)
def test_conv1x1_dual_exact(ops, B, Ho, K1, K2, Cout, s):
    c, y, x, wy, wx = X.dual_case(B, Ho, K1, K2, Cout, s)
    yd, xd, b = _h(y), _h(x), _b(c.bias)
    w = torch.cat([_pack(wy), _pack(wx)], 1).contiguous()
    _variants(c, lambda relu, r: ops.conv1x1_dual(yd, xd, w, b, s, relu), res=(False,))


@pytest.mark.parametrize("B,H,N2,dual", FUSED_CASES)
def test_conv1x1_fused_next_exact(ops, B, H, N2, dual):
    """``out`` is the exact (coarse-grid, fp16-representable) tail; ``z`` the
    once-rounded reduce conv of exactly that ``out``."""
    first, y, x = fused_first(B, H, dual)
    yd, xd, b = _h(y), _h(x), _b(first.bias)
    if dual:
        w = torch.cat([_pack(first.w[:, :64]), _pack(first.w[:, 64:])], 1).contiguous()
    else:
        w = _pack(first.w)
    fails = []
    for relu in (True, False):
        second = fused_second(B, H, N2, dual, relu)
        w2, b2 = _pack(second.w), _b(second.bias)
        if dual:
            out, z = ops.conv1x1_fused_next(yd, w, b, w2, b2, x2=xd, relu=relu)
        else:
            out, z = ops.conv1x1_fused_next(yd, w, b, w2, b2, residual=xd, relu=relu)
        out_ref, z_ref = X.nhwc(second.x), X.nhwc(second.ref(True, False))
        for name, got, ref in (("out", out, out_ref), ("z", z, z_ref)):
            try:
                X.assert_bits(got, X.expect_f16(ref), ref)
            except AssertionError as e:
                fails.append(f"{name} relu={relu}: {e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,W", C64_CASES)
def test_conv3x3_c64_exact(ops, B, H, W):
    """Tile 50 (conv3x3_c64.hip): paired and plain widths, several tiles per workgroup at B = 40."""
    c = X.conv_case(B, H, W, 64, 64, 3, 1, 1)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, 3, 3, 1, 1, relu, residual=r, tile=50))


@pytest.mark.parametrize("max_grid", [0, 3])
@pytest.mark.parametrize("B,H,Cin,Cout", BAND_CASES)
def test_conv3x3_band_f16_exact(ops, B, H, Cin, Cout, max_grid):
    """conv3x3_band.hip on fp16 operands, free and capped persistent grid; through
    ops.conv2d tile 70 equals the default and the 128 x 128 im2col tile bit for bit."""
    c = X.conv_case(B, H, H, Cin, Cout, 3, 1, 1)
    x, w, b = _h(c.x), _pack(c.w), _b(c.bias)
    ext = ops.load()
    _variants(c, lambda relu, r: ext.conv3x3_band_f16(x, w, b, r, relu, max_grid))
    if max_grid == 0:
        _variants(c, {f"tile {t}": lambda relu, r, t=t: ops.conv2d(x, w, b, 3, 3, 1, 1, relu, residual=r, tile=t)
                      for t in (70, -1, 36)})


@pytest.mark.parametrize("k,s,p,H", STEM_CASES)
def test_conv_small_c_stem_exact(ops, k, s, p, H):
    """conv_igemm.hip's small-C path on an NHWC4 fp16 input built directly (4th channel zero)."""
    from idunno.models.packed import pack_conv_weight

    c = X.conv_case(2, H, H, 3, 64, k, s, p)
    x4 = torch.zeros(2, H, H, 4, dtype=torch.float16, device=DEV)
    x4[..., :3] = _h(c.x)
    pw, small = pack_conv_weight(c.w.float())
    assert small
    w, b = pw.to(DEV), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv2d(x4, w, b, k, k, s, p, relu, residual=r))
    _variants(c, lambda relu, r: ops.conv2d(x4, w, b, k, k, s, p, relu, out_f32=True), res=(False,), f32=True)


@pytest.mark.parametrize("splits", LINEAR_SPLITS)
@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
def test_linear_exact(ops, M, K, N, splits):
    c = X.linear_case(M, K, N)
    x = c.x.view(M, K).half().to(DEV)
    w = c.w.view(N, K).half().to(DEV)
    b = _b(c.bias)
    for f32 in (False, True):
        _variants(c, lambda relu, r: ops.linear(x, w, b, relu=relu, out_f32=f32, splits=splits).view(M, 1, 1, N),
                  res=(False,), f32=f32)


@pytest.mark.parametrize("case", GROUPED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_grouped_exact(ops, case):
    """conv3x3_grouped.hip on fp16 operands (block-local weights of pack_grouped_weight):
    the float64 grouped conv rounded once."""
    from idunno.models.packed import pack_grouped_weight

    B, H, W, C, groups, stride = case
    c = X.grouped_case(B, H, W, C, groups, stride)
    x, w, b = _h(c.x), pack_grouped_weight(c.w.float(), groups).to(DEV), _b(c.bias)
    _variants(c, lambda relu, r: ops.conv3x3_grouped(x, w, b, groups, stride, relu), res=(False,))
