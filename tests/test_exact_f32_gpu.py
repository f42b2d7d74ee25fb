"""Bit-exact checks of the f32-MFMA conv / FC kernels and the fused Winograd conv
(exact_ref.py): on dyadic grid data every result is the float64 reference
itself (``expect_f32`` is lossless), compared with ``torch.equal``.  The case
lists are test_kernels_f32_gpu.py's own; test_exact_cpu.py qualifies them.
"""
import pytest
import torch

import exact_ref as X
import test_kernels_f32_gpu as TF

DEV = "cuda"

CONV_CASES = TF.CONV_CASES            # (B, H, Cin, Cout, k, s, p), with the odd (1, 9, 48, 20, 3, 1, 1)
F32_TILES = TF.F32_TILES
TILE_HS = X.parametrize_args(TF.test_conv_f32_all_tiles_with_residual, "H")
WINO_CASES = TF.WINO_CASES            # (B, H, W, Cin, Cout)
WINO_VARIANTS = X.parametrize_args(TF.test_conv_wino_f32, "variant")
LINEAR_CASES = [(37, 512, 1000), (130, 2048, 36), (7, 4096, 4096)]      # (M, K, N)
SPLITK_CASES = [(37, 512, 1000), (130, 2048, 36)]
SPLITK_SPLITS = [1, 2, 4, 8]


def tile_case(H):
    return X.conv_case(2, H, H, 128, 256, 3, 1, 1)


def wino_case(B, H, W, Cin, Cout):
    return X.conv_case(B, H, W, Cin, Cout, 3, 1, 1, wino=True)


def cpu_cases():
    """(id, thunk -> Case) of every distinct data set the tests below run."""
    cs = {}
    for B, H, Cin, Cout, k, s, p in CONV_CASES:
        cs[f"conv{(B, H, Cin, Cout, k, s, p)}"] = lambda a=(B, H, H, Cin, Cout, k, s, p): X.conv_case(*a)
    for H in TILE_HS:
        cs[f"tile{(H,)}"] = lambda a=H: tile_case(a)
    for c in WINO_CASES:
        cs[f"wino{c}"] = lambda a=c: wino_case(*a)
    for c in LINEAR_CASES + SPLITK_CASES:
        cs[f"linear{c}"] = lambda a=c: X.linear_case(*a)
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


def _f(t):
    """NCHW float64 -> NHWC fp32 on the GPU (lossless on the grid)."""
    return None if t is None else X.nhwc(t).float().to(DEV)


def _pack(w):
    from idunno.models.packed import pack_conv_weight

    pw, small = pack_conv_weight(w.float(), "fp32")
    assert not small and pw.dtype == torch.float32
    return pw.to(DEV)


def _variants(case, call, res=(False, True), relus=(True, False)):
    fails = []
    for use_res in res:
        for relu in relus:
            ref = X.nhwc(case.ref(relu, use_res))
            y = call(relu, _f(case.res) if use_res else None)
            try:
                X.assert_bits(y, X.expect_f32(ref), ref)
            except AssertionError as e:
                fails.append(f"residual={use_res} relu={relu}: {e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", CONV_CASES)
def test_conv_f32_default_tile_exact(ops, B, H, Cin, Cout, k, s, p):
    c = X.conv_case(B, H, H, Cin, Cout, k, s, p)
    x, w, b = _f(c.x), _pack(c.w), c.bias.float().to(DEV)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, k, k, s, p, relu, residual=r))


@pytest.mark.parametrize("tile", F32_TILES)
@pytest.mark.parametrize("H", TILE_HS)
def test_conv_f32_all_tiles_exact(ops, tile, H):
    c = tile_case(H)
    x, w, b = _f(c.x), _pack(c.w), c.bias.float().to(DEV)
    _variants(c, lambda relu, r: ops.conv2d(x, w, b, 3, 3, 1, 1, relu, residual=r, tile=tile))


@pytest.mark.parametrize("variant", WINO_VARIANTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout", WINO_CASES)
def test_conv_wino_f32_exact(ops, B, H, W, Cin, Cout, variant):
    """Fused F(2x2,3x3): U = G g G^T is exact on the grid (test_exact_cpu.py), the
    input / output transforms only add, so the result is the direct conv's."""
    from idunno.models.packed import wino_weight

    c = wino_case(B, H, W, Cin, Cout)
    assert ops.wino_supported(H, W, Cin, Cout)
    x, u, b = _f(c.x), wino_weight(c.w.float()).to(DEV), c.bias.float().to(DEV)
    _variants(c, lambda relu, r: ops.conv2d_wino(x, u, b, relu, r, variant))


@pytest.mark.parametrize("splits", [None, 1])
@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
def test_linear_f32_exact(ops, M, K, N, splits):
    c = X.linear_case(M, K, N)
    x, w, b = c.x.view(M, K).float().to(DEV), c.w.view(N, K).float().to(DEV), c.bias.float().to(DEV)
    _variants(c, lambda relu, r: ops.linear(x, w, b, relu=relu, splits=splits).view(M, 1, 1, N), res=(False,))


@pytest.mark.parametrize("splits", SPLITK_SPLITS)
@pytest.mark.parametrize("M,K,N", SPLITK_CASES)
def test_linear_f32_splitk_exact(ops, M, K, N, splits):
    c = X.linear_case(M, K, N)
    x, w, b = c.x.view(M, K).float().to(DEV), c.w.view(N, K).float().to(DEV), c.bias.float().to(DEV)
    ext = ops.load()
    _variants(c, lambda relu, r: ext.linear_f32_splitk(x, w, b, relu, splits, -1).view(M, 1, 1, N), res=(False,))
