"""MobileNetV3 on the GPU against fp64 oracles on the CPU: the depthwise k x k conv with
its fused squeeze, the SE gate, the narrow 1x1 conv's additions and both whole models.
Bounds are the suite's for these kernel families (test_mobilenet_gpu._check) and its
whole-model logit bounds."""
import functools

import pytest
import torch
import torch.nn.functional as F

from idunno.models import packed

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _check(y, ref, dtype):
    y = y.double().cpu()
    scale, err = ref.abs().max().item(), (y - ref).abs().max().item()
    bound = 2e-5 * scale if dtype == "fp32" else 1e-2 * scale + 1e-3
    assert err <= bound, f"max err {err:.3e} vs scale {scale:.3e}"


def _act(y, act):
    return [y, F.relu(y), y.clamp(0.0, 6.0), F.hardswish(y), F.hardsigmoid(y)][act]


def _randn(g, dtype, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(DTYPES[dtype])


DW_CASES = [(1, 1, 1, 8, 5, 1), (1, 2, 5, 24, 5, 2), (1, 9, 13, 72, 5, 2), (2, 7, 7, 960, 5, 1), (2, 14, 14, 672, 5, 2),
            (1, 37, 19, 16, 3, 1), (1, 37, 19, 16, 5, 2), (3, 28, 28, 120, 5, 1), (2, 112, 112, 16, 3, 2)]


@functools.lru_cache(maxsize=None)
def _dw_case(case, dtype):
    """Operands in the kernel's precision and the fp64 pre-activation outputs for the plain and the
    hardswished input; inputs and outputs straddle every activation knee (-3, 0, 3, 6)."""
    B, H, W, C, k, s = case
    g = torch.Generator().manual_seed(sum(case))
    x, b = _randn(g, dtype, B, H, W, C, scale=4.0), torch.randn(C, generator=g)
    w = _randn(g, dtype, C, 1, k, k, scale=3.0 / k)
    xd = x.double().permute(0, 3, 1, 2)
    pre = [F.conv2d(v, w.double(), b.double(), s, k // 2, groups=C).permute(0, 2, 3, 1) for v in (xd, F.hardswish(xd))]
    return x, w, b, pre


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", DW_CASES)
def test_depthwise_and_fused_squeeze_vs_fp64(ops, case, dtype):
    x, w, b, pre = _dw_case(case, dtype)
    k, s = case[4:]
    xg, wk, bg = x.to(DEV), packed.pack_dw_weight(w, dtype).to(DEV), b.to(DEV)
    for act in (0, 1, 3):
        ref = _act(pre[0], act)
        _check(ops.conv_dw(xg, wk, bg, k, s, act), ref, dtype)
        means = []
        for _ in range(2):
            pool = torch.full((case[0], case[3]), float("nan"), dtype=xg.dtype, device=DEV)
            y = ops.conv_dw(xg, wk, bg, k, s, act, pool=pool)
            means.append(pool)
        _check(y, ref, dtype)
        _check(pool, ref.mean(dim=(1, 2)), dtype)
        assert torch.equal(means[0], means[1])
    if case == DW_CASES[2]:
        _check(ops.conv_dw(xg, wk, bg, k, s, 3, act_in=3), _act(pre[1], 3), dtype)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("B,C,Csq", [(1, 16, 8), (3, 72, 24), (17, 672, 168), (33, 960, 240)])
def test_se_excite_vs_fp64(ops, B, C, Csq, dtype):
    g = torch.Generator().manual_seed(B + C)
    m, b1, b2 = _randn(g, dtype, B, C), torch.randn(Csq, generator=g), 2.0 * torch.randn(C, generator=g)
    w1, w2 = _randn(g, dtype, Csq, C, 1, 1, scale=2.0 / C ** 0.5), _randn(g, dtype, C, Csq, 1, 1, scale=4.0 / Csq ** 0.5)
    hid = F.relu(m.double() @ w1.double().view(Csq, C).t() + b1.double())
    pre = hid @ w2.double().view(C, Csq).t() + b2.double()
    assert min((pre < -3).float().mean(), (pre > 3).float().mean()).item() > 0.05
    got = ops.se_excite(m.to(DEV), packed.pack_pw_weight(w1, dtype).to(DEV), b1.to(DEV),
                        packed.pack_pw_weight(w2, dtype).to(DEV), b2.to(DEV))
    _check(got, F.hardsigmoid(pre), dtype)


# (B, H, W, K, N), in_scale, residual, res_act, act
PW_CASES = [((3, 7, 7, 72, 40), True, False, 0, 0), ((2, 5, 5, 960, 160), True, True, 0, 0),
            ((2, 9, 13, 16, 16), False, True, 3, 0), ((33, 1, 1, 960, 1280), False, False, 0, 3),
            ((1, 1, 1, 16, 16), False, False, 0, 4)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case,scaled,with_res,res_act,act", PW_CASES)
def test_pointwise_additions_vs_fp64(ops, case, scaled, with_res, res_act, act, dtype):
    B, H, W, K, N = case
    g = torch.Generator().manual_seed(sum(case))
    x, b = _randn(g, dtype, B, H, W, K), 2.0 * torch.randn(N, generator=g)
    w = _randn(g, dtype, N, K, 1, 1, scale=4.0 / K ** 0.5)
    res = _randn(g, dtype, B, H, W, N, scale=3.0)
    sc = torch.rand(B, K, generator=g).to(DTYPES[dtype])          # a distinct gate row per image
    xs = x.double() * sc.double()[:, None, None, :] if scaled else x.double()
    ref = F.conv2d(xs.permute(0, 3, 1, 2), w.double(), b.double()).permute(0, 2, 3, 1)
    if with_res:
        ref = ref + (F.hardswish(res.double()) if res_act else res.double())
    got = ops.conv1x1_narrow(x.to(DEV), packed.pack_pw_weight(w, dtype).to(DEV), b.to(DEV), act,
                             residual=res.to(DEV) if with_res else None, in_scale=sc.to(DEV) if scaled else None,
                             res_act=res_act)
    _check(got, _act(ref, act), dtype)


def test_binding_checks(ops):
    x, b = torch.zeros(1, 4, 4, 16, dtype=torch.float16, device=DEV), torch.zeros(16, device=DEV)
    w25, wp = torch.zeros(25, 16, dtype=torch.float16, device=DEV), torch.zeros(16, 32, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="k must be 3 or 5"):
        ops.conv_dw(x, w25[:16].contiguous(), b, 4, 1, 0)
    with pytest.raises(RuntimeError, match="stride"):
        ops.conv_dw(x, w25, b, 5, 3, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.conv_dw(x[..., :12].contiguous(), w25[:, :12].contiguous(), b[:12], 5, 1, 0)
    with pytest.raises(RuntimeError, match="in_scale"):
        ops.conv1x1_narrow(x, wp, b, 0, in_scale=torch.zeros(2, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError, match="in_scale"):
        ops.conv1x1_narrow(x, wp, b, 0, in_scale=torch.zeros(1, 16, device=DEV))
    wide = torch.zeros(1, 1, 257, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="pool"):
        ops.conv_dw(wide, w25, b, 5, 1, 0, pool=torch.zeros(1, 16, dtype=torch.float16, device=DEV))


@pytest.mark.parametrize("dtype,rel", [("fp16", 0.03), ("fp32", 1e-4)])
@pytest.mark.parametrize("name", ["mobilenet_v3_large", "mobilenet_v3_small"])
def test_model_vs_fp64_module(ops, name, dtype, rel):
    """B = 3, BN randomised: logits within the suite's whole-model bound of the fp64 module's, the
    same top-1 wherever the oracle's top-2 gap exceeds it, three bit-equal graph replays, and the
    float batch of the same images within the same bound.  (torch's own fp32 CPU forward of these
    modules stays within 1e-6 of the logit scale of the fp64 one.)"""
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    m = ref.build(name, seed=7, randomize_bn=True)
    runner = HipRunner(compile_model(m, name, dtype=dtype))
    assert not runner._guarded()
    img = torch.randint(0, 256, (3, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        r = m.double()(ref.preprocess_u8(img).double())
    tol = rel * r.abs().max().item()
    eager = runner.logits(img.to(DEV))
    err = (eager.double().cpu() - r).abs().max().item()
    print(f"{name} {dtype}: logit err {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    cls, prob = runner.forward(img.to(DEV))
    top2 = r.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > tol
    assert torch.equal(cls.long().cpu()[clear], r.argmax(1)[clear])
    sin, replay = runner.capture(3)
    sin.copy_(img.to(DEV))
    for _ in range(3):
        gcls, gprob = replay()
        assert torch.equal(gcls, cls) and torch.equal(gprob, prob)
    xf = ref.preprocess_u8(img).to(DEV)
    assert (runner.logits(xf).double().cpu() - r).abs().max().item() <= tol
