"""The depthwise 3x3 and narrow 1x1 conv kernels and the MobileNetV2 forward on the GPU,
against fp64 oracles on the CPU.  Bounds are the suite's: test_kernels_f32_gpu._check for
fp32, test_kernels_gpu._check for fp16, and their whole-model logit bounds."""
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
    return y.clamp(0.0, 6.0) if act == 2 else F.relu(y) if act else y


DW_CASES = [(1, 1, 1, 8, 1), (1, 2, 5, 24, 2), (1, 9, 13, 144, 1), (3, 15, 15, 96, 2), (2, 14, 14, 576, 2),
            (2, 7, 7, 960, 1), (40, 28, 28, 192, 1)]


@functools.lru_cache(maxsize=None)
def _dw_case(case, dtype):
    """Operands in the kernel's precision (NHWC x, w [C,1,3,3], bias) and the fp64 pre-activation
    outputs for the plain and the clamped input; a sizeable share lies below 0 and above 6, and
    of the inputs above 6."""
    B, H, W, C, s = case
    g = torch.Generator().manual_seed(sum(case))
    x = (5.0 * torch.randn(B, H, W, C, generator=g)).to(DTYPES[dtype])
    w = torch.randn(C, 1, 3, 3, generator=g).to(DTYPES[dtype])
    b = torch.randn(C, generator=g)
    xd = x.double().permute(0, 3, 1, 2)
    pre = [F.conv2d(v, w.double(), b.double(), s, 1, groups=C).permute(0, 2, 3, 1) for v in (xd, xd.clamp(max=6.0))]
    return x, w, b, pre


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", DW_CASES)
def test_depthwise_vs_fp64(ops, case, dtype):
    x, w, b, pre = _dw_case(case, dtype)
    xg, w9, bg = x.to(DEV), packed.pack_dw_weight(w, dtype).to(DEV), b.to(DEV)
    for act in (0, 2):
        _check(ops.conv3x3_dw(xg, w9, bg, case[4], act), _act(pre[0], act), dtype)
    if case in (DW_CASES[2], DW_CASES[3]):
        assert (x.float() > 6).float().mean().item() > 0.05
        _check(ops.conv3x3_dw(xg, w9, bg, case[4], 2, clamp_in=True), _act(pre[1], 2), dtype)


PW_CASES = [(1, 1, 1, 8, 8), (1, 9, 13, 16, 96), (2, 7, 7, 24, 144), (3, 5, 5, 144, 24), (1, 3, 3, 160, 960),
            (2, 7, 7, 960, 160), (1, 7, 7, 320, 1280), (5, 28, 28, 32, 192)]


@functools.lru_cache(maxsize=None)
def _pw_case(case, dtype):
    B, H, W, K, N = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, W, K, generator=g).to(DTYPES[dtype])
    w = (4.0 / K ** 0.5 * torch.randn(N, K, 1, 1, generator=g)).to(DTYPES[dtype])
    b = torch.randn(N, generator=g)
    res = (3.0 * torch.randn(B, H, W, N, generator=g)).to(DTYPES[dtype])
    pre = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double()).permute(0, 2, 3, 1)
    return x, w, b, res, pre


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", PW_CASES)
def test_pointwise_vs_fp64(ops, case, dtype):
    x, w, b, res, pre = _pw_case(case, dtype)
    xg, wp, bg = x.to(DEV), packed.pack_pw_weight(w, dtype).to(DEV), b.to(DEV)
    for act in (0, 1, 2):
        _check(ops.conv1x1_narrow(xg, wp, bg, act), _act(pre, act), dtype)
    _check(ops.conv1x1_narrow(xg, wp, bg, 0, residual=res.to(DEV)), pre + res.double(), dtype)
    if case == PW_CASES[2]:
        # x as a channel slice of a wider tensor whose other channels are huge: only the zero fill of the
        # staged rows from K = 24 up to Kp keeps them out of the sum
        wide = torch.full((*x.shape[:3], 64), 3.0e4, dtype=x.dtype, device=DEV)
        wide[..., :24] = xg
        _check(ops.conv1x1_narrow(wide[..., :24], wp, bg, 0), pre, dtype)


def test_binding_checks(ops):
    x, b = torch.zeros(1, 4, 4, 16, dtype=torch.float16, device=DEV), torch.zeros(16, device=DEV)
    w9, wp = torch.zeros(9, 16, dtype=torch.float16, device=DEV), torch.zeros(16, 32, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="stride"):
        ops.conv3x3_dw(x, w9, b, 3, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.conv3x3_dw(x[..., :12].contiguous(), w9[:, :12].contiguous(), b[:12], 1, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.conv1x1_narrow(x[..., :12].contiguous(), wp, b, 0)
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv1x1_narrow(x, wp, b, 0, residual=torch.zeros(1, 4, 4, 16, device=DEV))


@pytest.mark.parametrize("dtype,rel", [("fp16", 0.03), ("fp32", 1e-4)])
def test_model_vs_fp64_module(ops, dtype, rel):
    """B = 3, BN randomised: logits within the suite's whole-model bound of the fp64 module's, the
    same top-1 wherever the oracle's top-2 gap exceeds it, a bit-equal graph replay, and the float
    batch of the same images within the same bound."""
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    m = ref.build("mobilenet_v2", seed=7, randomize_bn=True)
    runner = HipRunner(compile_model(m, "mobilenet_v2", dtype=dtype))
    assert not runner._guarded()
    img = torch.randint(0, 256, (3, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        r = m.double()(ref.preprocess_u8(img).double())
    tol = rel * r.abs().max().item()
    eager = runner.logits(img.to(DEV))
    err = (eager.double().cpu() - r).abs().max().item()
    print(f"mobilenet_v2 {dtype}: logit err {err:.3e}, bound {tol:.3e}")
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
