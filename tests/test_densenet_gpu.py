"""The fused dense layer, the fused transition, the max pool into a buffer, the norm5 head and the DenseNet forward
on the GPU, against fp64 oracles on the CPU computed from operands rounded to the kernel's dtype.  Bounds are the
suite's: test_squeezenet_gpu._check and its whole-model logit bounds."""
import functools

import pytest
import torch
import torch.nn.functional as F

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
    print(f"max err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}")
    assert err <= bound, f"max err {err:.3e} vs scale {scale:.3e}"


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _affine(x, scale, shift):
    return x * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)


def _mixed(pre):
    neg = (pre < 0).double().mean().item()
    assert 0.1 < neg < 0.9, neg


# (B, H, W, Cin, Ctot)
LAYER_CASES = [(1, 1, 1, 64, 96), (2, 3, 5, 96, 160), (1, 7, 7, 992, 1024), (1, 14, 14, 256, 320),
               (1, 28, 28, 128, 160), (1, 56, 56, 64, 96), (1, 6, 9, 160, 224)]


@functools.lru_cache(maxsize=None)
def _layer_case(case, dtype):
    """Operands in the kernel's precision and the fp64 slice.  shift1 and b1 have mean +0.5: a pad slot staged
    through the prologue (relu(shift1)) or a halo computed from zero-padded input (relu(b1)) would show."""
    B, H, W, Cin, Ctot = case
    g, dt = torch.Generator().manual_seed(sum(case)), DTYPES[dtype]
    buf = torch.full((B, H, W, Ctot), 7.0).to(dt)
    buf[..., :Cin] = torch.randn(B, H, W, Cin, generator=g).to(dt)
    scale1 = 0.5 + torch.rand(Cin, generator=g)
    shift1 = 0.5 + 0.5 * torch.randn(Cin, generator=g)
    w1 = (torch.randn(128, Cin, generator=g) / Cin ** 0.5).to(dt)
    b1 = 0.5 + 0.5 * torch.randn(128, generator=g)
    w2 = (torch.randn(32, 128, 3, 3, generator=g) / 1152 ** 0.5).to(dt)
    pre1 = _affine(_nchw(buf[..., :Cin]), scale1, shift1)
    pre2 = F.conv2d(F.relu(pre1), w1.double().view(128, Cin, 1, 1), b1.double())
    _mixed(pre1)
    _mixed(pre2)
    ref = F.conv2d(F.relu(pre2), w2.double(), padding=1).permute(0, 2, 3, 1)
    return buf, scale1, shift1, w1, b1, w2.permute(0, 2, 3, 1).reshape(32, 1152).contiguous(), ref


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", LAYER_CASES)
def test_dense_layer_vs_fp64(ops, case, dtype):
    buf, scale1, shift1, w1, b1, w2, ref = _layer_case(case, dtype)
    cin = case[3]
    assert ops.dense_layer_ok(*case[1:])
    dbuf = buf.to(DEV)
    out = ops.dense_layer(dbuf, cin, scale1.to(DEV), shift1.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV))
    assert out is dbuf
    got = dbuf.cpu()
    _check(got[..., cin:cin + 32], ref, dtype)
    assert torch.equal(got[..., :cin], buf[..., :cin]) and torch.equal(got[..., cin + 32:], buf[..., cin + 32:])


# (B, H, W, C, Ctot_next)
TRANS_CASES = [(1, 2, 2, 64, 64), (2, 6, 10, 160, 96), (1, 5, 7, 96, 48), (1, 14, 14, 1792, 928)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", TRANS_CASES)
def test_dense_transition_vs_fp64(ops, case, dtype):
    B, H, W, C, Cn = case
    g, dt = torch.Generator().manual_seed(sum(case)), DTYPES[dtype]
    x = torch.randn(B, H, W, C, generator=g).to(dt)
    scale, shift = 0.5 + torch.rand(C, generator=g), 0.5 + 0.5 * torch.randn(C, generator=g)
    w = (torch.randn(C // 2, C, generator=g) / C ** 0.5).to(dt)
    pre = _affine(_nchw(x), scale, shift)
    _mixed(pre)
    ref = F.avg_pool2d(F.conv2d(F.relu(pre), w.double().view(C // 2, C, 1, 1)), 2, 2).permute(0, 2, 3, 1)
    out = torch.full((B, H // 2, W // 2, Cn), 7.0, dtype=dt, device=DEV)
    assert ops.dense_transition(x.to(DEV), scale.to(DEV), shift.to(DEV), w.to(DEV), out) is out
    _check(out[..., :C // 2], ref, dtype)
    assert bool((out[..., C // 2:] == 7.0).all())


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("shape,ctot", [((1, 8, 8, 64), 96), ((2, 7, 9, 64), 256)])
def test_maxpool2d_into_exact(ops, shape, ctot, dtype):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(ctot)).to(DTYPES[dtype])
    ref = F.max_pool2d(_nchw(x), 3, 2, 1).permute(0, 2, 3, 1)
    buf = torch.full((*ref.shape[:3], ctot), 7.0, dtype=DTYPES[dtype], device=DEV)
    assert ops.maxpool2d_into(x.to(DEV), buf, 3, 2, 1) is buf
    assert torch.equal(buf[..., :64].double().cpu(), ref) and bool((buf[..., 64:] == 7.0).all())


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 64), (3, 7, 7, 1920)])
def test_bn_relu_avgpool_vs_fp64(ops, shape, dtype):
    g, dt = torch.Generator().manual_seed(shape[3]), DTYPES[dtype]
    x = torch.randn(*shape, generator=g).to(dt)
    scale, shift = 0.5 + torch.rand(shape[3], generator=g), 0.5 * torch.randn(shape[3], generator=g)
    ref = F.relu(_affine(_nchw(x), scale, shift)).mean(dim=(2, 3))
    args = (x.to(DEV), scale.to(DEV), shift.to(DEV))
    y = ops.bn_relu_avgpool(*args)
    assert y.dtype == dt and tuple(y.shape) == (shape[0], shape[3])
    _check(y, ref, dtype)
    assert torch.equal(y, ops.bn_relu_avgpool(*args))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_binding_checks(ops, dtype):
    def call(cin=64, ctot=96, nscale=None, buf=None):
        z = lambda *shape: torch.zeros(*shape, dtype=DTYPES[dtype], device=DEV)
        f = lambda n: torch.zeros(n, device=DEV)
        buf = z(1, 4, 8, ctot) if buf is None else buf
        return ops.dense_layer(buf, cin, f(cin if nscale is None else nscale), f(cin), z(128, cin), f(128), z(32, 1152))

    assert tuple(call().shape) == (1, 4, 8, 96)
    with pytest.raises(RuntimeError, match="cin: must be a multiple of 32"):
        call(cin=48)
    with pytest.raises(RuntimeError, match=r"cin: cin \+ 32 must be at most"):
        call(cin=96, ctot=96)
    with pytest.raises(RuntimeError, match="scale1: must have"):
        call(nscale=32)
    with pytest.raises(RuntimeError, match="buf must be contiguous"):
        call(buf=torch.zeros(1, 4, 8, 192, dtype=DTYPES[dtype], device=DEV)[..., :96])


@pytest.mark.parametrize("dtype,rel", [("fp16", 0.03), ("fp32", 1e-4)])
@pytest.mark.parametrize("name", ["densenet121", "densenet169", "densenet201"])
def test_model_vs_fp64_module(ops, name, dtype, rel):
    """B = 2, randomised BN: logits within the suite's whole-model bound of the fp64 module's, the same top-1
    wherever the oracle's top-2 gap exceeds it, a bit-equal graph replay, and the float batch of the same images
    within the same bound."""
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    m = ref.build(name, seed=7, randomize_bn=True)
    runner = HipRunner(compile_model(m, name, dtype=dtype))
    assert not runner._guarded()
    img = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        r = m.double()(ref.preprocess_u8(img).double())
    tol = rel * r.abs().max().item()
    eager = runner.logits(img.to(DEV))
    err = (eager.double().cpu() - r).abs().max().item()
    print(f"{name} {dtype}: logit err {err:.3e}, bound {tol:.3e}")
    assert eager.dtype == torch.float32 and err <= tol
    cls, prob = runner.forward(img.to(DEV))
    top2 = r.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > tol
    assert torch.equal(cls.long().cpu()[clear], r.argmax(1)[clear])
    sin, replay = runner.capture(2)
    sin.copy_(img.to(DEV))
    for _ in range(3):
        gcls, gprob = replay()
        assert torch.equal(gcls, cls) and torch.equal(gprob, prob)
    xf = ref.preprocess_u8(img).to(DEV)
    assert (runner.logits(xf).double().cpu() - r).abs().max().item() <= tol
