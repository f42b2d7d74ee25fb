"""The fused Fire kernel, the pooled conv head, the ceil-mode max pool and the SqueezeNet forward
on the GPU, against fp64 oracles on the CPU computed from operands rounded to the kernel's dtype.
Bounds are the suite's: test_mobilenet_gpu._check and its whole-model logit bounds."""
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
    print(f"max err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}")
    assert err <= bound, f"max err {err:.3e} vs scale {scale:.3e}"


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


# (B, H, W, Cin, S, E1, E3)
FIRE_CASES = [(1, 1, 1, 64, 16, 64, 64), (3, 3, 5, 96, 16, 64, 64), (1, 7, 17, 256, 48, 192, 192),
              (2, 13, 13, 512, 64, 256, 256), (1, 27, 27, 128, 32, 128, 128), (1, 55, 55, 64, 16, 64, 64),
              (1, 6, 9, 64, 16, 64, 128)]


@functools.lru_cache(maxsize=None)
def _fire_case(case, dtype):
    """Operands in the kernel's precision and the fp64 module output; bs has mean +0.5, so relu(bs) != 0
    and a halo squeezed from zero-padded x would show."""
    B, H, W, Cin, S, E1, E3 = case
    g, dt = torch.Generator().manual_seed(sum(case)), DTYPES[dtype]
    x = torch.randn(B, H, W, Cin, generator=g).to(dt)
    ws = (torch.randn(S, Cin, 1, 1, generator=g) / Cin ** 0.5).to(dt)
    bs = 0.5 + 0.5 * torch.randn(S, generator=g)
    w1 = (torch.randn(E1, S, 1, 1, generator=g) / S ** 0.5).to(dt)
    w3 = (torch.randn(E3, S, 3, 3, generator=g) / (9 * S) ** 0.5).to(dt)
    be = torch.randn(E1 + E3, generator=g)
    pre = F.conv2d(_nchw(x), ws.double(), bs.double())
    neg = (pre < 0).double().mean().item()
    assert 0.1 < neg < 0.9, neg
    s = F.relu(pre)
    y = torch.cat([F.conv2d(s, w1.double(), be[:E1].double()), F.conv2d(s, w3.double(), be[E1:].double(), padding=1)], 1)
    return x, ws, bs, w1, w3, be, F.relu(y).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", FIRE_CASES)
def test_fire_vs_fp64(ops, case, dtype):
    x, ws, bs, w1, w3, be, ref = _fire_case(case, dtype)
    assert ops.fire_ok(*case[1:])
    args = (x.to(DEV), packed.pack_pw_weight(ws, dtype).to(DEV), bs.to(DEV),
            packed.pack_fire_weights(w1, w3, dtype).to(DEV), be.to(DEV), case[5])
    _check(ops.fire(*args), ref, dtype)
    if case == FIRE_CASES[6]:
        out = torch.full(ref.shape, 7.0, dtype=DTYPES[dtype], device=DEV)
        assert ops.fire(*args, out=out) is out
        _check(out, ref, dtype)


HEAD_CASES = [(1, 1, 1, 16, 8), (3, 13, 13, 512, 1000), (2, 5, 7, 64, 24)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", HEAD_CASES)
def test_pooled_head_vs_fp64(ops, case, dtype):
    B, H, W, K, N = case
    g, dt = torch.Generator().manual_seed(sum(case)), DTYPES[dtype]
    x = torch.randn(B, H, W, K, generator=g).to(dt)
    w = (torch.randn(N, K, 1, 1, generator=g) / K ** 0.5).to(dt)
    b = 0.5 + 0.5 * torch.randn(N, generator=g)
    ref = F.relu(F.conv2d(_nchw(x), w.double(), b.double())).mean(dim=(2, 3))
    xg, wp, bg = x.to(DEV), packed.pack_pw_weight(w, dtype).to(DEV), b.to(DEV)
    y = ops.conv1x1_relu_pool(xg, wp, bg)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, N)
    _check(y, ref, dtype)
    assert torch.equal(y, ops.conv1x1_relu_pool(xg, wp, bg))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("shape", [(1, 54, 54, 96), (2, 6, 6, 16), (1, 55, 55, 64)])
def test_ceil_pool_exact(ops, shape, dtype):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1])).to(DTYPES[dtype])
    ref = F.max_pool2d(_nchw(x), 3, 2, 0, ceil_mode=True).permute(0, 2, 3, 1)
    y = ops.maxpool2d(x.to(DEV), 3, 2, 0, ceil_mode=True)
    assert y.shape == ref.shape and torch.equal(y.double().cpu(), ref)
    if shape[1] == 54:
        assert tuple(ops.maxpool2d(x.to(DEV), 3, 2, 0).shape) == (1, 26, 26, 96)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_binding_checks(ops, dtype):
    def call(w=8, s=16, nbias=128):
        z = lambda *shape: torch.zeros(*shape, dtype=DTYPES[dtype], device=DEV)
        ws, we = packed.pack_pw_weight(torch.zeros(s, 64, 1, 1), dtype), z(128, packed.fire_kpad(s, dtype))
        return ops.fire(z(1, 4, w, 64), ws.to(DEV), torch.zeros(s, device=DEV), we, torch.zeros(nbias, device=DEV), 64)

    assert tuple(call().shape) == (1, 4, 8, 128)
    with pytest.raises(RuntimeError, match="S must be"):
        call(s=24)
    with pytest.raises(RuntimeError, match="W must be"):
        call(w=512)
    with pytest.raises(RuntimeError, match="be: must have"):
        call(nbias=64)


@pytest.mark.parametrize("dtype,rel", [("fp16", 0.03), ("fp32", 1e-4)])
@pytest.mark.parametrize("name", ["squeezenet1_0", "squeezenet1_1"])
def test_model_vs_fp64_module(ops, name, dtype, rel):
    """B = 3, conv biases perturbed: logits within the suite's whole-model bound of the fp64
    module's, the same top-1 wherever the oracle's top-2 gap exceeds it, a bit-equal graph replay,
    and the float batch of the same images within the same bound."""
    from idunno.models import HipRunner, compile_model
    from idunno.models import reference as ref

    m = ref.build(name, seed=7)
    g = torch.Generator().manual_seed(11)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.bias.data = 0.1 * torch.randn(mod.out_channels, generator=g)
    runner = HipRunner(compile_model(m, name, dtype=dtype))
    assert not runner._guarded()
    img = torch.randint(0, 256, (3, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
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
    sin, replay = runner.capture(3)
    sin.copy_(img.to(DEV))
    for _ in range(3):
        gcls, gprob = replay()
        assert torch.equal(gcls, cls) and torch.equal(gprob, prob)
    xf = ref.preprocess_u8(img).to(DEV)
    assert (runner.logits(xf).double().cpu() - r).abs().max().item() <= tol
