"""The fused ShuffleNetV2 unit (both strides) and the ShuffleNetV2 forward on the GPU, against fp64 oracles on the
CPU computed from operands rounded to the kernel's dtype.  Bounds are the suite's: test_densenet_gpu._check and its
whole-model logit bounds."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from idunno.models import packed
from idunno.models import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}
OPERANDS = ("w1", "b1", "wd", "bd", "w2", "b2", "wd1", "bd1", "wp1", "bp1")


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _check(y, r, dtype):
    y = y.double().cpu()
    scale, err = r.abs().max().item(), (y - r).abs().max().item()
    bound = 2e-5 * scale if dtype == "fp32" else 1e-2 * scale + 1e-3
    print(f"max err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}")
    assert err <= bound, f"max err {err:.3e} vs scale {scale:.3e}"


def _mixed(pre):
    neg = (pre < 0).double().mean().item()
    assert 0.1 < neg < 0.9, neg


def _case(cin, c, stride, shape, dtype):
    """A packed unit, its input with the pad channels at 7.0, and the fp64 halves (left, right) as NHWC.  Every folded
    bias has mean +0.5: a map border holding relu(b1), or a pad channel that is not zero, would show."""
    g = torch.Generator().manual_seed(cin + c + sum(shape))
    u = ref.ShuffleUnit(cin, c, stride).eval()
    for m in u.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) / (m.weight[0].numel() ** 0.5)
        elif isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.weight.data, m.bias.data = 0.5 + torch.rand(n, generator=g), 0.5 + 0.5 * torch.randn(n, generator=g)
            m.running_mean.data, m.running_var.data = 0.2 * torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g)
    pu = packed.pack_shuffle_unit(u, dtype)
    x = torch.full((*shape, -(-cin // 8) * 8), 7.0).to(DTYPES[dtype])
    x[..., :cin] = torch.randn(*shape, cin, generator=g).to(DTYPES[dtype])
    w = {k: v.double() for k, v in packed.unpack_shuffle_unit(pu).items()}
    xl, h = x[..., :cin].double().permute(0, 3, 1, 2), c // 2
    if stride == 1:
        left, t = xl[:, :h], xl[:, h:]
    else:
        pre = F.conv2d(F.conv2d(xl, w["wd1"], w["bd1"], 2, 1, groups=cin), w["wp1"], w["bp1"])
        _mixed(pre)
        left, t = F.relu(pre), xl
    pre1 = F.conv2d(t, w["w1"], w["b1"])
    pre2 = F.conv2d(F.conv2d(F.relu(pre1), w["wd"], w["bd"], stride, 1, groups=h), w["w2"], w["b2"])
    _mixed(pre1)
    _mixed(pre2)
    return pu, x, left.permute(0, 2, 3, 1), F.relu(pre2).permute(0, 2, 3, 1)


def _run(ops, pu, x):
    dev = lambda t: None if t is None else t.to(DEV)
    return ops.shuffle_unit(x.to(DEV), *(dev(getattr(pu, k)) for k in OPERANDS[:6]), stride=pu.stride,
                            **{k: dev(getattr(pu, k)) for k in OPERANDS[6:]}, c=pu.c).cpu()


# (B, H, W, c); the last one is ragged in both precisions (the issue's 28 rows split evenly in fp32)
S1_CASES = [(1, 1, 1, 48), (2, 3, 5, 48), (1, 7, 7, 464), (3, 7, 7, 192), (1, 14, 14, 232), (1, 28, 28, 116),
            (1, 26, 28, 176)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_stride1_cases_hold_a_ragged_band_and_a_shared_workgroup(ops, dtype):
    plans = [ops.shuffle_plan(H, W, c, c, 1, dtype == "fp32") | {"H": H} for _, H, W, c in S1_CASES]
    assert any(p["bands"] >= 2 and p["H"] % p["R"] for p in plans)
    assert any(p["imgs"] >= 2 for p in plans)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", S1_CASES)
def test_stride1_unit_vs_fp64(ops, case, dtype):
    B, H, W, c = case
    pu, x, left, right = _case(c, c, 1, (B, H, W), dtype)
    got = _run(ops, pu, x)
    assert tuple(got.shape) == (B, H, W, x.shape[3]) and got.dtype == x.dtype
    _check(got[..., 1:c:2], right, dtype)
    assert torch.equal(got[..., 0:c:2], x[..., :c // 2])         # x1 is copied: bit-equal
    assert bool((got[..., c:] == 0).all())                       # the pad of width 116


# (B, H, W, cin, c)
S2_CASES = [(1, 2, 2, 24, 48), (2, 5, 7, 24, 116), (1, 56, 56, 24, 176), (1, 28, 28, 116, 232), (1, 14, 14, 352, 704)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", S2_CASES)
def test_stride2_unit_vs_fp64(ops, case, dtype):
    B, H, W, cin, c = case
    pu, x, left, right = _case(cin, c, 2, (B, H, W), dtype)
    got = _run(ops, pu, x)
    assert tuple(got.shape) == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, -(-c // 8) * 8)
    _check(got[..., 0:c:2], left, dtype)
    _check(got[..., 1:c:2], right, dtype)
    assert bool((got[..., c:] == 0).all())


@pytest.mark.parametrize("what,match", [("h", "w2: must be"), ("dtype", "w1 has wrong dtype"),
                                         ("view", "x must be contiguous"), ("stride3", "stride must be 1 or 2"),
                                         ("branch1", "stride 2 needs branch 1")])
def test_binding_rejections(ops, what, match):
    z = lambda *shape, dt=torch.float16: torch.zeros(*shape, dtype=dt, device=DEV)
    f = lambda n: torch.zeros(n, device=DEV)
    x = z(1, 4, 4, 96)[..., :48] if what == "view" else z(1, 4, 4, 48)
    w1 = z(32, 32, dt=torch.float32 if what == "dtype" else torch.float16)
    w2 = z(64, 64) if what == "h" else z(32, 32)
    args = (x, w1, f(32), z(9, 32), f(32), w2, f(32))
    with pytest.raises(RuntimeError, match=match):
        if what == "branch1":
            ops.shuffle_unit(z(1, 4, 4, 24), z(32, 32), *args[2:], stride=2, c=48)
        else:
            ops.shuffle_unit(*args, stride=3 if what == "stride3" else 1)
    assert tuple(ops.shuffle_unit(z(1, 4, 4, 48), z(32, 32), *args[2:5], z(32, 32), f(32)).shape) == (1, 4, 4, 48)


@pytest.mark.parametrize("dtype,rel", [("fp16", 0.03), ("fp32", 1e-4)])
@pytest.mark.parametrize("name", ["shufflenet_v2_x0_5", "shufflenet_v2_x1_0", "shufflenet_v2_x1_5"])
def test_model_vs_fp64_module(ops, name, dtype, rel):
    """B = 2, randomised BN: logits within the suite's whole-model bound of the fp64 module's, the same top-1
    wherever the oracle's top-2 gap exceeds it, three bit-equal graph replays, and the float batch of the same
    images within the same bound."""
    from idunno.models import HipRunner, compile_model

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
