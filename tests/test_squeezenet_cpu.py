"""SqueezeNet without a GPU: Fire weight packing, the packed program against the module, FLOPs,
names and checkpoints."""
import pytest
import torch

from idunno.models import checkpoint, compile_model, packed
from idunno.models import reference as ref
from idunno.parallel.elastic import MODEL_IDS


def _perturbed(name):
    m = ref.build(name, seed=3)
    g = torch.Generator().manual_seed(5)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.bias.data = 0.1 * torch.randn(mod.out_channels, generator=g)
    return m


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("s,e1,e3", [(16, 64, 64), (48, 192, 176)])
def test_fire_pack_round_trip(s, e1, e3, dtype):
    g = torch.Generator().manual_seed(s)
    dt = torch.float16 if dtype == "fp16" else torch.float32
    w1 = torch.randn(e1, s, 1, 1, generator=g).to(dt).float()
    w3 = torch.randn(e3, s, 3, 3, generator=g).to(dt).float()
    we = packed.pack_fire_weights(w1, w3, dtype)
    assert we.dtype == dt and tuple(we.shape) == (e1 + e3, packed.fire_kpad(s, dtype))
    assert packed.fire_kpad(s, dtype) % (32 if dtype == "fp16" else 16) == 0
    u1, u3 = packed.unpack_fire_weights(we, e1, s)
    assert torch.equal(u1, w1) and torch.equal(u3, w3)
    assert we.float().abs().sum().item() == pytest.approx((w1.abs().sum() + w3.abs().sum()).item(), rel=1e-6)
    assert we[e1, 4 * s + 1] == w3[0, 1, 1, 1]              # tap-major: k = (3 kh + kw) S + c
    with pytest.raises(ValueError, match="S must be"):
        packed.pack_fire_weights(torch.zeros(16, 24, 1, 1), torch.zeros(16, 24, 3, 3), dtype)


@pytest.mark.parametrize("name", ["squeezenet1_0", "squeezenet1_1"])
def test_emulate_matches_module(name):
    m = _perturbed(name)
    img = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = m(ref.preprocess_u8(img))
    p = compile_model(m, name, dtype="fp32")
    assert p.kind == "squeezenet" and [k for k, _ in p.features].count("fire") == 8
    got = packed.emulate(p, img)
    assert tuple(got.shape) == (2, 1000)
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_program_flops_and_bytes():
    p = compile_model(ref.build("squeezenet1_1"), "squeezenet1_1")
    fires = [(64, 16, 64, 64, 55), (128, 16, 64, 64, 55), (128, 32, 128, 128, 27), (256, 32, 128, 128, 27),
             (256, 48, 192, 192, 13), (384, 48, 192, 192, 13), (384, 64, 256, 256, 13), (512, 64, 256, 256, 13)]
    macs = 111 * 111 * 27 * 64 + sum(h * h * (c * s + s * e1 + 9 * s * e3) for c, s, e1, e3, h in fires) \
        + 13 * 13 * 512 * 1000
    assert packed.program_flops(p) == 2 * macs
    assert p.param_bytes() > 2 * 1_235_496                   # fp16, K padding and the 1x1 rows' zero taps on top


def test_names_and_ids():
    for alias in ("squeezenet", "squeezenet1.1", "squeezenet-1.1"):
        assert ref.canonical(alias) == "squeezenet1_1"
    for alias in ("squeezenet1.0", "squeezenet-1.0"):
        assert ref.canonical(alias) == "squeezenet1_0"
    assert (MODEL_IDS["squeezenet1_0"], MODEL_IDS["squeezenet1_1"]) == (13, 14)


def test_checkpoint_round_trip_and_head_check():
    m = _perturbed("squeezenet1_0")
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert "features.3.squeeze.weight" in state and "features.12.expand3x3.bias" in state
    back = checkpoint.model_from_state("squeezenet1.0", state)
    assert checkpoint.state_digest(back) == checkpoint.state_digest(m)
    state["classifier.1.weight"] = torch.zeros(10, 512, 1, 1)
    state["classifier.1.bias"] = torch.zeros(10)
    with pytest.raises(ValueError, match="10 classes; only 1000-class"):
        checkpoint.model_from_state("squeezenet1_0", state)
