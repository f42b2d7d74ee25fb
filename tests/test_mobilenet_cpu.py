"""MobileNetV2 without a GPU: the reference module, its checkpoint round trip, the
depthwise / pointwise weight layouts, and the packed program's CPU emulation."""
import pytest
import torch

from idunno.models import checkpoint, packed
from idunno.models import reference as ref

KEYS = {"features.0.0.weight": (32, 3, 3, 3), "features.1.conv.0.0.weight": (32, 1, 3, 3),
        "features.1.conv.1.weight": (16, 32, 1, 1), "features.2.conv.0.0.weight": (96, 16, 1, 1),
        "features.2.conv.1.0.weight": (96, 1, 3, 3), "features.2.conv.2.weight": (24, 96, 1, 1),
        "features.2.conv.3.running_var": (24,), "features.18.0.weight": (1280, 320, 1, 1),
        "classifier.1.weight": (1000, 1280)}


@pytest.fixture(scope="module")
def model():
    return ref.build("mobilenet_v2", seed=1, randomize_bn=True)


def test_module_parameters_keys_and_names(model):
    from idunno.parallel.elastic import MODEL_IDS

    assert sum(p.numel() for p in model.parameters()) == 3_504_872
    sd = model.state_dict()
    assert {k: tuple(sd[k].shape) for k in KEYS} == KEYS
    for alias in ("mobilenet", "mobilenetv2", "mobilenet-v2", "MobileNet_V2"):
        assert ref.canonical(alias) == "mobilenet_v2"
    assert MODEL_IDS["mobilenet_v2"] == 10


def test_checkpoint_round_trip(model):
    got = checkpoint.load_model("mobilenet_v2", model.state_dict())
    assert checkpoint.state_digest(got) == checkpoint.state_digest(model)
    bad = dict(model.state_dict())
    bad["classifier.1.weight"] = torch.zeros(10, 1280)
    with pytest.raises(ValueError, match="classifier.1"):
        checkpoint.load_model("mobilenet_v2", bad)


@pytest.mark.parametrize("dtype,rel", [("fp16", 2e-3), ("fp32", 1e-4)])
def test_emulated_program_matches_fp64_module(model, dtype, rel):
    """test_packing.py's bounds for the other kinds: 2e-3 of the logit scale for fp16 weights,
    1e-4 for the fp32 fold."""
    torch.manual_seed(0)
    img = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8)
    with torch.no_grad():
        r = model.double()(ref.preprocess_u8(img).double())
    model.float()
    p = packed.compile_model(model, "mobilenet_v2", dtype)
    assert p.kind == "mobilenet" and len(p.mblocks) == 17 and p.mblocks[0].expand is None
    assert [mb.residual for mb in p.mblocks[:4]] == [False, False, True, False]
    e = packed.emulate(p, img).double()
    assert (r - e).abs().max().item() < rel * r.abs().max().item()
    assert torch.equal(r.argmax(1), e.argmax(1))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_pack_unpack_round_trips(dtype):
    dt = torch.float16 if dtype == "fp16" else torch.float32
    w = torch.randn(24, 1, 3, 3)
    w9 = packed.pack_dw_weight(w, dtype)
    assert w9.shape == (9, 24) and w9.dtype == dt and torch.equal(w9[5], w[:, 0, 1, 2].to(dt))
    assert torch.equal(packed.unpack_dw_weight(w9), w.to(dt).float())
    for k, kp16, kp32 in [(24, 32, 32), (144, 160, 144), (16, 32, 16), (320, 320, 320)]:
        w = torch.randn(40, k, 1, 1)
        wp = packed.pack_pw_weight(w, dtype)
        assert wp.shape == (40, kp16 if dtype == "fp16" else kp32) and wp.dtype == dt
        assert wp[:, k:].abs().sum().item() == 0
        assert torch.equal(packed.unpack_pw_weight(wp, k), w.to(dt).float())


def test_program_flops_is_the_layer_sum():
    p = packed.build_program("mobilenet_v2")
    tot, h, cin = 112 * 112 * 2 * 27 * 32, 112, 32
    for t, c, n, s in ref.MOBILENET_V2_SETTINGS:
        for i in range(n):
            hid, ho = cin * t, h // (s if i == 0 else 1)
            tot += (h * h * 2 * cin * hid if t != 1 else 0) + ho * ho * 2 * 9 * hid + ho * ho * 2 * hid * c
            h, cin = ho, c
    tot += 7 * 7 * 2 * 320 * 1280 + 2 * 1280 * 1000
    assert packed.program_flops(p) == tot
    assert p.param_bytes() == sum(c.w.numel() * 2 + c.b.numel() * 4 for c in p.all_convs())
