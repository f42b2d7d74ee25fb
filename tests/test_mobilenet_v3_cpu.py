"""MobileNetV3 large / small without a GPU: the reference modules, their checkpoint round
trip, the 5x5 depthwise weight layout, and the packed programs' CPU emulation."""
import pytest
import torch

from idunno.models import checkpoint, packed
from idunno.models import reference as ref

MODELS = {
    "mobilenet_v3_large": (5_483_032, 11, 1280,
                           {"features.0.0.weight": (16, 3, 3, 3), "features.1.block.0.0.weight": (16, 1, 3, 3),
                            "features.4.block.2.fc1.weight": (24, 72, 1, 1), "features.4.block.2.fc2.bias": (72,),
                            "features.4.block.3.0.weight": (40, 72, 1, 1), "features.16.0.weight": (960, 160, 1, 1),
                            "classifier.3.weight": (1000, 1280)}),
    "mobilenet_v3_small": (2_542_856, 12, 1024,
                           {"features.1.block.1.fc1.weight": (8, 16, 1, 1), "features.12.0.weight": (576, 96, 1, 1),
                            "classifier.0.weight": (1024, 576)}),
}


@pytest.fixture(scope="module", params=sorted(MODELS))
def named(request):
    return request.param, ref.build(request.param, seed=1, randomize_bn=True)


def test_module_parameters_keys_and_names(named):
    from idunno.parallel.elastic import MODEL_IDS
    from idunno.runtime.jobstate import DEFAULT_BATCHSIZE

    name, model = named
    count, mid, _, keys = MODELS[name]
    assert sum(p.numel() for p in model.parameters()) == count
    sd = model.state_dict()
    assert {k: tuple(sd[k].shape) for k in keys} == keys
    size = name.rsplit("_", 1)[1]
    for alias in (f"mobilenetv3_{size}", f"mobilenet-v3-{size}", f"MobileNet_V3_{size}"):
        assert ref.canonical(alias) == name
    assert ref.canonical("mobilenet_v3") == "mobilenet_v3_large"
    assert MODEL_IDS[name] == mid and DEFAULT_BATCHSIZE[name] == 400
    assert all(bn.eps == 0.001 for bn in model.modules() if isinstance(bn, torch.nn.BatchNorm2d))


def test_checkpoint_round_trip(named):
    name, model = named
    got = checkpoint.load_model(name, model.state_dict())
    assert checkpoint.state_digest(got) == checkpoint.state_digest(model)
    bad = dict(model.state_dict())
    bad["classifier.3.weight"] = torch.zeros(10, MODELS[name][2])
    with pytest.raises(ValueError, match="classifier.3"):
        checkpoint.load_model(name, bad)


@pytest.mark.parametrize("dtype,rel", [("fp16", 2e-3), ("fp32", 1e-4)])
def test_emulated_program_matches_fp64_module(named, dtype, rel):
    """test_packing.py's bounds: 2e-3 of the logit scale for fp16 weights, 1e-4 for the fp32 fold."""
    name, model = named
    img = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        r = model.double()(ref.preprocess_u8(img).double())
    model.float()
    p = packed.compile_model(model, name, dtype)
    rows = ref.MOBILENET_V3_SETTINGS[name.rsplit("_", 1)[1]]
    assert p.kind == "mobilenet_v3" and len(p.mblocks) == len(rows) and p.mblocks[0].expand is None
    assert [(mb.dw.kh, mb.dw.stride, mb.se is not None, mb.dw.act) for mb in p.mblocks] == \
        [(k, s, se, 3 if hs else 1) for _, k, _, _, se, hs, s in rows]
    assert [mb.residual for mb in p.mblocks[:3]] == [name.endswith("large"), False, True]
    e = packed.emulate(p, img).double()
    assert (r - e).abs().max().item() < rel * r.abs().max().item()
    assert torch.equal(r.argmax(1), e.argmax(1))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_pack_unpack_5x5_round_trip(dtype):
    dt = torch.float16 if dtype == "fp16" else torch.float32
    w = torch.randn(24, 1, 5, 5)
    w25 = packed.pack_dw_weight(w, dtype)
    assert w25.shape == (25, 24) and w25.dtype == dt and torch.equal(w25[5 * 3 + 4], w[:, 0, 3, 4].to(dt))
    assert torch.equal(packed.unpack_dw_weight(w25), w.to(dt).float())


def test_program_flops_is_the_layer_sum(named):
    name, _ = named
    p = packed.build_program(name)
    rows = ref.MOBILENET_V3_SETTINGS[name.rsplit("_", 1)[1]]
    tot, h = 112 * 112 * 2 * 27 * 16, 112
    for cin, k, exp, cout, se, _, s in rows:
        ho = h // s
        tot += (h * h * 2 * cin * exp if exp != cin else 0) + ho * ho * 2 * k * k * exp + ho * ho * 2 * exp * cout
        tot += 2 * 2 * exp * ref._make_divisible(exp // 4) if se else 0
        h = ho
    c, last = rows[-1][3], MODELS[name][2]
    tot += 7 * 7 * 2 * c * 6 * c + 2 * 6 * c * last + 2 * last * 1000
    assert packed.program_flops(p) == tot
    assert p.param_bytes() == sum(c.w.numel() * 2 + c.b.numel() * 4 for c in p.all_convs())
