"""DenseNet without a GPU: packing, the fp32 emulation of the packed program against the module, the analytic FLOPs,
registration, a checkpoint round trip and the dense-layer band planner."""
import pytest
import torch

from idunno.models import checkpoint, packed
from idunno.models import reference as ref

NAMES = ("densenet121", "densenet169", "densenet201")
CONFIGS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_pack_unpack_dense_layer(dtype):
    layer = ref.build("densenet121", seed=3, randomize_bn=True).features.denseblock2.denselayer5
    d = packed.pack_dense_layer(layer, dtype)
    assert d.cin == 256 and tuple(d.w1.shape) == (128, 256) and tuple(d.w2.shape) == (32, 1152)
    assert d.scale1.dtype == d.b1.dtype == torch.float32 and d.w1.dtype == packed._dt(dtype)
    w1, w2 = packed.unpack_dense_layer(d)
    f1, fb = packed.fold_bn(layer.conv1.weight, None, layer.norm2)
    tol = 1e-3 if dtype == "fp16" else 0.0
    assert (w1 - f1).abs().max() <= tol * f1.abs().max() and torch.equal(d.b1, fb)
    assert (w2 - layer.conv2.weight).abs().max() <= tol * layer.conv2.weight.abs().max()
    # tap-major: k = (3 kh + kw) 128 + c
    assert d.w2[5, (3 * 2 + 1) * 128 + 17].float() == pytest.approx(layer.conv2.weight[5, 17, 2, 1].item(), rel=1e-3)


@pytest.mark.parametrize("name", NAMES)
def test_emulate_matches_module(name):
    m = ref.build(name, seed=7, randomize_bn=True)
    img = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        r = m(ref.preprocess_u8(img))
    y = packed.emulate(packed.compile_model(m, name, dtype="fp32"), img)
    assert (y - r).abs().max().item() <= 1e-4 * r.abs().max().item()


def test_program_flops_densenet121():
    macs, c, h = 112 * 112 * 64 * 147, 64, 56
    for i, n in enumerate(CONFIGS["densenet121"]):
        for j in range(n):
            macs += h * h * ((c + 32 * j) * 128 + 9 * 128 * 32)
        c += 32 * n
        if i < 3:
            macs += h * h * c * (c // 2)        # the module's conv runs before its pool
            c, h = c // 2, h // 2
    macs += c * 1000
    assert c == 1024
    assert packed.program_flops(packed.build_program("densenet121")) == 2.0 * macs


def test_names_ids_batch():
    from idunno.config import ClusterConfig
    from idunno.parallel.elastic import MODEL_IDS
    from idunno.runtime.jobstate import DEFAULT_BATCHSIZE

    assert [MODEL_IDS[n] for n in NAMES] == [15, 16, 17]
    for n in NAMES:
        assert ClusterConfig().batch_size[n] == 400 and DEFAULT_BATCHSIZE[n] == 400
        assert ref.canonical(n.replace("densenet", "DenseNet-")) == n
        assert ref.BUILDERS[n]().block_config == CONFIGS[n]
    assert ref.canonical("densenet") == "densenet121"
    with pytest.raises(ValueError):
        ref.canonical("densenet161")


def test_checkpoint_round_trip(tmp_path):
    m = ref.build("densenet121", seed=5, randomize_bn=True)
    state = m.state_dict()
    for key in ("features.conv0.weight", "features.norm0.running_var", "features.denseblock3.denselayer24.conv2.weight",
                "features.denseblock1.denselayer1.norm1.weight", "features.transition2.conv.weight",
                "features.transition1.norm.bias", "features.norm5.running_mean", "classifier.bias"):
        assert key in state
    path = tmp_path / "densenet121.pth"
    torch.save(state, path)
    back = checkpoint.load_model("densenet121", str(path))
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(back(x), m(x))


def test_dense_plan_every_served_shape():
    """Every (H, Cin, dtype) the three models launch plans within 160 KiB; an image of <= 14 rows is one band."""
    from idunno import ops

    shapes = set()
    for cfg in CONFIGS.values():
        c, h = 64, 56
        for i, n in enumerate(cfg):
            shapes |= {(h, c + 32 * j, c + 32 * n) for j in range(n)}
            c, h = (c + 32 * n) // 2, h // 2
    assert len(shapes) == 98 + (24 + 16) + (32 + 32)      # 201's layers, then 121's and 169's blocks 3 and 4
    for h, cin, ctot in sorted(shapes):
        assert ops.dense_layer_ok(h, h, cin, ctot)
        for f32 in (False, True):
            p = ops.dense_plan(h, h, cin, f32)
            assert 0 < p["lds"] <= 160 * 1024 and p["bands"] == -(-h // p["R"]) and p["kc"] % (16 if f32 else 32) == 0
            assert p["xbytes"] == 16 * p["mf"] * (p["kc"] * (4 if f32 else 2) + 16)
            if h <= 14:
                assert p["bands"] == 1
    assert not ops.dense_layer_ok(56, 56, 48, 96) and not ops.dense_layer_ok(56, 56, 64, 80)
    assert not ops.dense_layer_ok(56, 65, 64, 96)
