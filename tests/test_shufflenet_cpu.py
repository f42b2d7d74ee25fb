"""ShuffleNetV2 without a GPU: packing, the fp32 emulation of the packed program against the module, the analytic
FLOPs, registration, a checkpoint round trip and the fused unit's band planner."""
import pytest
import torch

from idunno.models import checkpoint, packed
from idunno.models import reference as ref

NAMES = ("shufflenet_v2_x0_5", "shufflenet_v2_x1_0", "shufflenet_v2_x1_5")
WIDTHS = {"shufflenet_v2_x0_5": (48, 96, 192), "shufflenet_v2_x1_0": (116, 232, 464),
          "shufflenet_v2_x1_5": (176, 352, 704)}


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_pack_unpack_units(dtype):
    m = ref.build("shufflenet_v2_x1_0", seed=3, randomize_bn=True)
    tol = 1e-3 if dtype == "fp16" else 0.0
    close = lambda a, b: (a - b).abs().max() <= tol * b.abs().max()
    # stride 1 at width 116: h = 58, k0 = 56; columns 0, 1 (x1's last channels) and from 60 (the pad, the K fill) zero
    u = m.stage2[1]
    s1 = packed.pack_shuffle_unit(u, dtype)
    hp = 64
    assert (s1.cin, s1.c, s1.stride) == (116, 116, 1) and tuple(s1.w1.shape) == (hp, 64) and s1.wd1 is None
    assert tuple(s1.wd.shape) == (9, hp) and tuple(s1.w2.shape) == (hp, hp) and s1.b1.dtype == torch.float32
    assert not s1.w1[:, :2].any() and not s1.w1[:, 60:].any() and not s1.w1[58:].any() and not s1.b1[58:].any()
    assert not s1.wd[:, 58:].any() and not s1.w2[58:].any() and not s1.w2[:, 58:].any()
    w = packed.unpack_shuffle_unit(s1)
    f1, fb1 = packed.fold_bn(u.branch2[0].weight, None, u.branch2[1])
    fd, _ = packed.fold_bn(u.branch2[3].weight, None, u.branch2[4])
    assert close(w["w1"], f1) and torch.equal(w["b1"], fb1) and close(w["wd"], fd)
    assert s1.wd[3 * 2 + 1, 17].float() == pytest.approx(fd[17, 0, 2, 1].item(), rel=1e-3)     # tap-major
    # stride 2 from width 116 (stored as 120): the rows of channels 116 .. 119 are zero in every weight
    u = m.stage3[0]
    s2 = packed.pack_shuffle_unit(u, dtype)
    assert (s2.cin, s2.c, s2.stride) == (116, 232, 2) and tuple(s2.w1.shape) == tuple(s2.wp1.shape) == (128, 128)
    assert not s2.w1[:, 116:].any() and not s2.wp1[:, 116:].any() and not s2.wd1[:, 116:].any() and not s2.bd1[116:].any()
    w = packed.unpack_shuffle_unit(s2)
    fp, fbp = packed.fold_bn(u.branch1[2].weight, None, u.branch1[3])
    assert close(w["wp1"], fp) and torch.equal(w["bp1"], fbp) and tuple(w["wd1"].shape) == (116, 1, 3, 3)


@pytest.mark.parametrize("name", NAMES)
def test_emulate_matches_module(name):
    m = ref.build(name, seed=7, randomize_bn=True)
    img = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        r = m(ref.preprocess_u8(img))
    y = packed.emulate(packed.compile_model(m, name, dtype="fp32"), img)
    assert (y - r).abs().max().item() <= 1e-4 * r.abs().max().item()


def test_program_flops_x1_0():
    macs, cin, hw = 112 * 112 * 24 * 27, 24, 56
    for c, n in zip(WIDTHS["shufflenet_v2_x1_0"], (4, 8, 4)):
        h, ho = c // 2, hw // 2
        macs += hw * hw * cin * h + ho * ho * (9 * h + h * h)         # stride 2, branch 2: pw1 at the input size
        macs += ho * ho * (9 * cin + cin * h)                         # branch 1
        macs += (n - 1) * ho * ho * (2 * h * h + 9 * h)
        cin, hw = c, ho
    macs += 7 * 7 * 464 * 1024 + 1024 * 1000
    assert packed.program_flops(packed.build_program("shufflenet_v2_x1_0")) == 2.0 * macs


def test_names_ids_batch():
    from idunno.config import ClusterConfig
    from idunno.parallel.elastic import MODEL_IDS
    from idunno.runtime.jobstate import DEFAULT_BATCHSIZE

    assert [MODEL_IDS[n] for n in NAMES] == [18, 19, 20]
    for n in NAMES:
        assert ClusterConfig().batch_size[n] == 400 and DEFAULT_BATCHSIZE[n] == 400
        assert ref.canonical(n.replace("shufflenet_v2_", "ShuffleNetV2-").replace("_", ".")) == n
        assert ref.BUILDERS[n]().widths == WIDTHS[n]
    assert ref.canonical("shufflenet") == ref.canonical("shufflenet_v2") == "shufflenet_v2_x1_0"
    with pytest.raises(ValueError):
        ref.canonical("shufflenet_v2_x2_0")


def test_checkpoint_round_trip(tmp_path):
    m = ref.build("shufflenet_v2_x0_5", seed=5, randomize_bn=True)
    state = m.state_dict()
    for key in ("conv1.0.weight", "conv1.1.running_var", "stage2.0.branch1.0.weight", "stage2.0.branch1.3.bias",
                "stage3.7.branch2.5.weight", "stage4.3.branch2.6.running_mean", "conv5.0.weight", "conv5.1.weight",
                "fc.bias"):
        assert key in state
    assert not any(k.startswith("stage2.1.branch1") for k in state)
    path = tmp_path / "shufflenet.pth"
    torch.save(state, path)
    back = checkpoint.load_model("shufflenet_v2_x0_5", str(path))
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(back(x), m(x))


def test_shuffle_plan_every_served_shape():
    """Every unit shape the three models launch plans within 160 KiB, in whole bands, and as one band exactly when
    the whole image fits."""
    from idunno import ops

    shapes = set()
    for widths in WIDTHS.values():
        cin, hw = 24, 56
        for c in widths:
            shapes |= {(hw, cin, c, 2), (hw // 2, c, c, 1)}
            cin, hw = c, hw // 2
    assert len(shapes) == 18
    for hw, cin, c, stride in sorted(shapes):
        assert ops.shuffle_unit_ok(hw, hw, cin, c, stride)
        for f32 in (False, True):
            p = ops.shuffle_plan(hw, hw, cin, c, stride, f32)
            ho = hw if stride == 1 else hw // 2
            assert 0 < p["lds"] <= 160 * 1024 and p["bands"] == -(-ho // p["R"]) and p["Cp"] == -(-c // 8) * 8
            assert (p["bands"] == 1) == (p["lds_whole"] <= 160 * 1024)
            assert p["imgs"] == 1 or (p["bands"] == 1 and stride == 1 and p["imgs"] * hw * hw >= 64)
    assert not ops.shuffle_unit_ok(28, 28, 24, 48, 1) and not ops.shuffle_unit_ok(28, 28, 47, 47, 1)
    assert not ops.shuffle_unit_ok(28, 300, 48, 48, 1)
