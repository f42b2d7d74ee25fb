"""The rest of torchvision v0.10's ResNet family (ResNet101/152, ResNeXt, Wide
ResNet) on the CPU: architectures and names, checkpoint loading, the
channel-block-local packing of grouped 3x3 convs, emulation and the FLOP count."""
import pytest
import torch
import torch.nn.functional as F

from idunno.models import packed as P
from idunno.models import reference as ref
from idunno.models.checkpoint import load_state, model_from_state, state_digest
from idunno.models.packed import Conv

# torchvision v0.10 parameter counts, recomputed from the layer lists
PARAMS = {
    "resnet101": 44_549_160,
    "resnet152": 60_192_808,
    "resnext50_32x4d": 25_028_904,
    "resnext101_32x8d": 88_791_336,
    "wide_resnet50_2": 68_883_240,
    "wide_resnet101_2": 126_886_696,
}
# state_digest(build(name, seed=0)) before the family grew: builders, init order and seeds are unchanged
DIGESTS = {
    "resnet18": "85cd971c81b539e3d977a13d84de3ae3e5c744a07945fafa168bc332bb99805e",
    "resnet50": "5e95559bdb40d5fc9f93d0c2dd85eef686c432ec4e5d7f992eb174c9652f690a",
}


def _count(name):
    with torch.device("meta"):
        m = ref.BUILDERS[name]()
    return sum(p.numel() for p in m.parameters())


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_parameter_counts_match_torchvision(name):
    assert _count(name) == PARAMS[name]


def test_resnet50_parameter_count_unchanged():
    assert _count("resnet50") == 25_557_032


def test_resnext50_state_dict_keys_and_grouped_shape():
    with torch.device("meta"):
        a, b = ref.BUILDERS["resnext50_32x4d"]().state_dict(), ref.BUILDERS["resnet50"]().state_dict()
    assert list(a) == list(b)
    assert tuple(a["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(a["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
    assert tuple(a["layer1.0.conv3.weight"].shape) == (256, 128, 1, 1)


def test_resnext50_checkpoint_round_trip_and_refused_as_resnet50(tmp_path):
    m = ref.build("resnext50_32x4d", seed=1)
    path = tmp_path / "resnext50_32x4d.pth"
    torch.save(m.state_dict(), path)
    state = load_state(path)
    got = model_from_state("resnext50_32x4d", state)
    assert state_digest(got) == state_digest(m)
    assert state_digest(model_from_state("resnext50", state)) == state_digest(m)     # the alias
    with pytest.raises(ValueError, match=r"conv2"):
        model_from_state("resnet50", state)


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_seeded_weights_of_existing_builders_unchanged(name):
    assert state_digest(ref.build(name, seed=0)) == DIGESTS[name]


def _grouped(cg, seed=0):
    groups = 4 if cg >= 32 else 8
    c = cg * groups
    g = torch.Generator().manual_seed(seed + cg)
    return torch.randn(c, cg, 3, 3, dtype=torch.float64, generator=g) / (9 * cg) ** 0.5, groups, c


def _conv_of(w, groups, **kw):
    c = w.shape[0]
    return Conv(w=kw.pop("w16", None), b=torch.zeros(c), cin=c, cout=c, kh=3, kw=3, stride=1, pad=1, relu=False,
                groups=groups, **kw)


@pytest.mark.parametrize("cg", P.GROUPED_CG)
def test_grouped_pack_unpack_and_zero_slots(cg):
    w, groups, c = _grouped(cg)
    cb = P.grouped_block(cg)
    assert cb == max(16, cg)
    pw = P.pack_grouped_weight(w, groups)
    assert pw.dtype == torch.float16 and tuple(pw.shape) == (c, 9 * cb)
    assert torch.equal(P.unpack_grouped_weight(_conv_of(w, groups, w16=pw)), w.float().half().float())
    sw, scale = P.pack_grouped_split_weight(w, groups)
    assert sw.dtype == torch.float16 and tuple(sw.shape) == (c, 2 * 9 * cb)
    back = P.unpack_grouped_weight(_conv_of(w, groups, w16=w.float(), sw=sw, s_scale=scale)).double()
    assert (back - w).abs().max().item() <= 2.0 ** -22 * w.abs().max().item()
    # the same exponent rule as pack_split_weight: the largest scaled weight in [2^13, 2^14)
    top = (sw[:, :9 * cb].double() + sw[:, 9 * cb:].double()).abs().max().item()
    assert 2.0 ** 13 <= top < 2.0 ** 14 and scale == 1.0 / round(1.0 / scale)
    # every slot outside an output's own group is exactly zero, every slot inside holds its weight
    co = torch.arange(c)
    own = ((co % cb) // cg).view(c, 1, 1) == (torch.arange(cb) // cg).view(1, 1, cb)          # [c, 1, cb]
    for rows in (pw, sw[:, :9 * cb], sw[:, 9 * cb:]):
        r = rows.reshape(c, 9, cb)
        assert not r[~own.expand(c, 9, cb)].any()
    assert int((pw.reshape(c, 9, cb) != 0).sum()) == int((w.float().half() != 0).sum())


@pytest.mark.parametrize("cg", P.GROUPED_CG)
def test_expanded_dense_weight_computes_the_grouped_conv(cg):
    w, groups, c = _grouped(cg, seed=3)
    g = torch.Generator().manual_seed(cg)
    x = torch.randn(2, c, 6, 5, dtype=torch.float64, generator=g)
    dense = P.expand_grouped_weight(w, groups)
    assert tuple(dense.shape) == (c, c, 3, 3) and int((dense != 0).sum()) == int((w != 0).sum())
    for stride in (1, 2):
        want = F.conv2d(x, w, None, stride, 1, groups=groups)
        got = F.conv2d(x, dense, None, stride, 1)
        # the extra products are exact zeros; only fp64 summation order may differ
        assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()


@pytest.mark.parametrize("cg", [2, 12])
def test_packing_refuses_other_group_sizes(cg):
    w = torch.randn(4 * cg, cg, 3, 3)
    for pack in (P.pack_grouped_weight, P.pack_grouped_split_weight):
        with pytest.raises(ValueError, match=rf"\b{cg}\b.*channels per group"):
            pack(w, 4)
    with pytest.raises(ValueError, match=rf"\b{cg}\b"):
        P.grouped_block(cg)


@pytest.mark.parametrize("name", ["resnext50_32x4d", "wide_resnet50_2"])
def test_emulated_fp32_program_matches_module(name):
    from idunno.runtime.data import synth_images_cpu

    m = ref.build(name, seed=0)
    prog = P.compile_model(m, name, "fp32")
    img = torch.from_numpy(synth_images_cpu(0, 0, 1))[:, :64, :64].contiguous()
    got = P.emulate(prog, img).double()
    with torch.no_grad():
        want = m(ref.preprocess_u8(img)).double()
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err <= 1e-5, f"{name}: rel logit err {err:.2e}"


def test_resnext_programs_carry_no_dense_expansion():
    m = ref.build("resnext50_32x4d", seed=0)
    for dtype in ("fp32", "fp16"):
        prog = P.compile_model(m, "resnext50_32x4d", dtype)
        mids = [b.convs[1] for b in prog.blocks]
        assert all(c.groups == 32 and c.cin == c.cout for c in mids)
        for c in mids:
            cb = P.grouped_block(c.cin // 32)
            if dtype == "fp32":
                assert tuple(c.w.shape) == (c.cout, c.cin // 32, 3, 3) and c.w.dtype == torch.float32
                assert tuple(c.sw.shape) == (c.cout, 2 * 9 * cb) and c.wino is None
            else:
                assert tuple(c.w.shape) == (c.cout, 9 * cb) and c.w.dtype == torch.float16 and c.sw is None
        # no tensor of a grouped conv is as large as its dense [Cout, Cin, 3, 3] form
        for c in mids:
            for t in (c.w, c.sw):
                assert t is None or t.numel() < c.cout * c.cin * 9
    assert all(c.sw is not None for b in P.compile_model(m, "resnext50_32x4d", "fp32").blocks
               for c in [*b.convs, *([b.down] if b.down else [])])


def test_program_flops_divides_grouped_convs_by_groups():
    prog = P.compile_model(ref.build("resnext50_32x4d", seed=0), "resnext50_32x4d", "fp16")
    tot = 2 * 3 * 49 * 64 * 112 * 112                      # stem 7x7/2
    h, cin = 56, 64
    for i, (n, planes) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512))):
        width = planes * 2                                 # int(planes * 4 / 64) * 32
        for j in range(n):
            s = 2 if i > 0 and j == 0 else 1
            ho = h // s
            tot += 2 * cin * width * h * h                 # 1x1 reduce at the input resolution
            tot += 2 * width * 9 * width * ho * ho // 32   # grouped 3x3 (the stride sits here)
            tot += 2 * width * planes * 4 * ho * ho        # 1x1 expand
            if j == 0:
                tot += 2 * cin * planes * 4 * ho * ho      # downsample
            h, cin = ho, planes * 4
    tot += 2 * 2048 * 1000
    assert P.program_flops(prog) == tot


def test_names_ids_and_batch_sizes():
    from idunno.config import ClusterConfig
    from idunno.parallel.elastic import MODEL_IDS
    from idunno.runtime.jobstate import DEFAULT_BATCHSIZE

    for alias, name in {"resnext50": "resnext50_32x4d", "resnext101": "resnext101_32x8d",
                        "wide_resnet50": "wide_resnet50_2", "wide_resnet101": "wide_resnet101_2",
                        "resnet-101": "resnet101", "resnet-152": "resnet152", "ResNeXt50_32x4d": "resnext50_32x4d",
                        "resnet": "resnet18", "resnet-50": "resnet50"}.items():
        assert ref.canonical(alias) == name
    with pytest.raises(ValueError, match="unknown model"):
        ref.canonical("resnext101_64x4d")
    assert {k: MODEL_IDS[k] for k in ("alexnet", "resnet18", "resnet50", "resnet34")} == \
        {"alexnet": 0, "resnet18": 1, "resnet50": 2, "resnet34": 3}
    assert len(set(MODEL_IDS.values())) == len(MODEL_IDS) and set(MODEL_IDS) == set(ref.BUILDERS)
    assert [MODEL_IDS[n] for n in ("resnet101", "resnet152", "resnext50_32x4d", "resnext101_32x8d",
                                   "wide_resnet50_2", "wide_resnet101_2")] == [4, 5, 6, 7, 8, 9]
    cfg = ClusterConfig()
    for name in PARAMS:
        assert cfg.batch_size[name] == 400 and DEFAULT_BATCHSIZE[name] == 400
