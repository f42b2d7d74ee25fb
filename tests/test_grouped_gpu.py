"""Grouped 3x3 conv kernel (conv3x3_grouped.hip) and the models it serves
(ResNeXt; ResNet101 and Wide ResNet on the existing kernels) on the GPU.

Kernel oracle: ``F.conv2d(groups=)`` in fp64 on the same fp32 inputs, computed
once per case on the CPU and shared by the four (form, ReLU) variants.
Tolerances are the suite's own: split <= 2e-5 of the output scale
(tests/test_split.py::_check), fp16 <= 1e-2 * scale + 1e-3
(tests/test_kernels_gpu.py::_check)."""
import ast
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from idunno.models import HipRunner
from idunno.models import packed as P
from idunno.models import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _check_split(y, want, rel=2e-5):
    scale = want.abs().max().item() + 1e-12
    err = (y.double() - want).abs().max().item()
    print(f"split: max err {err:.3e}, scale {scale:.3e}, rel {err / scale:.2e}")
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


def _check_f16(y, want, tol=1e-2):
    scale = want.abs().max().item() + 1e-6
    err = (y.double() - want).abs().max().item()
    print(f"fp16: max err {err:.3e}, scale {scale:.3e}, rel {err / scale:.2e}")
    assert err <= tol * scale + 1e-3, f"max err {err} vs scale {scale}"


CASES = [
    # (B, H, W, C, groups, stride)
    (2, 56, 56, 128, 32, 1),     # Cg 4, the layer-1 shape
    (1, 9, 13, 64, 16, 1),       # Cg 4, H != W, nothing a tile multiple
    (3, 15, 15, 64, 8, 2),       # Cg 8, odd H at stride 2
    (2, 28, 28, 256, 32, 1),     # Cg 8
    (2, 14, 14, 512, 32, 2),     # Cg 16
    (3, 7, 7, 1024, 32, 1),      # Cg 32, M = 147
    (1, 7, 7, 2048, 32, 1),      # Cg 64
    (1, 1, 1, 64, 16, 1),        # every tap but the centre is padding
    (1, 2, 5, 128, 32, 2),       # tiny, strided
    (40, 28, 28, 128, 32, 1),    # more tiles than CUs (one workgroup per tile and 64-channel slab)
    # beyond the list the kernel was specified with: the code's other paths
    (1, 5, 6, 96, 24, 1),        # C % 64 == 32: the last slab is half a slab (two idle waves)
    (2, 9, 17, 160, 5, 2),       # Cg 32 at stride 2 with a half slab, Wo = 9 inside one 16-column tile
    (1, 10, 33, 64, 4, 1),       # Cg 16: two tile rows and three tile columns, the last of one column
]


@functools.lru_cache(maxsize=None)
def _case(case):
    """(x fp32 NHWC, w [C, Cg, 3, 3], bias, fp64 NHWC conv without ReLU), on the
    CPU.  One group's input channels are 64 x the others': a tap leaked from a
    neighbouring group of the same 16-channel block then sits far above tolerance."""
    B, H, W, C, groups, stride = case
    cg = C // groups
    g = torch.Generator().manual_seed(sum(case) + 1000 * groups)
    x = torch.randn(B, H, W, C, generator=g)
    hot = 1 % groups
    x[..., hot * cg:(hot + 1) * cg] *= 64.0
    w = torch.randn(C, cg, 3, 3, generator=g) / (9 * cg) ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride, 1, groups=groups)
    return x, w, b, y.permute(0, 2, 3, 1).contiguous()


def _want(case, relu):
    y = _case(case)[3]
    return F.relu(y) if relu else y


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_grouped_split_kernel_vs_fp64(ops, case, relu):
    B, H, W, C, groups, stride = case
    assert ops.conv3x3_grouped_ok(C, groups, stride)
    x, w, b, _ = _case(case)
    sw, scale = P.pack_grouped_split_weight(w, groups)
    y = ops.conv3x3_grouped_split(ops.split_from_f32(x.to(DEV)), sw.to(DEV), b.to(DEV), scale, groups, stride, relu)
    want = _want(case, relu)
    assert y.dtype == torch.float16 and tuple(y.shape) == (*want.shape[:3], 2 * C)
    _check_split(ops.f32_from_split(y).cpu(), want)
    assert torch.equal(P.from_split(y.cpu()), ops.f32_from_split(y).cpu())


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_grouped_f16_kernel_vs_fp64(ops, case, relu):
    B, H, W, C, groups, stride = case
    x, w, b, _ = _case(case)
    y = ops.conv3x3_grouped(x.to(DEV).half(), P.pack_grouped_weight(w, groups).to(DEV), b.to(DEV), groups, stride, relu)
    want = _want(case, relu)
    assert y.dtype == torch.float16 and tuple(y.shape) == tuple(want.shape)
    _check_f16(y.cpu(), want)


def test_grouped_ok_rule(ops):
    assert ops.conv3x3_grouped_ok(128, 32, 1) and ops.conv3x3_grouped_ok(2048, 32, 2)
    assert not ops.conv3x3_grouped_ok(96, 8, 1)        # Cg 12
    assert not ops.conv3x3_grouped_ok(128, 32, 3)      # stride 3
    assert not ops.conv3x3_grouped_ok(128, 1, 1)       # not grouped
    assert not ops.conv3x3_grouped_ok(48, 12, 1)       # C % 32
    assert not ops.conv3x3_grouped_ok(128, 24, 1)      # C % groups


def test_grouped_empty_batch_returns_at_once(ops):
    w = torch.zeros(64, 9 * 16, dtype=torch.float16, device=DEV)
    y = ops.conv3x3_grouped(torch.zeros(0, 8, 8, 64, dtype=torch.float16, device=DEV), w, torch.zeros(64, device=DEV),
                            16, 1, True)
    assert tuple(y.shape) == (0, 8, 8, 64)


def test_grouped_split_range_guard(ops):
    """An output past 65504 has no finite hi half: the kernel raises the
    runner's flag; the same conv with a small bias leaves it 0."""
    torch.manual_seed(5)
    x = P.to_split(torch.rand(2, 7, 7, 128, device=DEV) * 0.1)
    sw, scale = P.pack_grouped_split_weight(torch.randn(128, 4, 3, 3) * 0.01, 32)
    sw = sw.to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(bias):
        flag.zero_()
        ops.set_split_guard(flag)
        try:
            y = ops.conv3x3_grouped_split(x, sw, torch.full((128,), bias, device=DEV), scale, 32, 1, False)
        finally:
            ops.set_split_guard(None)
        torch.cuda.synchronize()
        return int(flag.item()), y

    f, y = run(60000.0)
    assert f == 0 and bool(torch.isfinite(P.from_split(y)).all())
    f, _ = run(70000.0)
    assert f == 1
    f, _ = run(100.0)                          # the flag was reset: clean again
    assert f == 0


def test_grouped_binding_checks_name_the_operand(ops):
    """Malformed operands are refused before anything launches, and the message
    names the operand."""
    def args(c=64, groups=16, cb=16):
        return dict(x=torch.zeros(1, 4, 4, c, dtype=torch.float16, device=DEV),
                    w=torch.zeros(c, 9 * cb, dtype=torch.float16, device=DEV), bias=torch.zeros(c, device=DEV),
                    groups=groups, stride=1, relu=True)

    def split_args(c=64, groups=16, cb=16):
        a = args(c, groups, cb)
        a["x"] = torch.zeros(1, 4, 4, 2 * c, dtype=torch.float16, device=DEV)
        a["w"] = torch.zeros(c, 18 * cb, dtype=torch.float16, device=DEV)
        return dict(a, acc_scale=1.0)

    for fn, mk in ((ops.conv3x3_grouped, args), (ops.conv3x3_grouped_split, split_args)):
        fn(**mk())                                                            # the valid call is accepted
        bad = [
            (r"\bx has wrong dtype", dict(mk(), x=mk()["x"].float())),
            (r"\bw has wrong dtype", dict(mk(), w=mk()["w"].float())),
            (r"\bbias has wrong dtype", dict(mk(), bias=mk()["bias"].half())),
            (r"\bx must be a GPU tensor", dict(mk(), x=mk()["x"].cpu())),
            (r"\bx must have rank 4", dict(mk(), x=mk()["x"][0])),
            (r"\bx must be contiguous", dict(mk(), x=torch.stack([mk()["x"]] * 2, -1)[..., 0])),
            (r"\bw must be contiguous", dict(mk(), w=torch.stack([mk()["w"]] * 2, -1)[..., 0])),
            (r"groups: 24 .* divide x's C = 64", dict(mk(), groups=24)),       # C % groups != 0
            (r"groups: C / groups = 12 ", dict(mk(96, 8, 16))),                # Cg 12
            (r"groups: 1 must be > 1", dict(mk(), groups=1)),
            (r"stride must be 1 or 2, got 3", dict(mk(), stride=3)),
            (r"\bw: must be \[", dict(mk(), w=torch.zeros(64, 9 * 64, dtype=torch.float16, device=DEV))),
            (r"\bw: must be \[", dict(mk(), w=mk(128)["w"])),
            (r"\bbias: must have C = 64", dict(mk(), bias=torch.zeros(32, device=DEV))),
            (r"\bx: .*C % 32 == 0", dict(mk(), x=mk()["x"][..., :48].contiguous())),
        ]
        for pattern, kw in bad:
            with pytest.raises(RuntimeError, match=pattern):
                fn(**kw)


def _one_conv_runner(w, b, groups, stride, relu, dtype):
    """A runner whose program is just enough to route one grouped conv."""
    conv = nn.Conv2d(w.shape[0], w.shape[0], 3, stride, 1, groups=groups, bias=True)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    c = P.make_conv(conv, None, relu, dtype)
    r = HipRunner(P.Program("one-grouped-conv", "resnet", dtype=dtype))
    return r, c.to(DEV)


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[4]], ids=lambda c: "x".join(map(str, c)))
def test_grouped_kernel_vs_dense_arm(ops, case):
    """The runner's ``grouped_dense`` arm -- the dense conv on the block-diagonal
    expansion, existing direct kernels -- against the grouped kernel: the same
    products (plus exact zeros), so only the summation order differs (split
    2e-6 of the scale, the bound tests/test_split.py uses for that; fp16 1e-2)."""
    B, H, W, C, groups, stride = case
    x, w, b, _ = _case(case)
    want = _want(case, True)
    r, c = _one_conv_runner(w, b, groups, stride, True, "fp32")
    xs = ops.split_from_f32(x.to(DEV))
    got = ops.f32_from_split(r._conv_split(c, xs)).cpu()
    r.grouped_dense = True
    dense = ops.f32_from_split(r._conv_split(c, xs)).cpu()
    assert len(r._gdense) == 1
    r._conv_split(c, xs)
    assert len(r._gdense) == 1                          # built once, cached on the runner
    _check_split(dense, want)
    _check_split(got, dense.double(), rel=2e-6)
    # the all-f32-MFMA path has no grouped kernel: always the dense fp32 expansion
    r.grouped_dense = False
    f32 = r._conv(c, x.to(DEV)).cpu()
    _check_split(f32, want)

    r, c = _one_conv_runner(w, b, groups, stride, True, "fp16")
    x16 = x.to(DEV).half()
    got = r._conv(c, x16).cpu()
    assert not r._gdense
    r.grouped_dense = True
    dense = r._conv(c, x16).cpu()
    assert len(r._gdense) == 1
    _check_f16(dense, want)
    scale = want.abs().max().item()
    assert (got.double() - dense.double()).abs().max().item() <= 1e-2 * scale


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fp32_model(name):
    """(module, fp32 program, images [2] on the CPU, fp64 logits), seed-0 weights."""
    from idunno.runtime.data import synth_images_cpu

    m = ref.build(name, seed=0)
    prog = P.compile_model(m, name, "fp32")
    img = torch.from_numpy(synth_images_cpu(0, 0, 2))
    with torch.no_grad():
        want = copy.deepcopy(m).double()(ref.preprocess_u8(img).double())
    return m, prog, img, want


def _rel_err(got, want):
    return (got.double().cpu() - want).abs().max().item() / want.abs().max().item()


def _confident(want, rel=1e-4):
    """Images whose fp64 top-1 / top-2 margin exceeds ``rel`` of the logit scale."""
    top2 = want.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > rel * want.abs().max()


@pytest.mark.parametrize("name", ["resnext50_32x4d", "wide_resnet50_2"])
def test_fp32_program_on_split_kernels_matches_fp64(ops, name):
    m, prog, img, want = _fp32_model(name)
    r = HipRunner(prog)
    assert r.split and r._split_ok()
    got = r.logits(img.to(DEV))
    err = _rel_err(got, want)
    print(f"{name} split: rel logit err {err:.2e}")
    assert r.overflow_reruns == 0
    assert err <= 1e-5, f"{name}: rel logit err {err:.2e}"
    sure = _confident(want)
    assert int(sure.sum()) >= 1
    assert torch.equal(got.cpu().argmax(1)[sure], want.argmax(1)[sure])
    if name == "resnext50_32x4d":
        assert not r._gdense                              # no dense expansion on the default path


@pytest.mark.parametrize("name", ["resnext50_32x4d", "wide_resnet50_2"])
def test_fp32_program_on_f32_mfma_kernels_matches_fp64(ops, name):
    """``split = False``: the all-f32-MFMA path; a grouped conv takes the dense fp32 expansion."""
    m, prog, img, want = _fp32_model(name)
    r = HipRunner(prog)
    r.split = False
    err = _rel_err(r.logits(img.to(DEV)), want)
    print(f"{name} f32 MFMA: rel logit err {err:.2e}")
    assert err <= 2e-5, f"{name}: rel logit err {err:.2e}"
    assert len(r._gdense) == (16 if name == "resnext50_32x4d" else 0)


def test_resnext_range_guard_rerun_matches_fp64(ops):
    """Stem weights x 1e5 (as test_split_activations_past_fp16_range_match_fp64):
    the split forward trips the guard and is recomputed on the f32 kernels,
    grouped convs on their dense fp32 expansion."""
    from idunno.runtime.data import synth_images_cpu

    m = ref.build("resnext50_32x4d", seed=3)
    with torch.no_grad():
        m.conv1.weight *= 1e5
    r = HipRunner(P.compile_model(m, "resnext50_32x4d", "fp32"))
    assert r.split and r._split_ok()
    img = torch.from_numpy(synth_images_cpu(4, 0, 2))
    with torch.no_grad():
        x = ref.preprocess_u8(img).double()
        md = m.double()
        want = md(x)
        assert torch.relu(md.bn1(md.conv1(x))).abs().max().item() > 1e5      # the regime under test
    got = r.logits(img.to(DEV))
    assert r.overflow_reruns == 1
    err = _rel_err(got, want)
    print(f"guard rerun: rel logit err {err:.2e}")
    assert err <= 2e-5, f"rel logit err {err:.2e}"


@pytest.mark.parametrize("name,B,damp", [("resnext50_32x4d", 4, 1.0), ("resnext101_32x8d", 1, 1.0),
                                         ("resnet101", 2, 0.25)])
def test_fp16_program_vs_fp32_torch_module(ops, name, B, damp):
    """As test_model_end_to_end_vs_fp32_oracle: logits within 3 % of their scale.
    resnext101_32x8d is the only whole-model run at 64 channels per group.

    ``damp`` scales the last BN gain of every block.  Under seed-7 random BN the
    residual stream of ResNet101's 33 dense blocks grows 1.66 x a block, to
    activations of 1.6e8 (fp32 torch module, CPU): fp16 activations end at 65504, so
    no fp16 program can carry that model whatever its kernels do.  At 0.25 the
    largest activation is 92 (4e3 at 0.5).  The ResNeXts stay below 30 undamped."""
    m = ref.build(name, seed=7, randomize_bn=True)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, ref.Bottleneck):
                mod.bn3.weight *= damp
    runner = HipRunner(P.compile_model(m, name))
    torch.manual_seed(8)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=DEV)
    logits = runner.logits(img)
    with torch.no_grad():
        want = m.to(DEV)(ref.preprocess_u8(img))
    scale = want.abs().max().item()
    err = (logits - want).abs().max().item()
    print(f"{name} fp16: logits err {err:.3e} vs scale {scale:.3e}")
    assert err < 0.03 * scale, f"{name}: logits err {err} vs scale {scale}"
    assert not runner._gdense


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_resnext_graph_replay_equals_eager(ops, dtype):
    m, prog32, _, _ = _fp32_model("resnext50_32x4d")
    r = HipRunner(prog32 if dtype == "fp32" else P.compile_model(m, "resnext50_32x4d", "fp16"))
    img = ops.synth_images(11, 0, 3, DEV)
    cls, prob = (t.clone() for t in r.forward(img))
    sin, replay = r.capture(3)
    sin.copy_(img)
    gcls, gprob = replay()
    torch.cuda.synchronize()
    assert torch.equal(gcls, cls) and torch.equal(gprob, prob)
    # the switch is part of every graph's key: the old graph is not replayed for the other arm
    assert r.has_graph(3)
    r.grouped_dense = True
    assert not r.has_graph(3)
    r.grouped_dense = False
    assert r.has_graph(3)
    r.close()


def test_hip_executor_agrees_with_torch_executor_on_resnext(ops):
    from idunno.runtime.data import synth_images_cpu
    from idunno.runtime.executor import TorchExecutor, make_executor

    name = "resnext50_32x4d"
    img = torch.from_numpy(synth_images_cpu(0, 0, 8))
    with torch.no_grad():
        want = ref.build(name, seed=0).double()(ref.preprocess_u8(img).double())
    sure = _confident(want).numpy()
    assert sure.sum() >= 1
    ex = make_executor("hip", seed=0)
    try:
        cls, prob = ex.run(name, img.to(DEV), 0, 7)
    finally:
        ex.close()
    tcls, tprob = TorchExecutor("cpu", seed=0).run(name, img, 0, 7)
    assert (cls[sure] == tcls[sure]).all() and (cls[sure] == want.argmax(1).numpy()[sure]).all()
    assert abs(prob[sure] - tprob[sure]).max() < 1e-4


def test_resnext_inference_query_through_a_two_node_cluster(ops):
    """One 8-image ``inference`` query for resnext50_32x4d through an in-process
    cluster with the HIP executor, as tests/test_cluster_gpu.py runs resnet18."""
    from idunno.runtime.cluster import LocalCluster
    from idunno.runtime.data import SyntheticSource, synth_images_cpu
    from idunno.runtime.executor import HipExecutor

    name = "resnext50_32x4d"
    fast = dict(heartbeat_period_s=0.05, failure_timeout_s=1.0, metadata_period_s=0.2, rpc_timeout_s=10.0)
    c = LocalCluster(num_nodes=2, executor_factory=lambda i: HipExecutor("cuda", seed=0),
                     source_factory=lambda i, node: SyntheticSource(node.cfg.data_seed, "cuda"), **fast).start()
    try:
        cl = c.client()
        cl.inference(0, 7, name)
        assert cl.wait_idle(120, {name: 8})["done"][name] == 8
        res = cl.view("c4")["results"]
    finally:
        c.stop()
    got = {}
    for k, chunks in res.items():
        if k.startswith(name + " "):
            for ch in chunks:
                for fname, cat, p in ast.literal_eval(ch):
                    got[int(fname[5:-5])] = (int(cat.split("_")[1]), p)
    assert sorted(got) == list(range(8))
    img = torch.from_numpy(synth_images_cpu(c.cfg.data_seed, 0, 8))
    with torch.no_grad():
        want = ref.build(name, seed=0).double()(ref.preprocess_u8(img).double())
    sure = _confident(want)
    assert int(sure.sum()) >= 1
    p64 = torch.softmax(want, 1)
    for i in range(8):
        if sure[i]:
            assert got[i][0] == int(want[i].argmax())
        assert abs(got[i][1] - p64[i, got[i][0]].item()) < 1e-4
