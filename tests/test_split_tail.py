"""The 1x1 downsample as a K tail of a basic block's second 3x3 conv
(ops.conv2d_split_tail, conv_glds.hip TAIL; HipRunner.fuse_down_tail):
conv3x3(y, W2) + conv1x1/s(x, Wd) as ONE split-fp16 GEMM over the
concatenated K, against the fp64 oracle in the style of test_split.py."""
import pytest
import torch
import torch.nn.functional as F

from idunno.models import HipRunner
from idunno.models import packed as P

DEV = "cuda"


# ---------------------------------------------------------------------------
# CPU: weight layout and arithmetic
# ---------------------------------------------------------------------------

def _grid_weights(cout, c, cx):
    """W2 / Wd on a grid the split format holds exactly at any exponent the
    pair can get (integers below 2^21 times 2^-24), Wd at 3x W2's scale."""
    g = torch.Generator().manual_seed(11)
    w2 = torch.randint(-2 ** 19, 2 ** 19, (cout, c, 3, 3), generator=g).double() * 2.0 ** -24
    wd = torch.randint(-3 * 2 ** 19, 3 * 2 ** 19, (cout, cx, 1, 1), generator=g).double() * 2.0 ** -24
    return w2.float(), wd.float()


def _unpack(sw, scale, cout, k, cin):
    v = sw.double().reshape(cout, k, k, cin // 32, 2, 32)
    return ((v[..., 0, :] + v[..., 1, :]).reshape(cout, k, k, cin) * scale).permute(0, 3, 1, 2)


def test_tail_weight_is_w2_then_wd_with_one_exponent_cpu():
    cout, c, cx = 32, 64, 32
    w2, wd = _grid_weights(cout, c, cx)
    sw, scale = P.pack_split_tail_weight(w2, wd)
    assert sw.dtype == torch.float16 and sw.shape == (cout, 9 * 2 * c + 2 * cx)
    # one exponent, from the max |w| over BOTH parts (here Wd's)
    e = P._split_scale(torch.cat([w2.flatten(), wd.flatten()]))
    assert scale == 2.0 ** -e and e == P._split_scale(wd) and e < P._split_scale(w2)
    assert 2 ** 13 <= float(sw.float().abs().max()) <= 2 ** 14
    # K order: the nine taps' blocks (pack_split_weight's order), then the tail's blocks
    assert torch.equal(sw[:, :9 * 2 * c], P.pack_split_weight(w2, e)[0])
    assert torch.equal(sw[:, 9 * 2 * c:], P.pack_split_weight(wd, e)[0])
    assert torch.equal(_unpack(sw[:, :9 * 2 * c], scale, cout, 3, c), w2.double())
    assert torch.equal(_unpack(sw[:, 9 * 2 * c:], scale, cout, 1, cx), wd.double())
    # a forced exponent only changes the scaling, not the layout
    own, own_scale = P.pack_split_weight(w2)
    assert own_scale == 2.0 ** -P._split_scale(w2)
    assert torch.equal(_unpack(own, own_scale, cout, 3, c), w2.double())


def _emu_products(x, sw, cout, cin, k, stride, pad):
    """hi*hi + hi*lo + lo*hi of one K part in fp64 (unscaled accumulator)."""
    xs = P.to_split(x).double().reshape(*x.shape[:-1], cin // 32, 2, 32)
    xh = xs[..., 0, :].reshape(x.shape).permute(0, 3, 1, 2)
    xl = xs[..., 1, :].reshape(x.shape).permute(0, 3, 1, 2)
    ws = sw.double().reshape(cout, k, k, cin // 32, 2, 32)
    wh = ws[..., 0, :].reshape(cout, k, k, cin).permute(0, 3, 1, 2)
    wl = ws[..., 1, :].reshape(cout, k, k, cin).permute(0, 3, 1, 2)
    return F.conv2d(xh, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad) + F.conv2d(xl, wh, None, stride, pad)


def test_tail_arithmetic_matches_fp32_accuracy_cpu():
    torch.manual_seed(2)
    c, cx, cout = 64, 32, 32
    y = F.relu(torch.randn(2, 6, 6, c))
    x = F.relu(torch.randn(2, 12, 12, cx))
    w2 = torch.randn(cout, c, 3, 3) / 24
    wd = torch.randn(cout, cx, 1, 1) / cx ** 0.5 * 3.0
    sw, scale = P.pack_split_tail_weight(w2, wd)
    acc = _emu_products(y, sw[:, :9 * 2 * c], cout, c, 3, 1, 1) + _emu_products(x, sw[:, 9 * 2 * c:], cout, cx, 1, 2, 0)
    got = acc * scale                                           # ONE accumulator, one scale
    ref = F.conv2d(y.double().permute(0, 3, 1, 2), w2.double(), None, 1, 1) + \
        F.conv2d(x.double().permute(0, 3, 1, 2), wd.double(), None, 2, 0)
    y32 = F.conv2d(y.permute(0, 3, 1, 2), w2, None, 1, 1) + F.conv2d(x.permute(0, 3, 1, 2), wd, None, 2, 0)
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    err32 = ((y32.double() - ref).abs().max() / ref.abs().max()).item()
    assert err < 4 * max(err32, 1e-7), (err, err32)


# ---------------------------------------------------------------------------
# GPU: the op against the fp64 oracle
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _check(y, ref, rel=2e-5):
    y = y.double()
    scale = ref.abs().max().item() + 1e-12
    err = (y - ref).abs().max().item()
    print(f"max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})")
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


def _ref64(y, x, w2, wd, b, stride2, relu):
    r = F.conv2d(y.double().permute(0, 3, 1, 2), w2.double().to(y.device), None, 1, 1) + \
        F.conv2d(x.double().permute(0, 3, 1, 2), wd.double().to(y.device), None, stride2, 0) + \
        b.double().to(y.device).view(1, -1, 1, 1)
    return (F.relu(r) if relu else r).permute(0, 2, 3, 1)


TAIL_CASES = [
    # (B, Ho, C = Cout, Cx, stride2, tile, H2)
    (2, 14, 256, 128, 2, 36, 28),     # layer-3-like
    (3, 7, 512, 256, 2, 42, 14),      # M = 147, not a tile multiple; a tile spans images
    (1, 9, 64, 32, 2, 36, 18),        # one tail stage; Cout masks part of a tile
    (2, 13, 128, 64, 2, -1, 25),      # default route; x2 of odd size 25 x 25
    (2, 9, 128, 64, 1, 36, 9),        # stride2 = 1
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Ho,C,Cx,s2,tile,H2", TAIL_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_conv_split_tail(ops, B, Ho, C, Cx, s2, tile, H2, relu):
    torch.manual_seed(B * 1000 + Ho + C + Cx)
    y = torch.randn(B, Ho, Ho, C, device=DEV)
    x = torch.randn(B, H2, H2, Cx, device=DEV)
    w2 = torch.randn(C, C, 3, 3) / (9 * C) ** 0.5
    wd = torch.randn(C, Cx, 1, 1) / Cx ** 0.5 * 3.0          # 3x the 3x3 conv's weight scale
    b = torch.randn(C) * 0.1
    sw, scale = P.pack_split_tail_weight(w2, wd)
    out = ops.conv2d_split_tail(ops.split_from_f32(y), ops.split_from_f32(x), sw.to(DEV), b.to(DEV), scale, s2, relu,
                                tile=tile)
    assert out.dtype == torch.float16 and out.shape == (B, Ho, Ho, 2 * C)
    _check(P.from_split(out), _ref64(y, x, w2, wd, b, s2, relu))


@pytest.mark.gpu
def test_conv_split_tail_reads_strided_views(ops):
    """y and x2 as channel slices of wider tensors (pixel strides ldx / ldx2)."""
    torch.manual_seed(9)
    B, Ho, C, Cx = 2, 7, 128, 64
    y = torch.randn(B, Ho, Ho, C, device=DEV)
    x = torch.randn(B, 14, 14, Cx, device=DEV)
    w2 = torch.randn(C, C, 3, 3) / (9 * C) ** 0.5
    wd = torch.randn(C, Cx, 1, 1) / Cx ** 0.5 * 3.0
    b = (torch.randn(C) * 0.1).to(DEV)
    sw, scale = P.pack_split_tail_weight(w2, wd)
    ys, xs = ops.split_from_f32(y), ops.split_from_f32(x)
    want = ops.conv2d_split_tail(ys, xs, sw.to(DEV), b, scale, 2, True)
    yw = torch.full((B, Ho, Ho, 2 * C + 64), 7.0, dtype=torch.float16, device=DEV)
    xw = torch.full((B, 14, 14, 4 * Cx), 7.0, dtype=torch.float16, device=DEV)
    yw[..., 64:] = ys
    xw[..., 2 * Cx:] = xs
    got = ops.conv2d_split_tail(yw[..., 64:], xw[..., 2 * Cx:], sw.to(DEV), b, scale, 2, True)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_conv_split_tail_rejects_bad_operands(ops):
    y = torch.zeros(1, 7, 7, 256, dtype=torch.float16, device=DEV)
    x = torch.zeros(1, 14, 14, 128, dtype=torch.float16, device=DEV)
    w = torch.zeros(128, 9 * 256 + 128, dtype=torch.float16, device=DEV)
    b = torch.zeros(128, device=DEV)
    ops.conv2d_split_tail(y, x, w, b, 1.0, 2, True)
    with pytest.raises(RuntimeError):                       # x2 does not give y's grid at this stride
        ops.conv2d_split_tail(y, x, w, b, 1.0, 1, True)
    with pytest.raises(RuntimeError):                       # weight row without the tail's K
        ops.conv2d_split_tail(y, x, w[:, :9 * 256].contiguous(), b, 1.0, 2, True)
    with pytest.raises(RuntimeError):                       # a tile without a K-tail form
        ops.conv2d_split_tail(y, x, w, b, 1.0, 2, True, tile=27)


@pytest.mark.gpu
def test_tail_default_rule(ops):
    """The library's rule: ResNet18's three stride-2 blocks at the headline batch, not
    where the unfused conv takes split-K (layers 3 / 4 of a 50-image chunk)."""
    ok = ops.conv2d_split_tail_ok
    assert ok(400, 28, 28, 128, 64, 128) and ok(400, 14, 14, 256, 128, 256) and ok(400, 7, 7, 512, 256, 512)
    assert ok(50, 28, 28, 128, 64, 128)
    assert not ok(50, 14, 14, 256, 128, 256) and not ok(50, 7, 7, 512, 256, 512)
    assert not ok(4, 14, 14, 256, 128, 256)
    assert not ok(400, 14, 14, 256, 128, 192)               # Cout % 128 != 0: no default tile
    # mode 2: every supported shape; 3: the rule, but not over the band kernel (W 28, a tile per CU)
    assert ok(4, 7, 7, 512, 256, 512, mode=2) and not ok(4, 7, 7, 512, 256, 192, mode=2)
    assert not ok(400, 28, 28, 128, 64, 128, mode=3) and ok(400, 14, 14, 256, 128, 256, mode=3)
    assert ok(50, 28, 28, 128, 64, 128, mode=3)             # below a band tile per CU: im2col either way
    assert not ok(400, 14, 14, 256, 128, 256, mode=0)


@pytest.mark.gpu
def test_split_guard_flags_tail_sum_past_fp16_range(ops):
    """conv3x3 + bias and the tail each fit fp16's range, their sum does not: the
    epilogue sees only the sum and must flag it."""
    torch.manual_seed(5)
    C, Cx = 128, 64
    y = P.to_split(torch.rand(2, 7, 7, C, device=DEV) * 0.1)
    x = P.to_split(torch.ones(2, 14, 14, Cx, device=DEV))
    w2 = torch.randn(C, C, 3, 3) * 0.01
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(bias, down):
        wd = torch.full((C, Cx, 1, 1), down / Cx)           # the tail alone sums to `down` at every output
        sw, scale = P.pack_split_tail_weight(w2, wd)
        flag.zero_()
        ops.set_split_guard(flag)
        try:
            out = ops.conv2d_split_tail(y, x, sw.to(DEV), torch.full((C,), bias, device=DEV), scale, 2, False)
        finally:
            ops.set_split_guard(None)
        torch.cuda.synchronize()
        return int(flag.item()), out

    f, out = run(20000.0, 40000.0)              # every part and the sum < 65504
    assert f == 0 and bool(torch.isfinite(P.from_split(out)).all())
    f, _ = run(10000.0, 60000.0)                # each part fits, the sum does not
    assert f == 1
    f, _ = run(10000.0, 40000.0)                # the flag was reset: clean again
    assert f == 0


# ---------------------------------------------------------------------------
# GPU: the whole ResNet18 forward
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet18(ops):
    from idunno.models import reference as ref

    m = ref.build("resnet18", seed=2, randomize_bn=True)
    prog = P.compile_model(m, "resnet18", "fp32")
    img = ops.synth_images(7, 0, 4, DEV)
    with torch.no_grad():
        want = m.double()(ref.preprocess_u8(img.cpu()).double())
    return prog, img, want


def _stem_out(r, img):
    s = r.p.stem
    return r.ops.stem_split(img, s.fs, s.fs_bias, s.fs_psum, s.fs_scale)


@pytest.mark.gpu
def test_resnet18_tail_fusion_same_logits_and_oracle(ops, resnet18):
    prog, img, want = resnet18
    r = HipRunner(prog)
    assert r.split and r._split_ok()
    r.fuse_down_tail = 0
    plain = r.logits(img).double()
    scale = plain.abs().max().item()
    # B = 4 is a split-K batch, where the default rule keeps the unfused path: force
    # the fusion on all three stride-2 blocks (mode 2)
    r.fuse_down_tail = 2
    x = _stem_out(r, img)
    seen = 0
    for blk in r.p.blocks:
        if blk.down is not None:
            assert r._tail_ok(blk, x)
            seen += 1
        x = r._block_split(blk, x)
    assert seen == 3
    fused = r.logits(img).double()
    d = (fused - plain).abs().max().item()
    err = (fused.cpu() - want).abs().max().item() / want.abs().max().item()
    print(f"on vs off {d / scale:.2e} of the logit scale; on vs fp64 {err:.2e}")
    assert d <= 1e-6 * scale
    assert err <= 2e-5
    assert torch.equal(fused.cpu().argmax(1), want.argmax(1))
    # the default rule (whatever it picks at this batch) agrees as well
    r.fuse_down_tail = 1
    assert (r.logits(img).double() - plain).abs().max().item() <= 1e-6 * scale


@pytest.mark.gpu
def test_resnet18_tail_fusion_graph_replay_is_eager_bitwise(ops, resnet18):
    prog, img, _ = resnet18
    r = HipRunner(prog)
    r.fuse_down_tail = 2
    c0, p0 = r.forward(img)
    _start, run = r.capture_window(img, 4)
    c1, p1 = run()
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and torch.equal(p0, p1)
    # off is another graph (the attribute is part of the capture key)
    r.fuse_down_tail = 0
    assert not r.has_graph(4)
    k_off = r._capture_key(4)
    r.fuse_down_tail = 2
    assert r._capture_key(4) != k_off


def _other(v):
    """A value of the switch's own kind that differs from ``v`` (also after int())."""
    if isinstance(v, bool):
        return not v
    return 2 if v is None else v + 1


@pytest.mark.gpu
def test_every_declared_graph_switch_is_in_the_capture_key(ops, resnet18):
    r = HipRunner(resnet18[0])
    assert "astem_form" in r.GRAPH_SWITCHES and "fuse_down_tail" in r.GRAPH_SWITCHES
    # a public attribute the constructor sets is a declared switch unless it is named here:
    # a switch added later cannot stay out of the key unnoticed
    not_switches = {"ops", "device", "p", "graph_pool", "overflow_fallback", "overflow_reruns", "direct_launch"}
    public = {k for k in vars(r) if not k.startswith("_")}
    assert public - not_switches == set(r.GRAPH_SWITCHES)
    k0 = r._capture_key(4)
    for name in r.GRAPH_SWITCHES:
        was = getattr(r, name)
        setattr(r, name, _other(was))
        assert r._capture_key(4) != k0, name
        setattr(r, name, was)
        assert r._capture_key(4) == k0, name


@pytest.mark.gpu
def test_astem_form_is_in_the_capture_key(ops):
    r = HipRunner(P.build_program("alexnet", seed=0))
    k0 = r._capture_key(4)
    r.astem_form = 0
    assert r._capture_key(4) != k0
