"""Normalised float batches on the HIP path: ops.float_to_nhwc4 / float_to_pack3 /
float_to_pack3_split (float_input.hip) and HipRunner's float route.

The operands are checked through their consumers (the stem convs the uint8
producers feed) against F.conv2d in float64, at the bounds the consumers' own
tests hold them to with a uint8 producer -- the float producer adds no
arithmetic.  37 x 45 is odd in both directions, no multiple of a 16-byte vector,
and five bands of 8 rows with a ragged last one; 224 x 224 is the models' size."""
import functools

import pytest
import torch
import torch.nn.functional as F

from idunno.models import HipRunner, compile_model
from idunno.models import packed as P
from idunno.models import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
FORMATS = ["nchw", "channels_last", "strided"]


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _images(B, H, W, dtype, fmt, seed=0):
    """Random normal x 3 [B,3,H,W] in the asked memory format; ``strided`` is the batch view
    base[1::2], whose rows start off the 16-byte grid at 37 x 45."""
    g = torch.Generator(device=DEV).manual_seed(seed + H)
    base = (torch.randn(2 * B + 1, 3, H, W, device=DEV, generator=g) * 3).to(dtype)
    if fmt == "strided":
        return base[1::2]
    x = base[:B].contiguous()
    return x.contiguous(memory_format=torch.channels_last) if fmt == "channels_last" else x


def _rel(y, want):
    return (y.double() - want).abs().max().item(), want.abs().max().item()


@pytest.mark.parametrize("B,H,W", [(3, 37, 45), (2, 224, 224)])
@pytest.mark.parametrize("k,s,p", [(7, 2, 3), (11, 4, 2)])
@pytest.mark.parametrize("form", ["nhwc4_f16", "nhwc4_f32", "pack3_f32", "pack3_f16", "pack3_split"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_operand_through_its_consumer(ops, dtype, fmt, form, k, s, p, B, H, W):
    x = _images(B, H, W, dtype, fmt)
    torch.manual_seed(k)
    w = torch.randn(64, 3, k, k) / (3 * k * k) ** 0.5
    b = torch.randn(64) * 0.1
    bd = b.to(DEV)
    if form == "nhwc4_f16":
        y = ops.conv2d(ops.float_to_nhwc4(x), P.pack_conv_weight(w)[0].to(DEV), bd, k, k, s, p, True)
    elif form == "nhwc4_f32":
        y = ops.conv2d(ops.float_to_nhwc4(x, f32=True), P.pack_conv_weight(w, "fp32")[0].to(DEV), bd, k, k, s, p, True)
    elif form == "pack3_split":
        sp3, scale = P.pack_split_weight_p3(w)
        y = ops.conv2d_pack3_split(ops.float_to_pack3_split(x, k, s, p), sp3.to(DEV), bd, scale, W, k, k, s, p, True)
    else:
        f16 = form == "pack3_f16"
        y = ops.conv2d_pack3(ops.float_to_pack3(x, k, s, p, f16=f16),
                             P.pack_conv_weight_p3(w, "fp16" if f16 else "fp32").to(DEV), bd, W, k, k, s, p, True)
    want = F.relu(F.conv2d(x.double(), w.double().to(DEV), b.double().to(DEV), s, p)).permute(0, 2, 3, 1)
    assert y.shape == want.shape
    err, scale = _rel(y, want)
    print(f"{form} {dtype} {fmt} {k}x{k} {H}x{W}: err {err:.3e}, scale {scale:.3e}")
    if form == "nhwc4_f16":          # test_kernels_gpu.py _check (test_conv_small_c_stem)
        assert err <= 1e-2 * (scale + 1e-6) + 1e-3
    elif form == "pack3_f16":        # test_pack3_f16_gpu.py test_conv_f16_pack3
        assert err <= 2e-3 * scale + 2e-3
    else:                            # test_kernels_f32_gpu.py / test_split.py _check: fp32 accuracy
        assert err <= 2e-5 * (scale + 1e-12)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_forms(ops, dtype, fmt):
    x = _images(3, 37, 45, dtype, fmt, seed=1)
    nhwc = x.permute(0, 2, 3, 1)
    y32 = ops.float_to_nhwc4(x, f32=True)
    assert y32.dtype == torch.float32 and y32.is_contiguous()
    assert torch.equal(y32[..., :3].view(torch.int32), nhwc.float().contiguous().view(torch.int32))
    y16 = ops.float_to_nhwc4(x)
    assert torch.equal(y16[..., :3].view(torch.int16), nhwc.half().contiguous().view(torch.int16))
    assert not y32[..., 3].any() and not y16[..., 3].any()
    # split packed rows (7x7/2 pad 3: four copies): the live positions of copy 0 are the row itself
    xs = ops.float_to_pack3_split(x, 7, 2, 3)
    nc = xs.shape[2] // 2
    hi, lo = (xs[:, :, c, 9:9 + 3 * 45].reshape(3, 37, 45, 3) for c in (0, nc))
    want_hi, want_lo = P._hi_lo(nhwc.float())                          # the contract, bit for bit
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    # ... and what it promises (exact_ref.py: hi and lo hold 11 bits and a sign each)
    back = hi.float() + lo.float()
    assert bool(((back - nhwc.float()).abs() <= nhwc.float().abs() * 2.0 ** -21 + 2.0 ** -24).all())
    assert not xs[:, :, 0, :9].any() and not xs[:, :, 0, 9 + 135:].any()     # the padding is zeros


@functools.lru_cache(maxsize=None)
def _model(name, dtype):
    """(module, program, uint8 images [4,224,224,3], float64 logits of the module on them)."""
    m = ref.build(name, seed=7, randomize_bn=True)
    u = torch.randint(0, 256, (4, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = m.double()(ref.preprocess_u8(u).double())
    m.float()
    return m, compile_model(m, name, dtype=dtype), u, want


@pytest.mark.parametrize("fmt,B,parts", [("nchw", 2, None), ("channels_last", 2, None), ("nchw", 4, 2)])
@pytest.mark.parametrize("name,dtype,split", [("resnet18", "fp32", True), ("resnet18", "fp32", False),
                                              ("resnet18", "fp16", True), ("alexnet", "fp32", True)])
def test_whole_model(ops, name, dtype, split, fmt, B, parts):
    _, prog, u, want = _model(name, dtype)
    r = HipRunner(prog)
    r.split, r.batch_parts = split, parts
    x = ref.preprocess_u8(u[:B]).to(DEV).contiguous()          # NCHW
    if dtype == "fp16":
        x = x.half()
    if fmt == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    err, scale = _rel(r.logits(x).cpu(), want[:B])
    print(f"{name} {dtype} split={split} {fmt} B={B}: rel logit err {err / scale:.2e}")
    # fp32: test_kernels_f32_gpu.py test_model_f32_vs_oracle; fp16: test_kernels_gpu.py end to end
    assert err <= (1e-4 if dtype == "fp32" else 0.03) * scale
    assert r.overflow_reruns == 0


def test_range_guard(ops):
    m, prog, u, _ = _model("resnet18", "fp32")
    x = ref.preprocess_u8(u[:2]).to(DEV)
    x[1, 2, 100, 17] = 7e4                      # no finite fp16 hi half
    r = HipRunner(prog)
    r.overflow_fallback = False
    cls, _ = r.forward(x)
    assert bool((cls == ops.OVERFLOW_CLASS).all()) and r.overflow_reruns == 0
    r.overflow_fallback = True
    got = r.logits(x)
    assert r.overflow_reruns == 1
    with torch.no_grad():
        want = m.double()(x.double().cpu())
    m.float()
    err, scale = _rel(got.cpu(), want)
    assert err <= 1e-4 * scale


def test_capture_float_beside_uint8(ops):
    _, prog, u, _ = _model("resnet18", "fp32")
    r = HipRunner(prog)
    u2 = u[:2].to(DEV)
    x = ref.preprocess_u8(u[2:4]).to(DEV)       # other images than the uint8 graph's
    sin8, replay8 = r.capture(2)
    sin8.copy_(u2)
    first8 = [t.clone() for t in replay8()]
    sinf, replayf = r.capture(2, in_dtype=torch.float32)
    assert sinf.shape == (2, 3, 224, 224) and sinf.dtype == torch.float32
    assert r.has_graph(2) and r.has_graph(2, in_dtype=torch.float32) and not r.has_graph(2, in_dtype=torch.float16)
    eager = r.forward(x)
    sinf.copy_(x)
    for _ in range(3):
        assert all(torch.equal(a, b) for a, b in zip(replayf(), eager))
    assert all(torch.equal(a, b) for a, b in zip(replay8(), first8))
    assert all(torch.equal(a, b) for a, b in zip(first8, r.forward(u2)))


@pytest.mark.parametrize("case", ["start", "256", "nhwc", "float64"])
def test_refusals(ops, case):
    r = HipRunner(_model("resnet18", "fp32")[1])
    shape = {"256": (2, 3, 256, 256), "nhwc": (2, 224, 224, 3)}.get(case, (2, 3, 224, 224))
    x = torch.zeros(shape, dtype=torch.float64 if case == "float64" else torch.float32, device=DEV)
    start = torch.zeros(1, dtype=torch.int64, device=DEV) if case == "start" else None
    with pytest.raises(ValueError):
        r.forward(x, start, 1 if case == "start" else -1)
