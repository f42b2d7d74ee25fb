"""ops.resize_crop_u8 (kernels/resize_u8.hip) and the runner paths it opens.

The kernel carries Pillow's own 8-bit fixed-point tables, so against Pillow's
``Image.resize(..., BILINEAR)`` + crop it has no rounding freedom: ``torch.equal``.
``runtime.jpeg.reference_resize_crop`` states the same filter in float64 with exact
weights; Pillow's weights are rounded to 22 bits, so the two differ by one level where
the exact value lies within ~3e-4 of a half (measured on the host: 9 of 150528 bytes at
375x500, Pillow's bytes equal to the kernel's tables in all cases).  Against that
model the bound is the one tests/test_jpeg_gpu.py holds this stage to: max <= 1."""
import numpy as np
import pytest
import torch

from idunno import ops as _ops
from idunno.models import HipRunner
from idunno.models import packed as P
from idunno.runtime import jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, Hi, Wi, resize, crop); the last one's vertical support does not fit the LDS strip (chunked form)
CASES = [(2, 375, 500, 256, 224), (2, 500, 375, 256, 224), (1, 224, 224, 256, 224), (1, 256, 256, 256, 256),
         (1, 225, 300, 256, 224), (3, 30, 40, 32, 29), (1, 17, 1031, 16, 16), (1, 1031, 17, 16, 16),
         (1, 7680, 7680, 256, 256)]
BOARDS = [(2, 375, 500, 256, 224), (3, 30, 40, 32, 29)]


def _pillow(img: np.ndarray, resize: int, crop: int) -> np.ndarray:
    from PIL import Image

    hr, wr, top, left = _ops.resize_crop_geometry(img.shape[0], img.shape[1], resize, crop)
    im = Image.fromarray(img).resize((wr, hr), Image.BILINEAR)
    return np.asarray(im.crop((left, top, left + crop, top + crop)), dtype=np.uint8)


def _input(case, board: bool) -> torch.Tensor:
    B, Hi, Wi = case[:3]
    if board:
        yx = torch.arange(Hi)[:, None] + torch.arange(Wi)[None, :]
        return ((yx % 2) * 255).to(torch.uint8)[None, :, :, None].expand(B, Hi, Wi, 3).contiguous().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(Hi * 100003 + Wi)
    return torch.randint(0, 256, (B, Hi, Wi, 3), dtype=torch.uint8, device=DEV, generator=g)


@pytest.mark.parametrize("case,board", [(c, False) for c in CASES] + [(c, True) for c in BOARDS])
def test_kernel_matches_pillow(case, board):
    B, Hi, Wi, resize, crop = case
    img = _input(case, board)
    got = _ops.resize_crop_u8(img, resize, crop)
    assert got.shape == (B, crop, crop, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    host, small = img.cpu().numpy(), Hi * Wi <= 1 << 20
    try:
        import PIL  # noqa: F401
    except ImportError:
        if not small:
            pytest.skip("the float64 model of a 7680 x 7680 image is too large; Pillow is the reference")
    else:
        want = torch.from_numpy(np.stack([_pillow(h, resize, crop) for h in host]))
        ndiff = int((got.cpu() != want).sum())
        print(f"resize_crop_u8 {case}{' board' if board else ''}: {ndiff} bytes differ from Pillow")
        assert torch.equal(got.cpu(), want)
    if small:
        model = np.stack([jpeg.reference_resize_crop(h, resize, crop) for h in host]).astype(np.int16)
        d = np.abs(got.cpu().numpy().astype(np.int16) - model)
        print(f"resize_crop_u8 {case}: vs the float64 model max {d.max()}, {int((d != 0).sum())} bytes differ")
        assert d.max() <= 1
    if (Hi, Wi, resize) == (256, 256, 256):
        assert torch.equal(got, img)                       # the identity


def test_out_slice_leaves_neighbours_untouched():
    case = (1, 30, 40, 32, 29)
    img = _input(case, False)
    big = torch.full((3, 29, 29, 3), 7, dtype=torch.uint8, device=DEV)
    ret = _ops.resize_crop_u8(img, 32, 29, out=big[1:2])
    assert ret.data_ptr() == big[1:2].data_ptr()
    assert torch.equal(big[1:2], _ops.resize_crop_u8(img, 32, 29))
    assert bool((big[0] == 7).all()) and bool((big[2] == 7).all())


@pytest.mark.parametrize("bad", ["dtype", "channels", "cpu", "crop_gt_resize", "crop_gt_256", "strided"])
def test_binding_refusals(bad):
    img = torch.zeros(1, 40, 48, 4 if bad == "channels" else 3, dtype=torch.uint8, device=DEV)
    resize, crop = {"crop_gt_resize": (16, 20), "crop_gt_256": (300, 257)}.get(bad, (32, 29))
    if bad == "dtype":
        img = img.to(torch.int8)
    elif bad == "cpu":
        img = img.cpu()
    elif bad == "strided":
        img = img[:, :, ::2]
    with pytest.raises(RuntimeError):
        _ops.resize_crop_u8(img, resize, crop)


@pytest.fixture(scope="module")
def batch():
    return _input((3, 300, 400), False)


_PROGRAMS: dict = {}


def _runner(name, dtype):
    if (name, dtype) not in _PROGRAMS:
        _PROGRAMS[name, dtype] = P.build_program(name, seed=0, randomize_bn=True, dtype=dtype)
    return HipRunner(_PROGRAMS[name, dtype], DEV)


@pytest.mark.parametrize("name", ["resnet18", "alexnet"])
@pytest.mark.parametrize("split", [True, False])
def test_fp32_runner_takes_any_size(batch, name, split):
    r = _runner(name, "fp32")
    r.split = split
    got = r.logits(batch)
    assert got.shape == (3, 1000) and bool(torch.isfinite(got).all())
    assert torch.equal(got, r.logits(_ops.resize_crop_u8(batch, 256, 224)))
    cls, _ = r.forward(batch)
    assert torch.equal(cls.long(), got.argmax(1))
    with pytest.raises(ValueError, match="device-side windows"):
        r.logits(batch, torch.zeros(1, dtype=torch.int64, device=DEV), 2)


def test_fp16_runner_resize_u8_switch(batch):
    r = _runner("resnet18", "fp16")
    o, s = r.ops, r.p.stem
    x = o.maxpool2d(o.conv2d(o.resize_crop(batch, 256, 224), s.w, s.b, s.kh, s.kw, s.stride, s.pad, s.relu), 3, 2, 1)
    x = o.global_avgpool(r._blocks(r.p.blocks, x))
    for i, fc in enumerate(r.p.fcs):
        x = o.linear(x, fc.w, fc.b, relu=fc.relu, out_f32=i == len(r.p.fcs) - 1)
    assert not r.resize_u8
    assert torch.equal(r.logits(batch), x)                 # the default: as before the switch existed
    r.resize_u8 = True
    assert torch.equal(r.logits(batch), r.logits(_ops.resize_crop_u8(batch, 256, 224)))
