"""The memory-bound kernels' host side, without a GPU: resize_crop's geometry
against the JPEG path's, and the float64 reference of tests/elementwise_ref.py
against torch's own bilinear interpolation (so the GPU tests compare the
kernels with something that is itself checked)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from elementwise_ref import (GREY, MEAN, RESIZE_CASES, RESIZE_MARGIN, STD, center_crop_geometry, half_ulp_f16,
                             noise_u8, resize_case_image, resize_crop_ref, softmax_top1_ref)

from idunno import ops
from idunno.runtime import jpeg


def _sizes():
    out = {(h, w) for h in range(1, 601) for w in (1, 7, 224, 256, 333, 500, 600)}
    for a in range(200, 521):
        for b in (256, 300, 333, 375, 500):
            out.add((a, b))
            out.add((b, a))
    return sorted(out)


@pytest.mark.parametrize("resize,crop", [(256, 224), (32, 29), (24, 16)])
def test_resize_crop_geometry_is_the_jpeg_paths(resize, crop):
    """The binding's (Hr, Wr, top, left), the one definition resize_crop launches
    with, equals jpeg.resize_geometry (= load_image_u8 = torchvision CenterCrop:
    offsets rounded half to even) wherever the crop fits the resized image."""
    sizes = _sizes()
    skipped, odd_even = 0, 0
    for hi, wi in sizes:
        nw, nh, left, top = jpeg.resize_geometry(wi, hi, resize, crop)
        if nw < crop or nh < crop:
            skipped += 1
            continue
        assert ops.resize_crop_geometry(hi, wi, resize, crop) == (nh, nw, top, left), (hi, wi)
        assert center_crop_geometry(hi, wi, resize, crop) == (nh, nw, top, left), (hi, wi)
        d = max(nw, nh) - crop
        odd_even += d % 2 == 1 and (d // 2) % 2 == 0       # where rounding half up differs
    print(f"resize {resize} crop {crop}: {len(sizes)} sizes, {skipped} skipped, {odd_even} where half-up differs")
    assert skipped <= 0.05 * len(sizes)
    if (resize, crop) == (256, 224):
        assert skipped == 0
    assert odd_even > 100


def test_resize_crop_geometry_of_the_4_3_image():
    assert ops.resize_crop_geometry(375, 500) == (256, 341, 16, 58)
    assert ops.resize_crop_geometry(500, 375) == (341, 256, 58, 16)
    assert ops.resize_crop_geometry(300, 400, 256, 224) == (256, 341, 16, 58)
    assert ops.resize_crop_geometry(30, 40, 32, 29) == (32, 42, 2, 6)
    assert ops.resize_crop_geometry(224, 224, 256, 224) == (256, 256, 16, 16)


def _interpolate_ref(img, size, top, left, crop):
    f = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    r = F.interpolate(f, size=size, mode="bilinear", align_corners=False)[0]
    r = r[:, top:top + crop, left:left + crop].permute(1, 2, 0)
    return ((r / 255 - torch.tensor(MEAN, dtype=torch.float64)) / torch.tensor(STD, dtype=torch.float64)).numpy()


def test_resize_crop_ref_is_torch_bilinear_cropped_half_even():
    img = noise_u8((375, 500, 3), 11)
    got = resize_crop_ref(img, 256, 224)
    assert got.shape == (224, 224, 3) and got.dtype == np.float64
    assert np.abs(got - _interpolate_ref(img, (256, 341), 16, 58, 224)).max() <= 1e-9
    # the half-up offset is a different picture: a test against this reference tells the two apart
    assert np.abs(got - _interpolate_ref(img, (256, 341), 16, 59, 224)).max() > 0.1
    assert np.abs(resize_crop_ref(img, 256, 224, left=59) - _interpolate_ref(img, (256, 341), 16, 59, 224)).max() <= 1e-9
    # portrait and upscale
    p = noise_u8((40, 30, 3), 12)
    assert np.abs(resize_crop_ref(p, 32, 29) - _interpolate_ref(p, (42, 32), 6, 2, 29)).max() <= 1e-9
    u = noise_u8((20, 20, 3), 13)
    assert np.abs(resize_crop_ref(u, 32, 28) - _interpolate_ref(u, (32, 32), 2, 2, 28)).max() <= 1e-9


def test_resize_crop_fp32_slack_is_as_recorded():
    """The fp32 emulation's distance from the float64 reference, in either order
    of the coordinate's roundings, stays within the figures RESIZE_CASES records
    (the GPU test's slack is RESIZE_MARGIN x that), the records are measurements
    and no loose caps, and the GPU test's whole tolerance stays below a tenth of
    a grey level (if it did not, the reference would be wrong)."""
    worst = {}
    for i, (B, Hi, Wi, resize, crop, err32) in enumerate(RESIZE_CASES):
        img = resize_case_image(i)
        assert img.shape == (B, Hi, Wi, 3)
        r64 = resize_crop_ref(img, resize, crop)
        assert r64.shape == (B, crop, crop, 3)
        err = 0.0
        for scale_first in (False, True):
            r32 = resize_crop_ref(img, resize, crop, dtype=np.float32, scale_first=scale_first)
            assert r32.dtype == np.float32
            err = max(err, float(np.abs(r32.astype(np.float64) - r64).max()))
        print(f"case {(B, Hi, Wi, resize, crop)}: fp32 emulation max err {err:.3e} (recorded {err32:.1e})")
        assert err <= err32
        worst[err32] = max(worst.get(err32, 0.0), err)
        tol = half_ulp_f16(r64).max().item() + RESIZE_MARGIN * err32
        assert tol < 0.1 * GREY, tol
    for err32, err in worst.items():
        assert err >= 0.9 * err32, (err32, err)


def test_half_ulp_f16_is_the_rounding_error_bound():
    torch.manual_seed(0)
    x = torch.cat([torch.rand(20000, dtype=torch.float64) * 6 - 3, torch.rand(2000, dtype=torch.float64) * 1e-4,
                   torch.tensor([2.0, 1.0, 0.5, 65504.0, 2.0 ** -14, 2.0 ** -24, 0.0], dtype=torch.float64)])
    x = x.float().double()                                  # fp32 values: one rounding on the way to fp16
    err = (x.float().half().double() - x).abs()
    assert bool((err <= half_ulp_f16(x)).all())
    assert (err / half_ulp_f16(x)).max().item() > 0.99      # and not a loose one


def test_softmax_ref_ties_take_the_lowest_index():
    z = torch.tensor([[0.0, 5.0, 5.0, 1.0], [7.0, 7.0, 7.0, 7.0], [float("-inf"), 2.0, float("-inf"), 2.0]])
    i, v = softmax_top1_ref(z)
    assert i.tolist() == [1, 0, 1]
    assert torch.allclose(v, torch.tensor([1 / (2 + np.exp(-5.0) + np.exp(-4.0)), 0.25, 0.5], dtype=torch.float64),
                          rtol=1e-12)
