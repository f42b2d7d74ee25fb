"""Plain float64 references of the memory-bound kernels (resize_crop, the pools,
softmax_top1), written from the operations' definitions, and the cases the
CPU and GPU tests share (no fixture files)."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
GREY = 1.0 / 255 / 0.229            # one grey level after normalisation (red: the smallest std)

# (B, Hi, Wi, resize, crop, err32).  err32 = max |resize_crop_ref(float32) - resize_crop_ref(float64)|,
# measured on the CPU with the seeded images of ``resize_case_image``, over both
# fp32 orders of the source coordinate ((o + 0.5) * n_in / n_out and
# (o + 0.5) * (n_in / n_out)): 1.46e-5 is the largest of the five small cases
# (61x64), 9.6e-5 the 375x500 case, whose coordinates are ten times larger.
# test_elementwise_cpu.py asserts the figures; the GPU test allows RESIZE_MARGIN
# times them for the kernel's own fp32 coordinate and blend rounding.
ERR32_SMALL, ERR32_LARGE = 1.5e-5, 1.0e-4
RESIZE_CASES = [
    (2, 30, 40, 32, 29, ERR32_SMALL),        # left 6, half-up would give 7
    (2, 40, 30, 32, 29, ERR32_SMALL),        # the portrait twin, top 6
    (1, 20, 20, 32, 28, ERR32_SMALL),        # upscale, square
    (3, 33, 47, 24, 16, ERR32_SMALL),
    (1, 61, 64, 48, 40, ERR32_SMALL),
    (1, 375, 500, 256, 224, ERR32_LARGE),    # the ImageNet 4:3 case, left 58
]
RESIZE_MARGIN = 4


def noise_u8(shape, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def resize_case_image(i: int) -> np.ndarray:
    B, Hi, Wi = RESIZE_CASES[i][:3]
    return noise_u8((B, Hi, Wi, 3), 700 + i)


def center_crop_geometry(hi: int, wi: int, resize: int, crop: int):
    """(Hr, Wr, top, left) of torchvision's Resize(resize) + CenterCrop(crop)."""
    if hi <= wi:
        hr, wr = resize, int(resize * wi / hi)
    else:
        hr, wr = int(resize * hi / wi), resize
    return hr, wr, int(round((hr - crop) / 2.0)), int(round((wr - crop) / 2.0))


def _taps(n_in: int, n_out: int, first: int, count: int, dtype, scale_first: bool = False):
    """Bilinear taps (half-pixel centres, no antialias) of outputs first .. first + count - 1."""
    o = np.arange(first, first + count).astype(dtype)
    if scale_first:             # the same coordinate, the other order of the two roundings
        src = (o + dtype(0.5)) * (dtype(n_in) / dtype(n_out)) - dtype(0.5)
    else:
        src = (o + dtype(0.5)) * dtype(n_in) / dtype(n_out) - dtype(0.5)
    src = np.maximum(src, dtype(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(dtype)).astype(dtype)


def resize_crop_ref(img_u8: np.ndarray, resize: int, crop: int, dtype=np.float64, top=None, left=None,
                    scale_first: bool = False) -> np.ndarray:
    """uint8 [..., Hi, Wi, 3] -> normalised [..., crop, crop, 3] in ``dtype``
    (float32: an emulation of fp32 arithmetic, to size tolerances only;
    ``scale_first`` picks the other order of the coordinate's roundings).
    ``top`` / ``left`` override the centre crop's offsets."""
    dtype = np.dtype(dtype).type
    hi, wi = img_u8.shape[-3:-1]
    hr, wr, t, l = center_crop_geometry(hi, wi, resize, crop)
    t, l = (t if top is None else top), (l if left is None else left)
    assert 0 <= t and t + crop <= hr and 0 <= l and l + crop <= wr
    a = img_u8.astype(dtype)
    y0, y1, wy = _taps(hi, hr, t, crop, dtype, scale_first)
    x0, x1, wx = _taps(wi, wr, l, crop, dtype, scale_first)
    wy, wx = wy[:, None, None], wx[:, None]
    rows = a[..., y0, :, :] * (dtype(1) - wy) + a[..., y1, :, :] * wy          # [..., crop, Wi, 3]
    v = rows[..., x0, :] * (dtype(1) - wx) + rows[..., x1, :] * wx             # [..., crop, crop, 3]
    out = (v / dtype(255) - np.asarray(MEAN, dtype)) / np.asarray(STD, dtype)
    assert out.dtype == dtype
    return out


def half_ulp_f16(ref) -> torch.Tensor:
    """Half an fp16 ulp at each (float64) reference value: the rounding of an
    exact result to fp16 (normal range 2^-14 .. 65504, subnormals below)."""
    r = torch.as_tensor(ref, dtype=torch.float64).abs()
    e = torch.floor(torch.log2(r.clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 11)


def maxpool_ref(x_nhwc: torch.Tensor, k: int, s: int, pad: int) -> torch.Tensor:
    """NHWC max pool in float64 (padding never wins)."""
    y = F.max_pool2d(x_nhwc.double().cpu().permute(0, 3, 1, 2), k, s, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def avgpool_ref(x_nhwc: torch.Tensor) -> torch.Tensor:
    return x_nhwc.double().cpu().mean((1, 2))


def softmax_top1_ref(logits: torch.Tensor):
    """(class int64 [rows], probability float64 [rows]); ties -> the lowest index."""
    p = torch.softmax(logits.double().cpu(), 1)
    v = p.max(1).values
    n = p.shape[1]
    first = torch.where(p == v[:, None], torch.arange(n), torch.tensor(n)).min(1).values
    return first, v
