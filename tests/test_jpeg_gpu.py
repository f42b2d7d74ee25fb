"""JPEG decode on the GPU (kernels/jpeg_decode.hip behind runtime/jpeg.py):
full-resolution output against Pillow and against the float64 model on the
same coefficients, resize + crop against load_image_u8, fallbacks inside a
batch, and the HBM-resident GpuJpegSource.

Bounds (set by the issue): against Pillow max <= 4 levels and mean <= 0.13 --
libjpeg's integer IDCT is within 1 level of the exact one per plane, which the
colour matrix carries to <= 3, plus one level for fp32 rounding at ties;
against the numpy model on the same coefficients max <= 1.

Measured on an MI355X: see docs/KERNELS.md, "JPEG decode"."""
import numpy as np
import pytest
import torch
from jpeg_cases import (MAX_GPU, MEAN_BOUND, diff_stats, encode, full_res_cases, pil_rgb, png, progressive,
                        resize_cases)

from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_full_resolution_mixed_batch_matches_pillow_and_model():
    cases = full_res_cases()
    imgs, info = jpeg.decode_batch([d for _, d in cases], DEV, resize=None, crop=None)
    assert info["fallbacks"] == [] and info["gpu_images"] == len(cases)
    worst = [0, 0.0, 0]
    for (name, data), t in zip(cases, imgs):
        got = t.cpu().numpy()
        want = pil_rgb(data)
        assert got.shape == want.shape and got.dtype == np.uint8, name
        mx, mean = diff_stats(got, want)
        hdr, coefs = jpeg.entropy_decode(data)
        mm, _ = diff_stats(got, jpeg.reference_backend(hdr, coefs))
        worst = [max(worst[0], mx), max(worst[1], mean), max(worst[2], mm)]
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)
        assert mm <= 1, (name, mm)
    print(f"full resolution, {len(cases)} images: vs Pillow max {worst[0]} mean <= {worst[1]:.4f}; vs model max {worst[2]}")


def test_resize_crop_matches_load_image_u8_batched_and_single():
    cases = resize_cases()
    datas = [d for _, d in cases]
    out, info = jpeg.decode_batch(datas, DEV)
    assert out.shape == (len(cases), 224, 224, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    assert info["fallbacks"] == []
    worst = [0, 0.0, 0]
    for i, (name, data) in enumerate(cases):
        got = out[i].cpu().numpy()
        mx, mean = diff_stats(got, load_image_u8(data))
        hdr, coefs = jpeg.entropy_decode(data)
        mm, _ = diff_stats(got, jpeg.reference_resize_crop(jpeg.reference_backend(hdr, coefs)))
        worst = [max(worst[0], mx), max(worst[1], mean), max(worst[2], mm)]
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)
        # against the model: <= 1 at full resolution (fp32 IDCT ties), and both resize passes keep
        # that -- same taps, convex weights, and rounding is monotone: |a - b| <= 1 rounds to <= 1
        assert mm <= 1, (name, mm)
        one, _ = jpeg.decode_batch([data], DEV)
        assert torch.equal(one[0], out[i]), name                 # a batch of one: bit-identical
    print(f"resize + crop: vs load_image_u8 max {worst[0]} mean <= {worst[1]:.4f}; vs model max {worst[2]}")


def test_fallbacks_inside_a_batch():
    base = [d for _, d in resize_cases()[:3]]
    datas = [base[0], progressive(), base[1], png(), None, base[2]]
    out, info = jpeg.decode_batch(datas, DEV)
    assert [(i, r) for i, r in info["fallbacks"]] == [(1, "progressive"), (3, "not_jpeg")]
    assert info["gpu_images"] == 3
    for i in (1, 3):
        assert np.array_equal(out[i].cpu().numpy(), load_image_u8(datas[i])), i
    assert int(out[4].sum()) == 0
    alone, _ = jpeg.decode_batch(base, DEV)
    for j, i in enumerate((0, 2, 5)):
        assert torch.equal(out[i], alone[j]), i                  # unchanged by their neighbours


def _write_dir(tmp_path, n=6):
    spec = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (120, 90, "420"), (300, 280, "grey"),
            (260, 300, "420")]
    for i in range(n):
        w, h, sub = spec[i % len(spec)]
        (tmp_path / f"test_{i}.JPEG").write_bytes(encode(w, h, sub, 90, seed=70 + i, smooth=True))


def test_gpu_jpeg_source_is_resident_and_evicts(tmp_path):
    _write_dir(tmp_path)
    src = GpuJpegSource(DEV, root=str(tmp_path))
    assert not src.cached(0, 5)
    a = src.get(0, 5)
    assert a.shape == (6, 224, 224, 3) and a.dtype == torch.uint8 and a.is_cuda and a.is_contiguous()
    assert src.cached(0, 5) and src.decoded == 6 and src.fallbacks == 0
    b = src.get(0, 5)
    assert torch.equal(a, b) and src.decoded == 6 and src.cache_hits == 6
    for i in range(6):
        mx, mean = diff_stats(a[i].cpu().numpy(), load_image_u8((tmp_path / f"test_{i}.JPEG").read_bytes()))
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (i, mx, mean)
    small = GpuJpegSource(DEV, root=str(tmp_path), cache_bytes=4 * 224 * 224 * 3)
    c = small.get(0, 5)
    assert torch.equal(c, a) and small.decoded == 6 and not small.cached(0, 1) and small.cached(2, 5)
    d = small.get(0, 5)                                         # 0 and 1 decoded again, 2..5 from HBM
    assert torch.equal(d, a) and small.decoded == 8 and small.cache_hits == 4


def test_hip_executor_takes_the_source_tensor(tmp_path):
    from idunno.runtime.executor import HipExecutor

    _write_dir(tmp_path)
    src = GpuJpegSource(DEV, root=str(tmp_path))
    x = src.get(0, 5)
    assert x.dtype == torch.uint8 and x.is_cuda and x.is_contiguous() and x.shape == (6, 224, 224, 3)
    ex = HipExecutor(torch.device("cuda", torch.cuda.current_device()), seed=3, dtype="fp16")
    cls, prob = ex.run("resnet18", x, 0, 5)
    assert len(cls) == 6 and len(prob) == 6 and all(0 <= int(c) < 1000 for c in cls)
    assert all(0 < float(p) <= 1 for p in prob)
    # the same pixels staged from the host give the same answer: the tensor was read as it is
    cls2, prob2 = ex.run("resnet18", x.cpu().to(x.device), 0, 5)
    assert list(cls) == list(cls2) and np.allclose(prob, prob2)
