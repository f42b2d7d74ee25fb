"""The opt-in device entropy stage (kernels/jpeg_entropy.hip behind
``entropy_on="gpu"``): its coefficients are bit-identical to the host
decoder's, so everything downstream is too -- decode_batch outputs are
``torch.equal`` between the two forms (no tolerance: same coefficients, same
kernels), fallbacks included, and GpuJpegSource serves the same rows."""
import numpy as np
import pytest
import torch
from jpeg_cases import encode, full_res_cases, png, progressive, resize_cases
from jpeg_entropy_cases import noise_q100, rst1, scan_mutant

from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_same_coefs(datas):
    hs, ho, hc = jpeg.entropy_coefs(datas, entropy_on="host")
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on="gpu")
    assert gs == hs == [0] * len(datas)
    assert go == ho and gc.dtype == torch.int16 and gc.shape == hc.shape
    ends = ho[1:] + [hc.numel()]
    for i, (a, b) in enumerate(zip(ho, ends)):
        assert torch.equal(gc[a:b], hc[a:b]), f"image {i}: coefficients differ"


def test_coefficients_are_bit_identical_to_the_host_decoder():
    base = [d for _, d in full_res_cases()] + [rst1(), noise_q100()]
    assert len(base) == 53
    datas = base + base[:47]                     # 100 images: one full wave and a partial one
    assert 65 <= len(datas) <= 130
    _assert_same_coefs(datas)
    _assert_same_coefs([noise_q100()])           # a batch of one
    _assert_same_coefs([rst1()])


def test_images_equal_the_host_form():
    datas = [d for _, d in resize_cases()]
    host, hinfo = jpeg.decode_batch(datas, DEV, entropy_on="host")
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on="gpu")
    assert hinfo["entropy_on"] == "host" and ginfo["entropy_on"] == "gpu"
    assert ginfo["fallbacks"] == [] and ginfo["gpu_images"] == len(datas)
    assert torch.equal(gpu, host)
    assert ginfo["entropy_s"] > 0 and 0 < ginfo["h2d_bytes"] < sum(len(d) for d in datas) + 16 * len(datas)
    full_h, _ = jpeg.decode_batch(datas, DEV, resize=None, crop=None)
    full_g, _ = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on="gpu")
    for a, b in zip(full_h, full_g):
        assert torch.equal(a, b)


def test_mixed_batch_falls_back_like_the_host_form():
    base = [d for _, d in resize_cases()[:3]]
    half = base[1][:len(base[1]) // 2]
    datas = [base[0], progressive(), base[1], png(), None, base[2], scan_mutant()]
    host, hinfo = jpeg.decode_batch(datas, DEV)
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on="gpu")
    assert ginfo["fallbacks"] == hinfo["fallbacks"]
    assert [r for _, r in ginfo["fallbacks"]] == ["progressive", "not_jpeg", "corrupt"]
    assert ginfo["gpu_images"] == hinfo["gpu_images"] == 3
    assert torch.equal(gpu, host)
    assert int(gpu[4].sum()) == 0
    assert np.array_equal(gpu[6].cpu().numpy(), load_image_u8(datas[6]))
    alone, _ = jpeg.decode_batch(base, DEV, entropy_on="gpu")
    for j, i in enumerate((0, 2, 5)):
        assert torch.equal(gpu[i], alone[j]), i                  # unchanged by their neighbours
    # a file cut in half: the kernel refuses it like the host decoder (corrupt), and its neighbours'
    # coefficients are untouched.  Pillow does not load a truncated file, so the fallback of either
    # form raises the same OSError for a batch that holds it.
    cut = datas + [half]
    hs, ho, hc = jpeg.entropy_coefs(cut, entropy_on="host")
    gs, go, gc = jpeg.entropy_coefs(cut, DEV, entropy_on="gpu")
    assert gs == hs and hs[6:] == [3, 3] and go == ho
    for i in (0, 2, 5):
        n = jpeg.parse(cut[i])["total_coefs"]
        assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), i
    errs = []
    for form in ("host", "gpu"):
        with pytest.raises(OSError) as e:
            jpeg.decode_batch(cut, DEV, entropy_on=form)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "truncated" in errs[0]


def test_gpu_jpeg_source_with_device_entropy(tmp_path):
    spec = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (120, 90, "420"), (300, 280, "grey"),
            (260, 300, "420")]
    for i, (w, h, sub) in enumerate(spec):
        (tmp_path / f"test_{i}.JPEG").write_bytes(encode(w, h, sub, 90, seed=70 + i, smooth=True))
    want = GpuJpegSource(DEV, root=str(tmp_path)).get(0, 5)
    src = GpuJpegSource(DEV, root=str(tmp_path), entropy_on="gpu")
    a = src.get(0, 5)
    assert torch.equal(a, want) and src.decoded == 6 and src.fallbacks == 0 and src.seconds["entropy_s"] > 0
    b = src.get(0, 5)                                            # resident: decodes nothing
    assert torch.equal(b, want) and src.decoded == 6 and src.cache_hits == 6
    src.CHUNK_GPU = 4                                            # more than one chunk: the prepare-ahead thread
    src.invalidate()
    assert torch.equal(src.get(0, 5), want) and src.decoded == 12
