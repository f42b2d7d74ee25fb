"""JPEG source without a GPU: the native host entropy decoder and the float64
numpy model of the GPU chain against Pillow, the decoder's status codes, and the
CPU behaviour of decode_batch / GpuJpegSource / deeplearning / the launcher."""
import numpy as np
import pytest
import torch
from jpeg_cases import (MAX_MODEL, MEAN_BOUND, cmyk, diff_stats, encode, full_res_cases, pil_rgb, png, progressive,
                        resize_cases)

from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, JpegSource, load_image_u8


@pytest.mark.parametrize("name,data", full_res_cases(), ids=[n for n, _ in full_res_cases()])
def test_host_decoder_and_model_match_pillow_full_resolution(name, data):
    got = jpeg.entropy_decode(data)
    assert not isinstance(got, str), got
    hdr, coefs = got
    assert coefs.dtype == np.int16 and coefs.size == hdr["total_coefs"]
    want = pil_rgb(data)
    assert (hdr["H"], hdr["W"]) == want.shape[:2]
    mx, mean = diff_stats(jpeg.reference_backend(hdr, coefs), want)
    print(f"{name}: max {mx} mean {mean:.4f}")
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


@pytest.mark.parametrize("name,data", resize_cases(), ids=[n for n, _ in resize_cases()])
def test_model_matches_load_image_u8_after_resize_crop(name, data):
    hdr, coefs = jpeg.entropy_decode(data)
    got = jpeg.reference_resize_crop(jpeg.reference_backend(hdr, coefs))
    mx, mean = diff_stats(got, load_image_u8(data))
    print(f"{name}: max {mx} mean {mean:.4f}")
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


def test_header_fields():
    hdr = jpeg.parse(encode(70, 46, "420", 75, seed=1))
    assert (hdr["W"], hdr["H"], hdr["ncomp"], hdr["mode"]) == (70, 46, 3, 2)
    y, cb, cr = hdr["comp"]
    assert (y["h"], y["v"], y["bw"], y["bh"]) == (2, 2, 10, 6) and (cb["bw"], cb["bh"]) == (5, 3)
    assert cb["coef_off"] == 10 * 6 * 64 and cr["coef_off"] == cb["coef_off"] + 5 * 3 * 64
    assert len(y["q"]) == 64 and all(1 <= v <= 255 for v in y["q"])
    assert jpeg.parse(encode(54, 22, "422", 75))["mode"] == 1
    assert jpeg.parse(encode(17, 9, "444", 75))["mode"] == 0
    g = jpeg.parse(encode(67, 45, "grey", 75))
    assert g["ncomp"] == 1 and (g["comp"][0]["bw"], g["comp"][0]["bh"]) == (9, 6)


def test_status_codes_each_have_their_own_reason():
    base = encode(64, 48, "420", 75, seed=2)
    reasons = {
        "progressive": jpeg.parse(progressive()),
        "cmyk": jpeg.parse(cmyk()),
        "png": jpeg.parse(png()),
        "empty": jpeg.parse(b""),
        "cut": jpeg.entropy_decode(base[:len(base) // 2]),
    }
    assert reasons == {"progressive": "progressive", "cmyk": "components", "png": "not_jpeg", "empty": "empty",
                       "cut": "corrupt"}
    # the batch entry reports the same through its status list, and never raises
    for bad in (progressive(), cmyk(), png(), b"", base[:len(base) // 2], base[:3], b"\xff\xd8\xff"):
        assert isinstance(jpeg.entropy_decode(bad), str)
    assert not isinstance(jpeg.entropy_decode(base), str)


def test_decode_batch_on_cpu_is_load_image_u8():
    datas = [encode(333, 250, "420", 90, seed=3, smooth=True), None, progressive(), png(),
             encode(120, 90, "444", 90, seed=4, smooth=True)]
    out, info = jpeg.decode_batch(datas, "cpu")
    assert out.shape == (5, 224, 224, 3) and out.dtype == torch.uint8 and out.device.type == "cpu"
    for i, d in enumerate(datas):
        want = np.zeros((224, 224, 3), np.uint8) if d is None else load_image_u8(d)
        assert np.array_equal(out[i].numpy(), want), i
    # no half-path: every present image is reported as decoded by Pillow
    assert [i for i, _ in info["fallbacks"]] == [0, 2, 3, 4] and info["gpu_images"] == 0
    full, _ = jpeg.decode_batch(datas[:2], "cpu", resize=None, crop=None)
    assert full[1] is None and np.array_equal(full[0].numpy(), pil_rgb(datas[0]))


def _write_dir(tmp_path):
    sizes = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (280, 260, "grey")]
    for i, (w, h, sub) in enumerate(sizes):
        (tmp_path / f"test_{i}.JPEG").write_bytes(encode(w, h, sub, 90, seed=20 + i, smooth=True))
    (tmp_path / "test_5.JPEG").write_bytes(progressive())          # index 4 is missing
    return 5


def test_gpu_jpeg_source_on_cpu_equals_jpeg_source_and_caches(tmp_path):
    last = _write_dir(tmp_path)
    old = JpegSource("cpu", root=str(tmp_path))
    new = GpuJpegSource("cpu", root=str(tmp_path))
    assert not new.cached(0, last)
    a, b = old.get(0, last), new.get(0, last)
    assert b.dtype == torch.uint8 and b.is_contiguous() and torch.equal(a, b)
    assert old.missing == [4] and new.missing == [4] and int(b[4].sum()) == 0
    assert new.decoded == 5 and new.fallbacks == 5 and new.cache_hits == 0
    # what was decoded is resident; the unreadable index is not (it is read again every time)
    assert new.cached(0, 3) and new.cached(5, 5) and not new.cached(4, 4) and not new.cached(0, last)
    c = new.get(0, last)
    assert torch.equal(b, c) and new.decoded == 5 and new.cache_hits == 5      # served from the cache
    assert new.missing == [4, 4] and torch.equal(old.get(0, last), c) and old.missing == [4, 4]
    assert torch.equal(new.get(2, 3), a[2:4]) and new.decoded == 5
    new.invalidate(2, 2)
    assert not new.cached(2, 3) and torch.equal(new.get(2, 3), a[2:4]) and new.decoded == 6
    # a cache of two images: oldest evicted first, decoded again on the next request
    small = GpuJpegSource("cpu", root=str(tmp_path), cache_bytes=2 * 224 * 224 * 3)
    assert torch.equal(small.get(0, 3), a[:4]) and small.decoded == 4
    assert not small.cached(0, 1) and small.cached(2, 3)
    assert torch.equal(small.get(0, 3), a[:4]) and small.decoded == 6
    # prefetch fills the cache in the background
    pf = GpuJpegSource("cpu", root=str(tmp_path))
    pf.prefetch(0, 1)
    pf._pool.shutdown(wait=True)
    assert pf.cached(0, 1) and pf.decoded == 2


class _FlakyStore:
    """SDFS stand-in whose get_bytes gives None for names not stored (yet)."""

    def __init__(self):
        self.files = {}

    def get_bytes(self, name):
        return self.files.get(name)


def test_gpu_jpeg_source_reads_an_unreadable_file_again():
    """A file that is not there at the first get (not put yet, no replica
    answered) must not stay a zero image: once it can be read it is decoded."""
    store = _FlakyStore()
    d0, d1 = encode(300, 260, "420", 90, seed=40, smooth=True), encode(260, 300, "422", 90, seed=41, smooth=True)
    store.files["test_0.JPEG"] = d0
    src = GpuJpegSource("cpu", sdfs=store)
    x = src.get(0, 1)
    assert src.missing == [1] and int(x[1].sum()) == 0 and np.array_equal(x[0].numpy(), load_image_u8(d0))
    assert src.cached(0, 0) and not src.cached(1, 1) and not src.cached(0, 1)
    y = src.get(0, 1)                                   # still absent: reported again, still not cached
    assert src.missing == [1, 1] and int(y[1].sum()) == 0 and src.decoded == 1
    store.files["test_1.JPEG"] = d1                     # the put arrives
    z = src.get(0, 1)
    assert np.array_equal(z[1].numpy(), load_image_u8(d1)) and np.array_equal(z[0].numpy(), load_image_u8(d0))
    assert src.missing == [1, 1] and src.decoded == 2 and src.cached(0, 1)
    assert torch.equal(src.get(0, 1), z) and src.decoded == 2


def test_launcher_accepts_jpeg_source():
    from idunno.launch import build_parser

    a = build_parser().parse_args(["node", "--source", "jpeg"])
    assert a.source == "jpeg"
    assert build_parser().parse_args(["node"]).source == "synthetic"        # the default is unchanged
    with pytest.raises(SystemExit):
        build_parser().parse_args(["node", "--source", "tiff"])


def test_deeplearning_gpu_decoder_on_cpu_returns_reference_tuples(tmp_path):
    from idunno.inference import deeplearning

    d = tmp_path / "alexnet"
    d.mkdir()
    for i in range(2):
        (d / f"test_{i}.JPEG").write_bytes(encode(300, 260, "420", 90, seed=30 + i, smooth=True))
    res, dt = deeplearning("alexnet", "alexnet", 0, 1, device="cpu", root=str(tmp_path), decoder="gpu")
    assert [r[0] for r in res] == ["test_0.JPEG", "test_1.JPEG"] and dt > 0
    assert all(isinstance(c, str) and 0 < p <= 1 for _, c, p in res)
    ref, _ = deeplearning("alexnet", "alexnet", 0, 1, device="cpu", root=str(tmp_path))     # default: Pillow
    assert [(n, c) for n, c, _ in ref] == [(n, c) for n, c, _ in res]
    assert max(abs(a[2] - b[2]) for a, b in zip(res, ref)) < 1e-6
    with pytest.raises(ValueError):
        deeplearning("alexnet", "alexnet", 0, 0, device="cpu", root=str(tmp_path), decoder="nv")
