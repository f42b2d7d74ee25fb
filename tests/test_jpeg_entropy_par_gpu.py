"""The sub-stream device entropy stage (jpeg_entropy_par_kernel behind
``entropy_on="gpu_parallel"``: one workgroup per image, csrc/jpeg_huff_par.h):
its coefficients are bit-identical to the host decoder's, so decode_batch
outputs are ``torch.equal`` to the host form's (no tolerance: same
coefficients, same kernels), fallbacks included, files with restart markers go
to the one-lane kernel inside the same batch, and GpuJpegSource serves the same
rows."""
import numpy as np
import pytest
import torch
from jpeg_cases import encode, full_res_cases, png, progressive, resize_cases
from jpeg_entropy_cases import noise_q100, rst1, scan_mutant

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORM = "gpu_parallel"


def _scan_bits(data: bytes) -> int:
    """Bits of the entropy-coded segment as the packer hands them over: FF 00 is one byte, cut at EOI."""
    scan = data[data.index(b"\xff\xda"):]
    scan = scan[2 + int.from_bytes(scan[2:4], "big"):]
    return 8 * len(scan[:scan.rindex(b"\xff\xd9")].replace(b"\xff\x00", b"\xff"))


def _assert_same_coefs(datas):
    hs, ho, hc = jpeg.entropy_coefs(datas, entropy_on="host")
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on=FORM)
    assert gs == hs == [0] * len(datas)
    assert go == ho and gc.dtype == torch.int16 and gc.shape == hc.shape
    ends = ho[1:] + [hc.numel()]
    for i, (a, b) in enumerate(zip(ho, ends)):
        assert torch.equal(gc[a:b], hc[a:b]), f"image {i}: coefficients differ"


def test_coefficients_are_bit_identical_to_the_host_decoder():
    cases = full_res_cases()
    base = [d for _, d in cases] + [rst1(), noise_q100()]
    assert len(base) == 53
    datas = base + base[:47]                     # 100 images, restart files among them (one-lane kernel, same batch)
    tiny = dict(cases)["8x8-444-q50"]
    assert _scan_bits(tiny) == 72 <= ops.JPEG_PAR_SUB_BITS           # one sub-stream
    assert any(_scan_bits(d) > 4 * ops.JPEG_PAR_SUB_BITS for d in base)
    packed = ops.jpeg_huff_pack(datas, True)
    assert packed.n_par == 98 and packed.n_lane == 2                 # 70x46-420-rst3 and rst1: the one-lane kernel
    _assert_same_coefs(datas)
    _assert_same_coefs([noise_q100()])           # batches of one
    _assert_same_coefs([rst1()])
    _assert_same_coefs([tiny])


def test_more_sub_streams_than_threads():
    per_pass = ops.JPEG_PAR_SUB_BITS * ops.JPEG_PAR_THREADS
    for w, h in ((640, 480), (1024, 768), (2048, 1536)):
        big = encode(w, h, "444", 95, seed=21)
        if _scan_bits(big) > per_pass:
            break
    assert _scan_bits(big) > per_pass            # threads take more than one sub-stream each
    _assert_same_coefs([big])


def test_images_equal_the_host_form():
    datas = [d for _, d in resize_cases()]
    host, hinfo = jpeg.decode_batch(datas, DEV, entropy_on="host")
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on=FORM)
    assert hinfo["entropy_on"] == "host" and ginfo["entropy_on"] == FORM
    assert ginfo["fallbacks"] == [] and ginfo["gpu_images"] == len(datas)
    assert torch.equal(gpu, host)
    assert ginfo["entropy_s"] > 0 and 0 < ginfo["h2d_bytes"] < sum(len(d) for d in datas) + 16 * len(datas)
    full_h, _ = jpeg.decode_batch(datas, DEV, resize=None, crop=None)
    full_g, finfo = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=FORM)
    assert finfo["fallbacks"] == []
    for a, b in zip(full_h, full_g):
        assert torch.equal(a, b)


def test_mixed_batch_falls_back_like_the_host_form():
    base = [d for _, d in resize_cases()[:3]]
    half = base[1][:len(base[1]) // 2]
    datas = [base[0], progressive(), base[1], png(), None, base[2], scan_mutant()]
    host, hinfo = jpeg.decode_batch(datas, DEV)
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on=FORM)
    assert ginfo["fallbacks"] == hinfo["fallbacks"]
    assert [r for _, r in ginfo["fallbacks"]] == ["progressive", "not_jpeg", "corrupt"]
    assert ginfo["gpu_images"] == hinfo["gpu_images"] == 3
    assert torch.equal(gpu, host)
    assert int(gpu[4].sum()) == 0
    assert np.array_equal(gpu[6].cpu().numpy(), load_image_u8(datas[6]))
    alone, _ = jpeg.decode_batch(base, DEV, entropy_on=FORM)
    for j, i in enumerate((0, 2, 5)):
        assert torch.equal(gpu[i], alone[j]), i                  # unchanged by their neighbours
    # a file cut in half: refused like the host decoder does (corrupt), its neighbours' coefficients untouched
    cut = datas + [half]
    hs, ho, hc = jpeg.entropy_coefs(cut, entropy_on="host")
    gs, go, gc = jpeg.entropy_coefs(cut, DEV, entropy_on=FORM)
    assert gs == hs and hs[6:] == [3, 3] and go == ho
    for i in (0, 2, 5):
        n = jpeg.parse(cut[i])["total_coefs"]
        assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), i


def test_gpu_jpeg_source_with_sub_stream_entropy(tmp_path):
    spec = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (120, 90, "420"), (300, 280, "grey"),
            (260, 300, "420")]
    for i, (w, h, sub) in enumerate(spec):
        (tmp_path / f"test_{i}.JPEG").write_bytes(encode(w, h, sub, 90, seed=70 + i, smooth=True))
    want = GpuJpegSource(DEV, root=str(tmp_path)).get(0, 5)
    src = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=FORM)
    a = src.get(0, 5)                                            # cold
    assert torch.equal(a, want) and src.decoded == 6 and src.fallbacks == 0 and src.seconds["entropy_s"] > 0
    b = src.get(0, 5)                                            # resident: decodes nothing
    assert torch.equal(b, want) and src.decoded == 6 and src.cache_hits == 6
    src.CHUNK_GPU_PARALLEL = 4                                   # more than one chunk: the prepare-ahead thread
    src.invalidate()
    assert torch.equal(src.get(0, 5), want) and src.decoded == 12
