"""``sampling="native"`` on the GPU: 4:4:0 (mode 3) and 4:1:1 (mode 4) files
(tests/jpeg_sampling_cases.py) in the three entropy forms.  The device entropy
kernels give the host decoder's statuses and coefficients on the new MCU shapes
(baseline, restart-interval and progressive files; one mixed batch and batches of
one); the IDCT and the two new upsamplers of jpeg_resize_crop_kernel stay within
the project's bounds against Pillow on the very same bytes and within one level of
the float64 model (their planes come from the fp64 pass jpeg_idct_exact_kernel);
the default keyword still hands exactly these files to Pillow; GpuJpegSource and deeplearning take the keyword."""
import functools

import numpy as np
import pytest
import torch
from jpeg_cases import MAX_GPU, MEAN_BOUND, diff_stats, encode, pil_rgb
from jpeg_cases import resize_cases as plain_resize_cases
from jpeg_sampling_cases import full_res_cases, named, progressive_cases, resize_cases

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("host", "gpu", "gpu_parallel")
DEVICE_FORMS = ("gpu", "gpu_parallel")
NS = len(full_res_cases())                         # 51, at the front of the mixed batch
RST = [c[0] for c in full_res_cases()].index("440-70x46-rst2")
NATIVE = dict(sampling="native", progressive="native")


@functools.lru_cache(maxsize=None)
def mixed():
    """Every full-resolution case, then ordinary 4:2:0 / 4:2:2 / 4:4:4 / grey files (one with
    restart markers) and a None."""
    plain = [encode(70, 46, "420", 75, seed=1), encode(54, 22, "422", 95, seed=2), encode(17, 9, "444", 50, seed=3),
             encode(67, 45, "grey", 75, seed=4), encode(70, 46, "420", 75, seed=8, restart_marker_blocks=3)]
    return tuple([c[1] for c in full_res_cases()] + plain + [None])


@functools.lru_cache(maxsize=None)
def host_coefs(which):
    """The host decoder over a batch, computed once: (status, offsets, coefficients)."""
    datas = list(mixed()) if which == "mixed" else [c[1] for c in progressive_cases()]
    return jpeg.entropy_coefs(datas, entropy_on="host", **NATIVE)


@functools.lru_cache(maxsize=None)
def model(which):
    """The float64 model of every image of a case list from the host decoder's coefficients, computed once."""
    cases = {"full": full_res_cases, "prog": progressive_cases, "resize": resize_cases}[which]()
    out = []
    for _, d, _ in cases:
        h, c = jpeg.entropy_decode(d, **NATIVE)
        rgb = jpeg.reference_backend(h, c)
        out.append(jpeg.reference_resize_crop(rgb) if which == "resize" else rgb)
    return tuple(out)


def _assert_same_coefs(datas, form, want=None, **kw):
    hs, ho, hc = want or jpeg.entropy_coefs(datas, entropy_on="host", **NATIVE)
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on=form, **NATIVE, **kw)
    assert gs == hs and go == ho and gc.dtype == torch.int16 and gc.shape == hc.shape
    for i, d in enumerate(datas):
        if hs[i] == 0:
            n = jpeg.parse(d, **NATIVE)["total_coefs"]
            assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), f"{form}: image {i}: coefficients differ"
    return gs


@pytest.mark.parametrize("form", DEVICE_FORMS)
def test_coefficients_of_the_mixed_batch_equal_the_host_decoders(form):
    datas = list(mixed())
    par = form == "gpu_parallel"
    pk = ops.jpeg_huff_pack(datas, par, False, False, True)
    assert pk.native_sampling is True and pk.status == [0] * (len(datas) - 1) + [1] and pk.n_gpu == len(datas) - 1
    # the two files with restart markers stay on one lane each, the rest is laid out for the form
    assert (pk.n_lane, pk.n_par) == ((2, len(datas) - 3) if par else (len(datas) - 1, 0))
    modes = pk.hdr.numpy().view(np.int32)[:NS, ops.JPEG_HEADER_MODE_OFFSET // 4].tolist()
    assert modes == [c[2] for c in full_res_cases()]
    st = _assert_same_coefs(datas, form, host_coefs("mixed"))
    assert st == [0] * (len(datas) - 1) + [1]
    # one restart interval per lane: the 4:4:0 file with markers and the ordinary one take the interval kernel
    pk = ops.jpeg_huff_pack(datas, par, False, True, True)
    assert pk.n_rst == 2 and sorted(set(pk.rst_items[:, 0].tolist())) == [RST, len(datas) - 2]
    assert _assert_same_coefs(datas, form, host_coefs("mixed"), restart="intervals") == st
    # without the keyword the new layouts are refused by the parse, the rest is decoded as before
    gs, go, _ = jpeg.entropy_coefs(datas, DEV, entropy_on=form)
    assert gs == [9] * NS + [0] * 5 + [1] and go[:NS] == [-1] * NS


@pytest.mark.parametrize("form", DEVICE_FORMS)
def test_coefficients_in_batches_of_one(form):
    hs, ho, hc = host_coefs("mixed")
    for i, d in enumerate(mixed()[:-1]):
        n = jpeg.parse(d, **NATIVE)["total_coefs"]
        for kw in ({}, {"restart": "intervals"}) if i == RST else ({},):
            gs, go, gc = jpeg.entropy_coefs([d], DEV, entropy_on=form, **NATIVE, **kw)
            assert gs == [0] and go == [0] and gc.numel() == n, (i, gs)
            assert torch.equal(gc, hc[ho[i]:ho[i] + n]), f"{form}: image {i} alone: coefficients differ"
    rst = mixed()[RST]
    assert ops.jpeg_huff_pack([rst], form == "gpu_parallel", False, True, True).n_rst == 1
    assert jpeg.entropy_coefs([None], DEV, entropy_on=form, **NATIVE)[0] == [1]


@pytest.mark.parametrize("form", FORMS)
def test_progressive_coefficients_equal_the_host_decoders(form):
    datas = [c[1] for c in progressive_cases()]
    if form != "host":
        pk = ops.jpeg_huff_pack(datas, form == "gpu_parallel", True, False, True)
        assert pk.n_prog == len(datas) and pk.nscans == 10 * len(datas)
    assert _assert_same_coefs(datas, form, host_coefs("prog")) == [0] * len(datas)
    hs, ho, hc = host_coefs("prog")
    for i, d in enumerate(datas):                                  # batches of one, against the single-image decoder too
        h, c = jpeg.entropy_decode(d, **NATIVE)
        gs, go, gc = jpeg.entropy_coefs([d], DEV, entropy_on=form, **NATIVE)
        assert gs == [0] and np.array_equal(gc.numpy(), c), (form, i)
        assert torch.equal(gc, hc[ho[i]:ho[i] + h["total_coefs"]])
    # progressive="native" alone does not take them
    assert jpeg.entropy_coefs(datas, DEV, entropy_on=form, progressive="native")[0] == [9] * len(datas)


def test_pixels_at_full_resolution_in_every_form():
    cases = full_res_cases() + progressive_cases()
    want = model("full") + model("prog")
    datas = [c[1] for c in cases]
    outs = []
    for form in FORMS:
        imgs, info = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=form, **NATIVE)
        assert info["fallbacks"] == [] and info["sampling"] == "native" and info["entropy_on"] == form
        assert info["sampling_images"] == len(datas) == info["gpu_images"]
        assert info["progressive_images"] == len(progressive_cases())
        outs.append(imgs)
    for k, (name, d, _) in enumerate(cases):
        got = outs[0][k].cpu().numpy()
        ref = pil_rgb(d)
        assert got.shape == ref.shape, name
        mx, mean = diff_stats(got, ref)
        mm, _ = diff_stats(got, want[k])
        print(name, "vs Pillow", mx, round(mean, 4), "vs model", mm)
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)
        assert mm <= 1, (name, mm)
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), name
    # restart="intervals" changes nothing of the pixels, and alone an image is what it is in the batch
    imgs, info = jpeg.decode_batch(datas[:NS], DEV, resize=None, crop=None, entropy_on="gpu", restart="intervals", **NATIVE)
    assert info["fallbacks"] == [] and info["restart_images"] == 1
    assert all(torch.equal(a, b) for a, b in zip(imgs, outs[0]))
    for name in ("440-2x33-q50", "440-67x45-q95", "411-27x5-q50", "411-161x9-q95"):
        k = [c[0] for c in cases].index(name)
        alone, _ = jpeg.decode_batch([datas[k]], DEV, resize=None, crop=None, **NATIVE)
        assert torch.equal(alone[0], outs[0][k]), name


@functools.lru_cache(maxsize=None)
def resized():
    """The four resize cases through Resize(256) + CenterCrop(224) in one batch, per form, computed once."""
    datas = [c[1] for c in resize_cases()]
    outs = []
    for form in FORMS:
        imgs, info = jpeg.decode_batch(datas, DEV, entropy_on=form, sampling="native")
        assert info["fallbacks"] == [] and info["sampling_images"] == 4 == info["gpu_images"]
        assert imgs.shape == (4, 224, 224, 3)
        outs.append(imgs)
    return tuple(outs)


def test_the_plan_counts_the_images_of_the_fp64_pass():
    datas = list(mixed())
    st, hdr, coefs, offs = ops.jpeg_entropy_batch(datas, 2, False, True)
    plan = ops.jpeg_plan(hdr, list(st), offs, coefs.numel(), None, 0, DEV)
    assert plan.n_gpu == len(datas) - 1 and plan.n_exact == NS
    st, hdr, coefs, offs = ops.jpeg_entropy_batch(datas, 2)                        # the default: none of them is planned
    plan = ops.jpeg_plan(hdr, list(st), offs, coefs.numel(), None, 0, DEV)
    assert plan.n_gpu == 5 and plan.n_exact == 0


def test_resize_and_crop_batched_and_alone():
    outs = resized()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for k, (name, d, _) in enumerate(resize_cases()):
        mx, mean = diff_stats(outs[0][k].cpu().numpy(), load_image_u8(d))
        print(name, "vs load_image_u8", mx, round(mean, 4))
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)
        alone, _ = jpeg.decode_batch([d], DEV, sampling="native")
        assert torch.equal(alone[0], outs[0][k]), name


@pytest.mark.parametrize("name", [c[0] for c in resize_cases()])
def test_resize_and_crop_against_the_model(name):
    """At most one level from the float64 model after both resize passes.  411-640x120 holds a Cr
    sample whose exact value is 164.5000034: an fp32 IDCT cannot tell it from 164.5, and R = Y + 1.402 Cr
    turns that one level of Cr into two of R at the four pixels the sample is replicated to, which is why
    the planes of these two layouts come from jpeg_idct_exact_kernel (fp64)."""
    k = [c[0] for c in resize_cases()].index(name)
    mm, _ = diff_stats(resized()[0][k].cpu().numpy(), model("resize")[k])
    print(name, "vs model", mm)
    assert mm <= 1, (name, mm)


@pytest.mark.parametrize("form", FORMS)
def test_the_default_hands_exactly_these_files_to_pillow(form):
    # full resolution: the mixed batch
    datas = list(mixed())
    nat, ninfo = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=form, sampling="native")
    assert ninfo["fallbacks"] == [] and ninfo["sampling_images"] == NS
    for kw in ({}, {"sampling": "fallback"}):
        imgs, info = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=form, **kw)
        assert info["fallbacks"] == [(i, "sampling") for i in range(NS)]
        assert info["sampling"] == "fallback" and info["sampling_images"] == 0 and info["gpu_images"] == 5
        for i in range(NS):
            assert np.array_equal(imgs[i].cpu().numpy(), pil_rgb(datas[i]))
        for i in range(NS, len(datas) - 1):
            assert torch.equal(imgs[i], nat[i])
        assert imgs[-1] is None and nat[-1] is None
    # resized and cropped: the four resize cases between ordinary files
    plain = [d for _, d in plain_resize_cases()[:3]]
    datas = [plain[0]] + [c[1] for c in resize_cases()] + plain[1:] + [None]
    at = [1, 2, 3, 4]
    nat, ninfo = jpeg.decode_batch(datas, DEV, entropy_on=form, sampling="native")
    imgs, info = jpeg.decode_batch(datas, DEV, entropy_on=form)
    assert ninfo["fallbacks"] == [] and ninfo["sampling_images"] == 4
    assert info["fallbacks"] == [(i, "sampling") for i in at] and info["sampling_images"] == 0
    for i in range(len(datas)):
        if i in at:
            assert np.array_equal(imgs[i].cpu().numpy(), load_image_u8(datas[i]))
        else:
            assert torch.equal(imgs[i], nat[i])


@pytest.mark.parametrize("form", FORMS)
def test_a_prepared_entropy_stage_decides_the_mode(form):
    datas = [c[1] for c in resize_cases()]
    want, _ = jpeg.decode_batch(datas, DEV, sampling="native")
    ent = jpeg.entropy_batch(datas, 2, form, sampling="native")
    imgs, info = jpeg.decode_batch(datas, DEV, entropy=ent)                       # asked for the default, prepared native
    assert info["sampling"] == "native" and info["fallbacks"] == [] and info["sampling_images"] == 4
    assert info["entropy_on"] == form and torch.equal(imgs, want)
    ent = jpeg.entropy_batch(datas, 2, form)                                      # and the other way round
    imgs, info = jpeg.decode_batch(datas, DEV, entropy=ent, sampling="native")
    assert info["sampling"] == "fallback" and info["sampling_images"] == 0
    assert info["fallbacks"] == [(i, "sampling") for i in range(4)]


@pytest.mark.parametrize("form", FORMS)
def test_gpu_jpeg_source_counts_the_native_images(tmp_path, form):
    datas = [c[1] for c in resize_cases()] + [plain_resize_cases()[0][1]]
    for i, d in enumerate(datas):
        (tmp_path / f"test_{i}.JPEG").write_bytes(d)
    want, _ = jpeg.decode_batch(datas, DEV, sampling="native")
    src = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=form, sampling="native")
    assert torch.equal(src.get(0, 4), want)                      # cold
    assert src.decoded == 5 and src.fallbacks == 0 and src.sampling_images == 4 and src.sampling == "native"
    assert torch.equal(src.get(0, 4), want) and src.decoded == 5 and src.cache_hits == 5
    src.CHUNK = src.CHUNK_GPU = src.CHUNK_GPU_PARALLEL = 2       # more than one chunk: the prepare-ahead thread
    src.invalidate()
    assert torch.equal(src.get(0, 4), want) and src.decoded == 10 and src.fallbacks == 0 and src.sampling_images == 8
    old = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=form)        # the default: these files through Pillow
    rows = old.get(0, 4)
    assert old.fallbacks == 4 and old.sampling_images == 0 and old.sampling == "fallback"
    assert old.fallback_reasons == {i: "sampling" for i in range(4)}
    assert torch.equal(rows[4], want[4])
    for i in range(4):
        assert np.array_equal(rows[i].cpu().numpy(), load_image_u8(datas[i]))


def test_deeplearning_takes_the_keyword(tmp_path):
    from idunno import inference

    d = tmp_path / "resnet18"
    d.mkdir()
    datas = [c[1] for c in resize_cases()] + [plain_resize_cases()[0][1]]
    for i, f in enumerate(datas):
        (d / f"test_{i}.JPEG").write_bytes(f)
    inference.drop_gpu_sources()
    try:
        pil, _ = inference.deeplearning("resnet18", "resnet18", 0, 4, device=DEV, root=str(tmp_path), topk=2)
        gpu, _ = inference.deeplearning("resnet18", "resnet18", 0, 4, device=DEV, root=str(tmp_path), topk=2,
                                        decoder="gpu", sampling="native")
        srcs = [s for k, s in inference._GPU_SOURCES.items() if k[-1] == "native"]
        assert len(srcs) == 1 and srcs[0].fallbacks == 0 and srcs[0].sampling_images == 4 and srcs[0].decoded == 5
        old, _ = inference.deeplearning("resnet18", "resnet18", 0, 4, device=DEV, root=str(tmp_path), topk=2, decoder="gpu")
        assert len(inference._GPU_SOURCES) == 2                  # the keyword is part of the key
        srcs = [s for k, s in inference._GPU_SOURCES.items() if k[-1] == "fallback"]
        assert len(srcs) == 1 and srcs[0].fallbacks == 4 and srcs[0].sampling_images == 0
    finally:
        inference.drop_gpu_sources()
    # a tie: the two best classes of the Pillow run within 5% of each other.  The decoders differ by at most
    # MAX_GPU levels in single pixels and MEAN_BOUND on average (5e-4 of the range), which moves no probability
    # by a twentieth of itself; the random-init network's margins on these images are 20% and more.
    clear = [i for i, (_, _, p) in enumerate(pil) if p[0] - p[1] > 0.05 * p[0]]
    assert len(clear) == 5
    for i in clear:
        assert gpu[i][0] == pil[i][0] == old[i][0] and gpu[i][1][0] == pil[i][1][0] == old[i][1][0], (i, gpu[i], pil[i])
