"""``colorspace="auto"`` on the GPU: RGB-coded, CMYK and YCCK files
(tests/jpeg_color_cases.py) in the three entropy forms.  The device entropy kernels give
the host decoder's statuses and coefficients (four-component files on the one-lane and
the progressive kernel, whatever the form); the colour stages of
jpeg_resize_crop_kernel stay within the derived bounds against Pillow on the very same
bytes and against the float64 model (their planes come from the fp64 pass
jpeg_idct_exact_kernel); the default keyword leaves every status and pixel as it was;
GpuJpegSource and deeplearning take the keyword."""
import functools

import numpy as np
import pytest
import torch
from jpeg_cases import diff_stats, encode, pil_rgb, png
from jpeg_cases import resize_cases as plain_resize_cases
from jpeg_color_cases import (CMYK, KIND, MAX_GPU_MODEL, MAX_PIL, MEAN_PIL, YCBCR, YCCK, full_res_cases,
                              progressive_cases, refusals, resize_cases)

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("host", "gpu", "gpu_parallel")
DEVICE_FORMS = ("gpu", "gpu_parallel")
AUTO = dict(colorspace="auto", progressive="native")
CASES = full_res_cases() + tuple(c[:3] for c in progressive_cases())
NAMES = [c[0] for c in CASES]
NF = len(full_res_cases())
NCOLOR = sum(1 for c in CASES if c[2] != YCBCR)
FOUR = [i for i, c in enumerate(CASES) if c[2] in (CMYK, YCCK)]


@functools.lru_cache(maxsize=None)
def host_coefs():
    """The host decoder over every case, computed once: (status, offsets, coefficients)."""
    return jpeg.entropy_coefs([c[1] for c in CASES], entropy_on="host", **AUTO)


@functools.lru_cache(maxsize=None)
def model(which):
    """The float64 model of every image of a case list from the host decoder's coefficients, computed once."""
    out = []
    for _, d, _ in (CASES if which == "full" else resize_cases()):
        h, c = jpeg.entropy_decode(d, **AUTO)
        rgb = jpeg.reference_backend(h, c)
        out.append(jpeg.reference_resize_crop(rgb) if which == "resize" else rgb)
    return tuple(out)


def _assert_same_coefs(datas, form, want, **kw):
    hs, ho, hc = want
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on=form, **AUTO, **kw)
    assert gs == hs and go == ho and gc.dtype == torch.int16 and gc.shape == hc.shape
    for i, d in enumerate(datas):
        if hs[i] == 0:
            n = jpeg.parse(d, **AUTO)["total_coefs"]
            assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), f"{form}: image {i}: coefficients differ"
    return gs


@pytest.mark.parametrize("form", FORMS)
def test_coefficients_of_the_whole_batch_equal_the_host_decoders(form):
    datas = [c[1] for c in CASES]
    assert host_coefs()[0] == [0] * len(datas)
    if form != "host":
        par = form == "gpu_parallel"
        pk = ops.jpeg_huff_pack(datas, par, True, False, False, True)
        assert pk.native_colorspace is True and pk.status == [0] * len(datas) and pk.n_prog == len(progressive_cases())
        cs = pk.hdr.numpy().view(np.int32)[:, ops.JPEG_HEADER_COLORSPACE_OFFSET // 4].tolist()
        assert cs == [c[2] for c in CASES]
        nrst = sum(1 for n in NAMES[:NF] if "rst" in n)
        nfour = sum(1 for i in FOUR if i < NF)
        rgb_rst = sum(1 for n in NAMES[:NF] if "rst" in n and n.startswith("rgb"))
        # four-component files and files with restart markers on one lane each, the rest laid out for the form
        lane = nfour + rgb_rst if par else NF
        assert (pk.n_lane, pk.n_par, pk.n_rst) == (lane, NF - lane if par else 0, 0)
        pk = ops.jpeg_huff_pack(datas, par, True, True, False, True)
        assert pk.n_rst == rgb_rst                          # intervals: for the RGB-coded file only
    assert _assert_same_coefs(datas, form, host_coefs()) == [0] * len(datas)
    assert _assert_same_coefs(datas, form, host_coefs(), restart="intervals") == [0] * len(datas)
    # without the keyword the four-component files are refused by the parse, the rest is decoded as before
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on=form, progressive="native")
    hs, ho, hc = host_coefs()
    assert gs == [7 if i in FOUR else 0 for i in range(len(datas))]
    for i, d in enumerate(datas):
        if gs[i] == 0:
            n = jpeg.parse(d, progressive="native")["total_coefs"]
            assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), (form, i)


@pytest.mark.parametrize("form", DEVICE_FORMS)
def test_coefficients_in_batches_of_one(form):
    hs, ho, hc = host_coefs()
    for i, (name, d, _) in enumerate(CASES):
        n = jpeg.parse(d, **AUTO)["total_coefs"]
        for kw in ({}, {"restart": "intervals"}) if "rst" in name else ({},):
            gs, go, gc = jpeg.entropy_coefs([d], DEV, entropy_on=form, **AUTO, **kw)
            assert gs == [0] and go == [0] and gc.numel() == n, (name, gs)
            assert torch.equal(gc, hc[ho[i]:ho[i] + n]), f"{form}: {name} alone: coefficients differ"
    assert jpeg.entropy_coefs([CASES[FOUR[0]][1]], DEV, entropy_on=form)[0] == [7]


def test_pixels_at_full_resolution_in_every_form():
    want = model("full")
    datas = [c[1] for c in CASES]
    outs = []
    for form in FORMS:
        imgs, info = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=form, **AUTO)
        assert info["fallbacks"] == [] and info["colorspace"] == "auto" and info["entropy_on"] == form
        assert info["colorspace_images"] == NCOLOR and info["gpu_images"] == len(datas)
        assert info["progressive_images"] == len(progressive_cases())
        outs.append(imgs)
    worst = {}
    for k, (name, d, cs) in enumerate(CASES):
        got = outs[0][k].cpu().numpy()
        ref = pil_rgb(d)
        assert got.shape == ref.shape, name
        mx, mean = diff_stats(got, ref)
        mm, _ = diff_stats(got, want[k])
        print(name, KIND[cs], "vs Pillow", mx, round(mean, 4), "vs model", mm)
        worst[KIND[cs]] = max(worst.get(KIND[cs], 0), mm)
        assert mm <= MAX_GPU_MODEL[cs], (name, mm)
        assert mx <= MAX_PIL[cs] + MAX_GPU_MODEL[cs] and mean <= MEAN_PIL[cs], (name, mx, mean)
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), name
    print("largest difference from the model per colour space:", worst)
    # restart="intervals" changes nothing of the pixels, and alone an image is what it is in the batch
    imgs, info = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on="gpu", restart="intervals", **AUTO)
    assert info["fallbacks"] == [] and info["restart_images"] == 1
    assert all(torch.equal(a, b) for a, b in zip(imgs, outs[0]))
    for name in ("cmyk-2x33-q50", "ycck-67x45-q95", "rgb420-2x33-q95", "rgb422-40x3-q50", "cmyk-noadobe-17x9-q50",
                 "p-ycck-67x45"):
        k = NAMES.index(name)
        alone, _ = jpeg.decode_batch([datas[k]], DEV, resize=None, crop=None, **AUTO)
        assert torch.equal(alone[0], outs[0][k]), name


@functools.lru_cache(maxsize=None)
def resized():
    """The resize cases through Resize(256) + CenterCrop(224) in one batch, per form, computed once."""
    datas = [c[1] for c in resize_cases()]
    outs = []
    for form in FORMS:
        imgs, info = jpeg.decode_batch(datas, DEV, entropy_on=form, colorspace="auto")
        assert info["fallbacks"] == [] and info["colorspace_images"] == len(datas) == info["gpu_images"]
        assert imgs.shape == (len(datas), 224, 224, 3)
        outs.append(imgs)
    return tuple(outs)


def test_resize_and_crop_batched_and_alone():
    outs = resized()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for k, (name, d, cs) in enumerate(resize_cases()):
        mx, mean = diff_stats(outs[0][k].cpu().numpy(), load_image_u8(d))
        print(name, "vs load_image_u8", mx, round(mean, 4))
        assert mx <= MAX_PIL[cs] + MAX_GPU_MODEL[cs] and mean <= MEAN_PIL[cs], (name, mx, mean)
        alone, _ = jpeg.decode_batch([d], DEV, colorspace="auto")
        assert torch.equal(alone[0], outs[0][k]), name


@pytest.mark.parametrize("name", [c[0] for c in resize_cases()])
def test_resize_and_crop_against_the_model(name):
    k = [c[0] for c in resize_cases()].index(name)
    cs = resize_cases()[k][2]
    mm, _ = diff_stats(resized()[0][k].cpu().numpy(), model("resize")[k])
    print(name, "vs model", mm)
    assert mm <= MAX_GPU_MODEL[cs], (name, mm)


@functools.lru_cache(maxsize=None)
def mixed():
    """An ordinary YCbCr file, a grey one, the three new kinds, a None, the subsampled-CMYK refusal, a PNG."""
    named = {c[0]: c[1] for c in full_res_cases()}
    return (encode(70, 46, "420", 75, seed=1), encode(67, 45, "grey", 75, seed=4), named["rgb420-67x45-q50"],
            named["cmyk-67x45-q95"], named["ycck-17x9-q50"], None, refusals()[0][1], png())


@pytest.mark.parametrize("form", FORMS)
def test_mixed_batch_with_and_without_the_keyword(form):
    datas = list(mixed())
    for full in (True, False):
        size = dict(resize=None, crop=None) if full else {}
        host = pil_rgb if full else load_image_u8
        nat, ninfo = jpeg.decode_batch(datas, DEV, entropy_on=form, colorspace="auto", **size)
        assert ninfo["fallbacks"] == [(6, "sampling"), (7, "not_jpeg")]
        assert ninfo["colorspace"] == "auto" and ninfo["colorspace_images"] == 3 and ninfo["gpu_images"] == 5
        for i in (2, 3, 4):
            cs = jpeg.parse(datas[i], colorspace="auto")["colorspace"]
            mx, mean = diff_stats(nat[i].cpu().numpy(), host(datas[i]))
            assert mx <= MAX_PIL[cs] + MAX_GPU_MODEL[cs] and mean <= MEAN_PIL[cs], (i, mx, mean)
        for i in (6, 7):
            assert np.array_equal(nat[i].cpu().numpy(), host(datas[i]))
        # the ordinary files alone under the default: what every batch must give for them
        alone, ainfo = jpeg.decode_batch(datas[:2], DEV, entropy_on=form, **size)
        assert ainfo["fallbacks"] == [] and ainfo["colorspace"] == "ycbcr" and ainfo["colorspace_images"] == 0
        for kw in ({}, {"colorspace": "ycbcr"}):
            imgs, info = jpeg.decode_batch(datas, DEV, entropy_on=form, **kw, **size)
            assert info["fallbacks"] == [(3, "components"), (4, "components"), (6, "components"), (7, "not_jpeg")]
            assert info["colorspace"] == "ycbcr" and info["colorspace_images"] == 0 and info["gpu_images"] == 3
            for i in (3, 4, 6, 7):
                assert np.array_equal(imgs[i].cpu().numpy(), host(datas[i]))
            for i in (0, 1):
                assert torch.equal(imgs[i], alone[i]) and torch.equal(imgs[i], nat[i])
            # the RGB-coded file under the default: decoded as YCbCr, no fallback, other pixels than under "auto"
            assert not torch.equal(imgs[2], nat[2])
        if full:
            assert nat[5] is None and imgs[5] is None
        else:
            assert not nat[5].any() and not imgs[5].any()


def test_the_plan_counts_the_colour_space_images_into_the_fp64_pass():
    datas = list(mixed())
    st, hdr, coefs, offs = ops.jpeg_entropy_batch(datas, 2, False, False, True)
    assert list(st) == [0, 0, 0, 0, 0, 1, 9, 2]
    plan = ops.jpeg_plan(hdr, list(st), offs, coefs.numel(), None, 0, DEV)
    assert plan.n_gpu == 5 and plan.n_exact == 3 and plan.n_color == 3
    st, hdr, coefs, offs = ops.jpeg_entropy_batch(datas, 2)                        # the default
    assert list(st) == [0, 0, 0, 7, 7, 1, 7, 2]
    plan = ops.jpeg_plan(hdr, list(st), offs, coefs.numel(), None, 0, DEV)
    assert plan.n_gpu == 3 and plan.n_exact == 0 and plan.n_color == 0


@pytest.mark.parametrize("form", FORMS)
def test_a_prepared_entropy_stage_decides_the_mode(form):
    datas = [c[1] for c in resize_cases()]
    want = resized()[0]
    ent = jpeg.entropy_batch(datas, 2, form, colorspace="auto")
    imgs, info = jpeg.decode_batch(datas, DEV, entropy=ent)                       # asked for the default, prepared auto
    assert info["colorspace"] == "auto" and info["fallbacks"] == [] and info["colorspace_images"] == len(datas)
    assert info["entropy_on"] == form and torch.equal(imgs, want)
    ent = jpeg.entropy_batch(datas, 2, form)                                      # and the other way round
    imgs, info = jpeg.decode_batch(datas, DEV, entropy=ent, colorspace="auto")
    assert info["colorspace"] == "ycbcr" and info["colorspace_images"] == 0
    assert info["fallbacks"] == [(0, "components"), (1, "components")]


def _directory(tmp_path):
    """One file of each kind: CMYK, YCCK, two subsampled RGB ones, an ordinary YCbCr one."""
    datas = [c[1] for c in resize_cases()] + [plain_resize_cases()[0][1]]
    for i, d in enumerate(datas):
        (tmp_path / f"test_{i}.JPEG").write_bytes(d)
    return datas, [c[2] for c in resize_cases()] + [YCBCR]


@pytest.mark.parametrize("form", FORMS)
def test_gpu_jpeg_source_counts_the_native_images(tmp_path, form):
    datas, css = _directory(tmp_path)
    n = len(datas)
    src = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=form, colorspace="auto")
    rows = src.get(0, n - 1)
    assert src.decoded == n and src.fallbacks == 0 and src.colorspace_images == n - 1 and src.colorspace == "auto"
    assert torch.equal(rows[:n - 1], resized()[0])
    for i, (d, cs) in enumerate(zip(datas, css)):
        mx, mean = diff_stats(rows[i].cpu().numpy(), load_image_u8(d))
        assert mx <= MAX_PIL[cs] + MAX_GPU_MODEL[cs] and mean <= MEAN_PIL[cs], (i, mx, mean)
    src.CHUNK = src.CHUNK_GPU = src.CHUNK_GPU_PARALLEL = 2       # more than one chunk: the prepare-ahead thread
    src.invalidate()
    assert torch.equal(src.get(0, n - 1), rows) and src.fallbacks == 0 and src.colorspace_images == 2 * (n - 1)
    old = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=form)        # the default: four components through Pillow
    orows = old.get(0, n - 1)
    assert old.fallbacks == 2 and old.colorspace_images == 0 and old.colorspace == "ycbcr"
    assert old.fallback_reasons == {0: "components", 1: "components"}
    assert torch.equal(orows[n - 1], rows[n - 1])
    for i in (0, 1):
        assert np.array_equal(orows[i].cpu().numpy(), load_image_u8(datas[i]))


def test_deeplearning_takes_the_keyword(tmp_path):
    from idunno import inference

    d = tmp_path / "resnet18"
    d.mkdir()
    datas, _ = _directory(d)
    n = len(datas)
    inference.drop_gpu_sources()
    try:
        pil, _ = inference.deeplearning("resnet18", "resnet18", 0, n - 1, device=DEV, root=str(tmp_path), topk=2)
        gpu, _ = inference.deeplearning("resnet18", "resnet18", 0, n - 1, device=DEV, root=str(tmp_path), topk=2,
                                        decoder="gpu", colorspace="auto")
        srcs = [s for s in inference._GPU_SOURCES.values() if s.colorspace == "auto"]
        assert len(srcs) == 1 and srcs[0].fallbacks == 0 and srcs[0].colorspace_images == n - 1 and srcs[0].decoded == n
        inference.deeplearning("resnet18", "resnet18", 0, n - 1, device=DEV, root=str(tmp_path), topk=2, decoder="gpu")
        assert len(inference._GPU_SOURCES) == 2                  # the keyword is part of the key
        srcs = [s for s in inference._GPU_SOURCES.values() if s.colorspace == "ycbcr"]
        assert len(srcs) == 1 and srcs[0].fallbacks == 2 and srcs[0].colorspace_images == 0
    finally:
        inference.drop_gpu_sources()
    # the decoders differ by a few levels in single pixels and MEAN_BOUND on average (5e-4 of the range), which
    # moves no probability by a twentieth of itself: wherever the Pillow run's two best classes are further apart
    # than that, both runs name the same best class
    assert [r[0] for r in gpu] == [r[0] for r in pil]
    for i, (_, _, p) in enumerate(pil):
        if p[0] - p[1] > 0.05 * p[0]:
            assert gpu[i][1][0] == pil[i][1][0], (i, gpu[i], pil[i])
