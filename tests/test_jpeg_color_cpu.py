"""``colorspace="auto"`` without a GPU: the classification of RGB-coded, CMYK and YCCK
files (tests/jpeg_color_cases.py) by the header parse, the unchanged default, the host
decoder and the float64 model against Pillow on the very same bytes, refusals, and the
option's validation and CPU-device behaviour everywhere it is accepted."""
import inspect
import io

import numpy as np
import pytest
import torch
from jpeg_cases import diff_stats, encode, pil_rgb
from jpeg_color_cases import (CMYK, KIND, MAX_PIL, MEAN_PIL, NEW_KINDS, RGB, YCBCR, YCBCR_KINDS, YCCK, add_adobe, cut,
                              full_res_cases, jfif_to_adobe, make, progressive_cases, refusals, resize_cases, rgb_ids,
                              set_transform)
from PIL import Image

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import load_image_u8

FULL = {c[0]: c for c in full_res_cases()}
PROG = {c[0]: c for c in progressive_cases()}
RESIZE = {c[0]: c for c in resize_cases()}


def test_every_recipe_is_classified_as_libjpeg_classifies_it():
    for kind in NEW_KINDS + YCBCR_KINDS:
        d, cs = make(kind, 38, 30, 75, seed=3, smooth=True)
        h = jpeg.parse(d, colorspace="auto")
        assert isinstance(h, dict) and h["colorspace"] == cs, (kind, h)
        assert h["ncomp"] == (4 if cs in (CMYK, YCCK) else 3)
    # the rules on rewritten files of every layout: JFIF wins, then Adobe, then the ids
    for sub in ("444", "422", "420"):
        src = encode(38, 30, sub, 75, seed=4, smooth=True)
        want = {YCBCR: [src, rgb_ids(src), add_adobe(src, 0), jfif_to_adobe(src, 1), cut(src, 0xE0)],
                RGB: [jfif_to_adobe(src, 0), rgb_ids(cut(src, 0xE0)), rgb_ids(jfif_to_adobe(src, 0))]}
        for cs, files in want.items():
            for k, d in enumerate(files):
                assert jpeg.parse(d, colorspace="auto")["colorspace"] == cs, (sub, cs, k)
    for name, d, cs in full_res_cases() + resize_cases() + tuple(c[:3] for c in progressive_cases()):
        h = jpeg.parse(d, progressive="native", colorspace="auto")
        assert isinstance(h, dict) and h["colorspace"] == cs, (name, h)
        # Pillow sees the same number of components: its mode follows libjpeg's out_color_space
        assert Image.open(io.BytesIO(d)).mode == ("CMYK" if cs in (CMYK, YCCK) else "RGB"), name
    grey = encode(17, 9, "grey", 75, seed=1)
    assert jpeg.parse(grey, colorspace="auto") == dict(jpeg.parse(grey), colorspace=0)


def test_four_component_header_has_four_full_size_planes():
    h = jpeg.parse(FULL["cmyk-67x45-q50"][1], colorspace="auto")
    assert (h["W"], h["H"], h["ncomp"], h["mode"], h["hmax"], h["vmax"]) == (67, 45, 4, 0, 1, 1)
    assert [(c["h"], c["v"], c["bw"], c["bh"]) for c in h["comp"]] == [(1, 1, 9, 6)] * 4
    assert [c["coef_off"] for c in h["comp"]] == [0, 54 * 64, 108 * 64, 162 * 64] and h["total_coefs"] == 216 * 64


def test_rgb_kinds_are_the_same_pixels_to_pillow_whatever_says_so():
    # RGB ids without any marker give the pixels of Adobe transform 0 on the same scan
    src = encode(38, 30, "420", 75, seed=11, smooth=True)
    assert np.array_equal(pil_rgb(rgb_ids(cut(src, 0xE0))), pil_rgb(jfif_to_adobe(src)))
    assert not np.array_equal(pil_rgb(jfif_to_adobe(src)), pil_rgb(src))
    # and the files that stay YCbCr give the pixels of the ordinary file
    for d in (rgb_ids(src), add_adobe(src, 0), jfif_to_adobe(src, 1), cut(src, 0xE0)):
        assert np.array_equal(pil_rgb(d), pil_rgb(src))


def test_default_is_unchanged():
    for name, d, cs in full_res_cases():
        got = jpeg.parse(d)
        assert got == jpeg.parse(d, colorspace="ycbcr"), name
        if cs in (CMYK, YCCK):
            assert got == "components", name
            assert jpeg.entropy_decode(d) == "components"
        else:
            assert got["colorspace"] == 0, name                # an RGB-coded file counts as YCbCr
            auto = jpeg.parse(d, colorspace="auto")
            assert {k: v for k, v in auto.items() if k != "colorspace"} == {k: v for k, v in got.items() if k != "colorspace"}
    d = FULL["cmyk-8x8-q50"][1]
    assert jpeg.entropy_coefs([d])[0] == [7] and ops.jpeg_parse(d)[:2] == (7, "components")
    assert ops.jpeg_huff_pack([d]).status == [7] and ops.jpeg_huff_pack([d]).native_colorspace is False
    # the model under a default header: the YCbCr matrix, as the kernels apply it
    d = FULL["rgb444-17x9-q95"][1]
    h0, c0 = jpeg.entropy_decode(d)
    h1, c1 = jpeg.entropy_decode(d, colorspace="auto")
    assert np.array_equal(c0, c1)
    assert not np.array_equal(jpeg.reference_backend(h0, c0), jpeg.reference_backend(h1, c1))
    assert np.array_equal(jpeg.reference_backend(h0, c0), jpeg.reference_backend(dict(h1, colorspace=0), c1))


def test_refusals():
    for name, d, reason in refusals():
        assert jpeg.parse(d, colorspace="auto") == reason, name
        assert jpeg.entropy_decode(d, colorspace="auto") == reason, name
        assert jpeg.parse(d) == "components", name
    d = FULL["cmyk-17x9-q50"][1]
    for t in (1, 3, 255):
        assert jpeg.parse(set_transform(d, t), colorspace="auto") == "components"
    two = bytearray(encode(17, 9, "444", 75, seed=2))
    at = two.index(b"\xff\xc0")
    two[at + 9] = 2                                        # two components: the frame header no longer fits its length
    assert jpeg.parse(bytes(two), colorspace="auto") in ("components", "corrupt")
    # a progressive four-component file needs progressive="native" as well
    assert jpeg.parse(progressive_cases()[0][1], colorspace="auto") == "progressive"


def test_unknown_value_is_refused_everywhere():
    from idunno import inference
    from idunno.runtime.data import GpuJpegSource

    d = FULL["cmyk-8x8-q50"][1]
    for bad in ("Auto", "", "rgb", None, True):
        for call in (lambda: jpeg.parse(d, colorspace=bad), lambda: jpeg.entropy_decode(d, colorspace=bad),
                     lambda: jpeg.entropy_batch([d], 1, colorspace=bad),
                     lambda: jpeg.entropy_coefs([d], colorspace=bad),
                     lambda: jpeg.decode_batch([d], "cpu", colorspace=bad),
                     lambda: GpuJpegSource("cpu", root=".", colorspace=bad),
                     lambda: inference.deeplearning("alexnet", "alexnet", 0, 0, device="cpu", colorspace=bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(SystemExit):
        inference.main(["alexnet", "0", "0", "--colorspace", "yes"])
    for fn in (jpeg.parse, jpeg.entropy_decode, jpeg.entropy_batch, jpeg.entropy_coefs, jpeg.decode_batch):
        assert inspect.signature(fn).parameters["colorspace"].default == "ycbcr", fn.__name__


def test_ycck_and_cmyk_twins_hold_the_same_coefficients():
    for name in ("cmyk-67x45-q50", "cmyk-17x9-q95", "cmyk-67x45-rst2"):
        d = FULL[name][1]
        hc, cc = jpeg.entropy_decode(d, colorspace="auto")
        hy, cy = jpeg.entropy_decode(set_transform(d, 2), colorspace="auto")
        assert (hc["colorspace"], hy["colorspace"]) == (CMYK, YCCK) and np.array_equal(cc, cy)
        assert dict(hc, colorspace=0) == dict(hy, colorspace=0)


@pytest.mark.parametrize("name", list(PROG))
def test_progressive_equals_baseline(name):
    _, prog, cs, base = PROG[name]
    assert jpeg.entropy_decode(prog, colorspace="auto") == "progressive"
    hp, cp = jpeg.entropy_decode(prog, progressive="native", colorspace="auto")
    hb, cb = jpeg.entropy_decode(base, colorspace="auto")
    assert hp["progressive"] is True and hb["progressive"] is False and hp["colorspace"] == hb["colorspace"] == cs
    assert hp["nscans"] > 1 and hb["nscans"] == 1
    # Pillow's files are twins: the same quantised coefficients, spread over scans
    assert np.array_equal(pil_rgb(prog), pil_rgb(base)), name
    assert np.array_equal(cp, cb), name
    mx, mean = diff_stats(jpeg.reference_backend(hp, cp), pil_rgb(prog))
    print(name, KIND[cs], mx, mean)
    assert mx <= MAX_PIL[cs] and mean <= MEAN_PIL[cs]


@pytest.mark.parametrize("name", list(FULL))
def test_model_against_pillow_at_full_resolution(name):
    _, d, cs = FULL[name]
    h, c = jpeg.entropy_decode(d, colorspace="auto")
    assert c.dtype == np.int16 and h["colorspace"] == cs
    got, want = jpeg.reference_backend(h, c), pil_rgb(d)
    assert got.shape == want.shape == (h["H"], h["W"], 3)
    mx, mean = diff_stats(got, want)
    print(name, KIND[cs], mx, mean)
    assert mx <= MAX_PIL[cs] and mean <= MEAN_PIL[cs]


@pytest.mark.parametrize("name", list(RESIZE))
def test_model_against_load_image_u8_after_resize_and_crop(name):
    _, d, cs = RESIZE[name]
    h, c = jpeg.entropy_decode(d, colorspace="auto")
    full = jpeg.reference_backend(h, c)
    mx, mean = diff_stats(full, pil_rgb(d))
    print(name, KIND[cs], "full", mx, mean)
    assert mx <= MAX_PIL[cs] and mean <= MEAN_PIL[cs]
    mx, mean = diff_stats(jpeg.reference_resize_crop(full), load_image_u8(d))
    print(name, KIND[cs], "resized", mx, mean)
    assert mx <= MAX_PIL[cs] and mean <= MEAN_PIL[cs]


def test_the_bounds_of_the_cmyk_formula_are_what_an_exhaustive_search_gives():
    c, nk = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    t = c * nk + 128
    assert np.array_equal(((t >> 8) + t) >> 8, np.floor(c * nk / 255 + 0.5).astype(np.int64))   # MULDIV255: round half up
    assert np.array_equal(jpeg._muldiv255(c, nk), ((t >> 8) + t) >> 8)

    def f(a, b):
        return b - jpeg._muldiv255(a, b)

    def worst(dc):
        w = 0
        for da in range(-dc, dc + 1):
            for db in (-1, 0, 1):
                a2, b2 = np.clip(c + da, 0, 255), np.clip(nk + db, 0, 255)
                ok = (a2 == c + da) & (b2 == nk + db)
                w = max(w, int(np.abs(f(a2, b2) - f(c, nk))[ok].max()))
        return w

    assert worst(1) == MAX_PIL[CMYK] == 2 and worst(3) == MAX_PIL[YCCK] == 4


def test_host_batch_and_coefs_take_the_keyword():
    ds = [FULL["cmyk-17x9-q95"][1], encode(17, 9, "420", 75, seed=1), None, FULL["rgb-ids-2x33-q50"][1],
          FULL["ycck-40x3-rst2"][1]]
    st, offs, coefs = jpeg.entropy_coefs(ds, colorspace="auto")
    assert st == [0, 0, 1, 0, 0] and offs[2] == -1
    for i in (0, 1, 3, 4):
        h, c = jpeg.entropy_decode(ds[i], colorspace="auto")
        assert np.array_equal(coefs[offs[i]:offs[i] + h["total_coefs"]].numpy(), c)
    assert jpeg.entropy_coefs(ds)[0] == [7, 0, 1, 0, 7]
    ent = jpeg.entropy_batch(ds, 2, colorspace="auto")
    assert list(ent.status) == [0, 0, 1, 0, 0] and ent.options.sampling == "fallback" and ent.options.colorspace == "auto"
    assert list(jpeg.entropy_batch(ds, 2).status) == [7, 0, 1, 0, 7] and jpeg.entropy_batch(ds, 2).options.colorspace == "ycbcr"
    cs = ent.hdr.numpy().view(np.int32)[:, ops.JPEG_HEADER_COLORSPACE_OFFSET // 4].tolist()
    assert cs == [CMYK, YCBCR, 0, RGB, YCCK]


def test_bindings_take_the_flag_last_and_the_packer_keeps_four_components_off_two_kernels():
    d = FULL["cmyk-67x45-q50"][1]
    rst = FULL["cmyk-67x45-rst2"][1]
    rgb = FULL["rgb420-67x45-rst2"][1]
    C = ops.load()
    assert C.jpeg_parse(d)[:2] == (7, "components") and C.jpeg_parse(d, False, False, False)[:2] == (7, "components")
    st, reason, h = C.jpeg_parse(d, False, False, True)
    assert (st, reason, h["colorspace"], h["ncomp"]) == (0, "ok", CMYK, 4)
    assert ops.jpeg_parse(d, native_colorspace=True)[0] == 0 and C.jpeg_parse(d, native_colorspace=True)[0] == 0
    assert list(ops.jpeg_entropy_batch([d], 1, False, False, True)[0]) == [0]
    assert list(ops.jpeg_entropy_batch([d], 1)[0]) == [7]
    # a four-component file takes the one-lane kernel in every layout, an RGB-coded one goes with its YCbCr twins
    for parallel in (False, True):
        for intervals in (False, True):
            pk = ops.jpeg_huff_pack([d, rst, rgb], parallel, False, intervals, False, True)
            assert pk.status == [0, 0, 0] and pk.native_colorspace is True
            # both CMYK files on one lane each, whatever the layout; only the RGB-coded file gets intervals
            assert (pk.n_lane, pk.n_par, pk.n_rst) == (3 - intervals, 0, int(intervals)), (parallel, intervals)
    pk = ops.jpeg_huff_pack([d, FULL["rgb420-67x45-q50"][1]], True, False, False, False, True)
    assert (pk.n_lane, pk.n_par) == (1, 1)
    pk = ops.jpeg_huff_pack([progressive_cases()[0][1]], True, True, True, False, True)
    assert (pk.n_prog, pk.n_lane, pk.status) == (1, 0, [0])
    # the header rows keep the layout of everything that was there
    assert ops.JPEG_HEADER_MODE_OFFSET == 20 and ops.JPEG_HEADER_PROGRESSIVE_OFFSET == 500
    assert ops.JPEG_HEADER_COLORSPACE_OFFSET == 508


def test_cpu_device_runs_nothing_native(tmp_path):
    from idunno import inference
    from idunno.runtime.data import GpuJpegSource

    datas = [RESIZE["cmyk-333x250"][1], RESIZE["rgb420-333x250"][1], None, FULL["ycck-67x45-q50"][1]]
    imgs, info = jpeg.decode_batch(datas, "cpu", colorspace="auto")
    assert info["colorspace"] == "auto" and info["colorspace_images"] == 0
    assert info["fallbacks"] == [(0, "cpu_device"), (1, "cpu_device"), (3, "cpu_device")]
    for i in (0, 1, 3):
        assert np.array_equal(imgs[i].numpy(), load_image_u8(datas[i]))
    base, binfo = jpeg.decode_batch(datas, "cpu")
    assert binfo["colorspace"] == "ycbcr" and binfo["colorspace_images"] == 0 and torch.equal(base, imgs)
    for i in range(2):
        (tmp_path / f"test_{i}.JPEG").write_bytes(datas[i])
    src = GpuJpegSource("cpu", root=str(tmp_path), colorspace="auto")
    assert src.colorspace == "auto" and torch.equal(src.get(0, 1), imgs[:2])
    assert src.colorspace_images == 0 and src.fallbacks == 2
    assert GpuJpegSource("cpu", root=str(tmp_path)).colorspace == "ycbcr"
    res, _ = inference.deeplearning(str(tmp_path), "alexnet", 0, 1, device="cpu", decoder="gpu", colorspace="auto")
    assert [r[0] for r in res] == ["test_0.JPEG", "test_1.JPEG"]
    inference.drop_gpu_sources()


def test_command_lines_pass_the_mode_on(monkeypatch):
    from idunno import inference, launch

    seen = []

    def fake(filename, modelname, start, end, **kw):
        seen.append(kw["colorspace"])
        return [], 0.0

    monkeypatch.setattr(inference, "deeplearning", fake)
    assert inference.main(["alexnet", "0", "0", "--decoder", "gpu", "--colorspace", "auto"]) == 0
    assert inference.main(["alexnet", "0", "0"]) == 0
    assert seen == ["auto", "ycbcr"]
    a = launch.build_parser().parse_args(["node", "--jpeg-colorspace", "auto"])
    assert a.jpeg_colorspace == "auto" and launch.build_parser().parse_args(["node"]).jpeg_colorspace == "ycbcr"
    src = inspect.getsource(launch)
    assert '"--jpeg-colorspace", a.jpeg_colorspace' in src and "colorspace=a.jpeg_colorspace" in src


def test_docstrings_say_what_the_default_does_with_rgb_coded_files():
    for doc in (jpeg.__doc__, jpeg.parse.__doc__, jpeg.decode_batch.__doc__, jpeg.entropy_batch.__doc__):
        flat = " ".join(doc.split())
        assert "RGB-coded" in flat and "YCbCr" in flat
    assert "decoded as YCbCr" in " ".join(jpeg.decode_batch.__doc__.split())
