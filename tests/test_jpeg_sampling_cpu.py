"""``sampling="native"`` without a GPU: the header parse of 4:4:0 and 4:1:1 files
(tests/jpeg_sampling_cases.py), the host decoder and the float64 model against
Pillow on the very same bytes, refusals, and the option's validation and
CPU-device behaviour everywhere it is accepted."""
import inspect

import numpy as np
import pytest
import torch
from jpeg_cases import MAX_MODEL, MEAN_BOUND, diff_stats, encode, pil_rgb
from jpeg_sampling_cases import full_res_cases, make_h1v4, named, progressive_cases, resize_cases, rewrite

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import load_image_u8


def test_native_parse_gives_the_modes_and_grids():
    h = jpeg.parse(named("440-70x46-q50")[1], sampling="native")
    assert (h["W"], h["H"], h["mode"], h["hmax"], h["vmax"]) == (70, 46, 3, 1, 2)
    assert [(c["h"], c["v"], c["bw"], c["bh"]) for c in h["comp"]] == [(1, 2, 9, 6), (1, 1, 9, 3), (1, 1, 9, 3)]
    assert [c["coef_off"] for c in h["comp"]] == [0, 54 * 64, 81 * 64] and h["total_coefs"] == 108 * 64
    h = jpeg.parse(named("411-128x24-q50")[1], sampling="native")
    assert (h["W"], h["H"], h["mode"], h["hmax"], h["vmax"]) == (128, 24, 4, 4, 1)
    assert [(c["h"], c["v"], c["bw"], c["bh"]) for c in h["comp"]] == [(4, 1, 16, 3), (1, 1, 4, 3), (1, 1, 4, 3)]
    assert [c["coef_off"] for c in h["comp"]] == [0, 48 * 64, 60 * 64] and h["total_coefs"] == 72 * 64
    for name, d, mode in full_res_cases() + resize_cases() + progressive_cases():
        hd = jpeg.parse(d, progressive="native", sampling="native")
        assert isinstance(hd, dict) and hd["mode"] == mode, (name, hd)


def test_default_still_refuses_both_layouts():
    for name, d, _ in full_res_cases():
        assert jpeg.parse(d) == "sampling" and jpeg.parse(d, sampling="fallback") == "sampling", name
    d = named("440-70x46-q50")[1]
    assert jpeg.entropy_decode(d) == "sampling"
    assert jpeg.entropy_coefs([d])[0] == [9]
    assert jpeg.parse(progressive_cases()[0][1], progressive="native") == "sampling"


def test_other_layouts_stay_refused_in_both_modes():
    src = encode(64, 48, "420", 80, seed=5, smooth=True)
    odd = [make_h1v4(64, 48),                       # luma 1x4
           rewrite(src, 0x42, 64, 48),              # luma 4x2
           rewrite(src, 0x24, 64, 48),              # luma 2x4
           rewrite(src, 0x31, 64, 48),              # luma 3x1
           rewrite(src, 0x32, 64, 48)]              # luma 3x2
    chroma = bytearray(rewrite(src, 0x41, 128, 24))
    at = chroma.index(b"\xff\xc0")
    chroma[at + 14] = 0x21                          # Cb 2x1 under luma 4x1
    differ = bytearray(rewrite(src, 0x12, 64, 48))
    differ[at + 17] = 0x12                          # Cr 1x2, Cb 1x1
    for d in odd + [bytes(chroma), bytes(differ)]:
        assert jpeg.parse(d) == "sampling" and jpeg.parse(d, sampling="native") == "sampling"
        assert jpeg.entropy_decode(d, sampling="native") == "sampling"
    # the three layouts of before are what they were, whatever the mode
    for sub, mode in (("444", 0), ("422", 1), ("420", 2)):
        d = encode(38, 30, sub, 75, seed=3)
        assert jpeg.parse(d)["mode"] == mode and jpeg.parse(d, sampling="native") == jpeg.parse(d)


@pytest.mark.parametrize("name", [c[0] for c in full_res_cases()])
def test_model_against_pillow_at_full_resolution(name):
    _, d, mode = named(name)
    h, c = jpeg.entropy_decode(d, sampling="native")
    assert c.dtype == np.int16 and h["mode"] == mode
    got, want = jpeg.reference_backend(h, c), pil_rgb(d)
    assert got.shape == want.shape == (h["H"], h["W"], 3)
    mx, mean = diff_stats(got, want)
    print(name, mx, mean)
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


@pytest.mark.parametrize("name", [c[0] for c in resize_cases()])
def test_model_against_load_image_u8_after_resize_and_crop(name):
    _, d, _ = next(c for c in resize_cases() if c[0] == name)
    h, c = jpeg.entropy_decode(d, sampling="native")
    mx, mean = diff_stats(jpeg.reference_resize_crop(jpeg.reference_backend(h, c)), load_image_u8(d))
    print(name, mx, mean)
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


@pytest.mark.parametrize("name", [c[0] for c in progressive_cases()])
def test_progressive_files_decode_to_the_model_bound(name):
    _, d, mode = next(c for c in progressive_cases() if c[0] == name)
    assert jpeg.entropy_decode(d, sampling="native") == "progressive"
    h, c = jpeg.entropy_decode(d, progressive="native", sampling="native")
    assert h["progressive"] is True and h["nscans"] == 10 and h["mode"] == mode
    mx, mean = diff_stats(jpeg.reference_backend(h, c), pil_rgb(d))
    print(name, mx, mean)
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


def test_upsample_h1v2_is_libjpegs_vertical_triangle_filter():
    p = np.array([[10, 200], [50, 100], [90, 0]], np.uint8)
    want = np.array([[10, 200], [20, 175], [40, 125], [60, 75], [80, 25], [90, 0]])
    #  even rows (3p + above + 1) >> 2, odd rows (3p + below + 2) >> 2, the neighbour clamped at both ends
    assert np.array_equal(jpeg._upsample_h1v2(p), want)


def test_host_batch_and_coefs_take_the_keyword():
    ds = [named("440-17x9-q95")[1], encode(17, 9, "420", 75, seed=1), None, named("411-59x5-q50")[1]]
    st, offs, coefs = jpeg.entropy_coefs(ds, sampling="native")
    assert st == [0, 0, 1, 0] and offs[2] == -1
    for i in (0, 1, 3):
        h, c = jpeg.entropy_decode(ds[i], sampling="native")
        assert np.array_equal(coefs[offs[i]:offs[i] + h["total_coefs"]].numpy(), c)
    assert jpeg.entropy_coefs(ds)[0] == [9, 0, 1, 9]
    ent = jpeg.entropy_batch(ds, 2, sampling="native")
    assert list(ent.status) == [0, 0, 1, 0] and ent.options.sampling == "native"
    assert list(jpeg.entropy_batch(ds, 2).status) == [9, 0, 1, 9]


def test_cpu_device_runs_nothing_native(tmp_path):
    from idunno.runtime.data import GpuJpegSource

    datas = [resize_cases()[0][1], resize_cases()[2][1], None, named("440-70x46-rst2")[1]]
    imgs, info = jpeg.decode_batch(datas, "cpu", sampling="native")
    assert info["sampling"] == "native" and info["sampling_images"] == 0
    assert info["fallbacks"] == [(0, "cpu_device"), (1, "cpu_device"), (3, "cpu_device")]
    for i in (0, 1, 3):
        assert np.array_equal(imgs[i].numpy(), load_image_u8(datas[i]))
    base, binfo = jpeg.decode_batch(datas, "cpu")
    assert binfo["sampling"] == "fallback" and binfo["sampling_images"] == 0 and torch.equal(base, imgs)
    for i in range(2):
        (tmp_path / f"test_{i}.JPEG").write_bytes(datas[i])
    src = GpuJpegSource("cpu", root=str(tmp_path), sampling="native")
    assert src.sampling == "native" and torch.equal(src.get(0, 1), imgs[:2])
    assert src.sampling_images == 0 and src.fallbacks == 2
    assert GpuJpegSource("cpu", root=str(tmp_path)).sampling == "fallback"


def test_unknown_mode_is_refused_everywhere():
    from idunno import inference
    from idunno.runtime.data import GpuJpegSource

    d = named("440-8x8-q50")[1]
    for bad in ("Native", "", "440", None):
        for call in (lambda: jpeg.parse(d, sampling=bad), lambda: jpeg.entropy_decode(d, sampling=bad),
                     lambda: jpeg.entropy_batch([d], 1, sampling=bad),
                     lambda: jpeg.entropy_coefs([d], sampling=bad),
                     lambda: jpeg.decode_batch([d], "cpu", sampling=bad),
                     lambda: GpuJpegSource("cpu", root=".", sampling=bad),
                     lambda: inference.deeplearning("alexnet", "alexnet", 0, 0, device="cpu", sampling=bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(SystemExit):
        inference.main(["alexnet", "0", "0", "--sampling", "yes"])


def test_both_parsers_take_the_flag_and_keep_their_defaults():
    d = named("411-128x24-q50")[1]
    C = ops.load()
    for parse in (ops.jpeg_parse, C.jpeg_parse):
        assert parse(d)[:2] == (9, "sampling") and parse(d, False)[:2] == (9, "sampling")
        assert parse(d, True)[:2] == (9, "sampling")                     # native_progressive alone does not take it
        st, reason, h = parse(d, False, True)
        assert (st, reason, h["mode"]) == (0, "ok", 4)
        assert parse(d, native_sampling=True)[0] == 0
    assert list(inspect.signature(ops.jpeg_parse).parameters) == ["data", "native_progressive", "native_sampling",
                                                                  "native_colorspace"]
    assert inspect.signature(ops.jpeg_parse).parameters["native_sampling"].default is False
    assert inspect.signature(ops.jpeg_parse).parameters["native_colorspace"].default is False
    for fn in (jpeg.parse, jpeg.entropy_decode, jpeg.entropy_batch, jpeg.entropy_coefs, jpeg.decode_batch):
        assert inspect.signature(fn).parameters["sampling"].default == "fallback", fn.__name__
    # the packer takes it too, remembers it, and lays such a file out like any other of its kind
    assert ops.jpeg_huff_pack([d]).status == [9] and ops.jpeg_huff_pack([d]).native_sampling is False
    pk = ops.jpeg_huff_pack([d], native_sampling=True)
    assert pk.status == [0] and pk.native_sampling is True and pk.n_lane == 1 and pk.coef_total == 72 * 64
    assert ops.jpeg_huff_pack([d], True, False, False, True).n_par == 1
    # the header rows keep their layout
    assert ops.JPEG_HEADER_MODE_OFFSET == 20 and ops.JPEG_HEADER_PROGRESSIVE_OFFSET == 500
    assert pk.hdr.numpy().view(np.int32)[0, ops.JPEG_HEADER_MODE_OFFSET // 4] == 4


def test_command_lines_pass_the_mode_on(monkeypatch):
    from idunno import inference, launch

    seen = []

    def fake(filename, modelname, start, end, **kw):
        seen.append(kw["sampling"])
        return [], 0.0

    monkeypatch.setattr(inference, "deeplearning", fake)
    assert inference.main(["alexnet", "0", "0", "--decoder", "gpu", "--sampling", "native"]) == 0
    assert inference.main(["alexnet", "0", "0"]) == 0
    assert seen == ["native", "fallback"]
    a = launch.build_parser().parse_args(["node", "--jpeg-sampling", "native"])
    assert a.jpeg_sampling == "native" and launch.build_parser().parse_args(["node"]).jpeg_sampling == "fallback"
    src = inspect.getsource(launch)
    assert '"--jpeg-sampling", a.jpeg_sampling' in src and "sampling=a.jpeg_sampling" in src
