"""``progressive="native"`` without a GPU: the marker walk and the host decoder on
progressive files against their baseline twins (identical quantised coefficients,
tests/jpeg_prog_cases.py), the float64 model against Pillow, refusals, and the
option's validation and CPU-device behaviour everywhere it is accepted."""
import numpy as np
import pytest
import torch
from jpeg_cases import MAX_MODEL, MEAN_BOUND, diff_stats, pil_rgb, progressive
from jpeg_prog_cases import clobber_scan, named, pairs, patch_refinement_ah

from idunno.runtime import jpeg


def test_default_still_refuses_progressive():
    p = named("70x46-420-q95")[1]
    assert jpeg.parse(p) == "progressive" and jpeg.parse(p, progressive="fallback") == "progressive"
    assert jpeg.entropy_decode(p) == "progressive"
    assert jpeg.parse(progressive()) == "progressive"


def test_native_parse_reports_the_scan_script():
    for name, p, twin in pairs():
        h, t = jpeg.parse(p, progressive="native"), jpeg.parse(twin, progressive="native")
        assert isinstance(h, dict), (name, h)
        assert h["progressive"] is True and h["nscans"] == (6 if "grey" in name else 10), name
        assert t["progressive"] is False and t["nscans"] == 1 and t == jpeg.parse(twin)
        for k in ("W", "H", "ncomp", "hmax", "vmax", "mode", "total_coefs", "comp"):
            assert h[k] == t[k], (name, k)          # the same frame, layout and quantisation tables


@pytest.mark.parametrize("name", [p[0] for p in pairs()])
def test_native_host_decode_equals_the_baseline_twin(name):
    _, p, twin = named(name)
    h, c = jpeg.entropy_decode(p, progressive="native")
    _, want = jpeg.entropy_decode(twin)
    assert c.dtype == np.int16 and np.array_equal(c, want)
    mx, mean = diff_stats(jpeg.reference_backend(h, c), pil_rgb(p))
    print(name, mx, mean)
    assert mx <= MAX_MODEL and mean <= MEAN_BOUND


def test_corrupt_progressive_files_are_refused():
    p = named("70x46-420-q95")[1]
    for bad in (p[:len(p) // 2], patch_refinement_ah(p), clobber_scan(p)):
        assert bad != p
        assert jpeg.entropy_decode(bad, progressive="native") == "corrupt"
        st, offs, _ = jpeg.entropy_coefs([p, bad], progressive="native")
        assert st[0] == 0 and st[1] == 3
    assert jpeg.parse(p[:len(p) // 2], progressive="native") == "corrupt"          # no EOI
    assert jpeg.parse(patch_refinement_ah(p), progressive="native") == "corrupt"   # Ah != Al + 1
    assert isinstance(jpeg.parse(clobber_scan(p), progressive="native"), dict)     # the walk is fine, the scan is not


def test_more_scans_than_the_cap_is_multiscan():
    from idunno import ops

    p = named("8x8-444-q50")[1]
    # repeat the last scan (a refinement: decoding it twice is harmless) until the cap is passed
    at = p.rindex(b"\xff\xda")
    scan = p[at:-2]
    many = p[:-2] + scan * (ops.JPEG_PROG_MAX_SCANS - 10) + p[-2:]
    assert jpeg.parse(many, progressive="native")["nscans"] == ops.JPEG_PROG_MAX_SCANS
    assert jpeg.parse(p[:-2] + scan * (ops.JPEG_PROG_MAX_SCANS - 9) + p[-2:], progressive="native") == "multiscan"


def test_unknown_mode_is_refused_everywhere():
    from idunno import inference
    from idunno.runtime.data import GpuJpegSource

    p = named("8x8-444-q50")[1]
    for bad in ("Native", "", "gpu"):
        for call in (lambda: jpeg.parse(p, progressive=bad), lambda: jpeg.entropy_decode(p, progressive=bad),
                     lambda: jpeg.entropy_batch([p], 1, progressive=bad),
                     lambda: jpeg.entropy_coefs([p], progressive=bad),
                     lambda: jpeg.decode_batch([p], "cpu", progressive=bad),
                     lambda: GpuJpegSource("cpu", root=".", progressive=bad),
                     lambda: inference.deeplearning("alexnet", "alexnet", 0, 0, device="cpu", progressive=bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(SystemExit):
        inference.main(["alexnet", "0", "0", "--progressive", "yes"])


def test_mode_is_reported_and_ignored_on_a_cpu_device(tmp_path):
    from idunno.runtime.data import GpuJpegSource, load_image_u8

    datas = [named("70x46-420-q95")[1], named("70x46-420-q95")[2], None]
    imgs, info = jpeg.decode_batch(datas, "cpu", progressive="native")
    assert info["progressive"] == "native" and info["progressive_images"] == 0
    assert [r for _, r in info["fallbacks"]] == ["cpu_device"] * 2
    for i in range(2):
        assert np.array_equal(imgs[i].numpy(), load_image_u8(datas[i]))
    base, binfo = jpeg.decode_batch(datas, "cpu")
    assert binfo["progressive"] == "fallback" and binfo["progressive_images"] == 0 and torch.equal(base, imgs)
    for i in range(2):
        (tmp_path / f"test_{i}.JPEG").write_bytes(datas[i])
    src = GpuJpegSource("cpu", root=str(tmp_path), progressive="native")
    assert src.progressive == "native" and torch.equal(src.get(0, 1), imgs[:2])
    assert src.progressive_images == 0 and src.fallbacks == 2
    assert GpuJpegSource("cpu", root=str(tmp_path)).progressive == "fallback"


def test_command_lines_pass_the_mode_on(monkeypatch):
    from idunno import inference, launch

    seen = []

    def fake(filename, modelname, start, end, **kw):
        seen.append(kw["progressive"])
        return [], 0.0

    monkeypatch.setattr(inference, "deeplearning", fake)
    assert inference.main(["alexnet", "0", "0", "--decoder", "gpu", "--progressive", "native"]) == 0
    assert inference.main(["alexnet", "0", "0"]) == 0
    assert seen == ["native", "fallback"]
    import inspect

    src = inspect.getsource(launch)
    assert "--jpeg-progressive" in src and "progressive=a.jpeg_progressive" in src
