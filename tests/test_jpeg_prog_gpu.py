"""``progressive="native"`` on the GPU, in the three entropy forms: progressive files
decode to the coefficients of their baseline twins (tests/jpeg_prog_cases.py; the
twins go through the untouched baseline host decoder), bit for bit, on the host
threads (``host``) and in jpeg_entropy_prog_kernel (``gpu``, ``gpu_parallel``), so
decode_batch outputs are ``torch.equal`` to the twins'.  The default mode still
falls back, a mixed batch falls back entry by entry, GpuJpegSource serves the
same rows."""
import numpy as np
import pytest
import torch
from jpeg_cases import MAX_GPU, MEAN_BOUND, diff_stats, pil_rgb, png, resize_cases
from jpeg_entropy_cases import rst1, scan_mutant
from jpeg_prog_cases import clobber_scan, named, pairs, resize_pairs

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource, load_image_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("host", "gpu", "gpu_parallel")


def _twin_coefs(twin):
    st, _, c = jpeg.entropy_coefs([twin], entropy_on="host")
    assert st == [0]
    return c


def _check_coefs(datas, twins):
    """datas[i] with twins[i] not None must decode to twins[i]'s host coefficients in every form."""
    want = {i: _twin_coefs(t) for i, t in enumerate(twins) if t is not None}
    seen = []
    for form in FORMS:
        st, offs, coefs = jpeg.entropy_coefs(datas, DEV, entropy_on=form, progressive="native")
        seen.append(st)
        for i, w in want.items():
            assert st[i] == 0 and offs[i] >= 0, (form, i, st[i])
            assert torch.equal(coefs[offs[i]:offs[i] + w.numel()], w), f"{form}: entry {i} differs from its twin"
    assert seen[0] == seen[1] == seen[2]
    return seen[0]


def test_coefficients_equal_the_baseline_twins_in_every_form():
    ps = pairs()
    assert len(ps) == 39
    datas, twins = [], []
    for _, p, t in ps:                              # progressive files, their twins interleaved
        datas += [p, t]
        twins += [t, t]
    datas += [rst1(), None, png()]
    twins += [rst1(), None, None]
    for _, p, t in ps[:30]:                         # 69 progressive entries: more than one wave of them
        datas.append(p)
        twins.append(t)
    packed = ops.jpeg_huff_pack(datas, False, True)
    assert packed.n_prog == 69 and packed.n_lane == 40 and packed.nscans == 69 * 10 - 4
    assert packed.ntabs < packed.nscans             # identical tables are shared
    par = ops.jpeg_huff_pack(datas, True, True)
    assert par.n_prog == 69 and par.n_lane == 2 and par.n_par == 38
    st = _check_coefs(datas, twins)
    assert st[-33:-30] == [0, 1, 2] and st.count(0) == len(datas) - 2
    for name in ("8x8-444-q50", "70x46-420-rst3", "200x150-420-q30"):       # batches of one
        _, p, t = named(name)
        assert _check_coefs([p], [t]) == [0]


@pytest.mark.parametrize("form", FORMS)
def test_images_equal_the_twins(form):
    progs = [p for _, p, _ in pairs()]
    twins = [t for _, _, t in pairs()]
    want, _ = jpeg.decode_batch(twins, DEV, resize=None, crop=None)
    got, info = jpeg.decode_batch(progs, DEV, resize=None, crop=None, entropy_on=form, progressive="native")
    assert info["fallbacks"] == [] and info["progressive_images"] == len(progs) == info["gpu_images"]
    assert info["progressive"] == "native" and info["entropy_on"] == form
    for (name, p, _), a, b in zip(pairs(), got, want):
        assert torch.equal(a, b), name
        mx, mean = diff_stats(a.cpu().numpy(), pil_rgb(p))
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)
    rp = resize_pairs()
    assert [t for _, _, t in rp] == [d for _, d in resize_cases()]
    progs = [p for _, p, _ in rp]
    want, _ = jpeg.decode_batch([t for _, _, t in rp], DEV)
    got, info = jpeg.decode_batch(progs, DEV, entropy_on=form, progressive="native")
    assert info["fallbacks"] == [] and info["progressive_images"] == len(progs)
    assert torch.equal(got, want)
    for (name, p, _), a in zip(rp, got):
        mx, mean = diff_stats(a.cpu().numpy(), load_image_u8(p))
        assert mx <= MAX_GPU and mean <= MEAN_BOUND, (name, mx, mean)


@pytest.mark.parametrize("form", FORMS)
def test_default_mode_still_falls_back(form):
    progs = [p for _, p, _ in pairs()[:6]]
    imgs, info = jpeg.decode_batch(progs, DEV, entropy_on=form)
    assert info["progressive"] == "fallback" and info["progressive_images"] == 0 and info["gpu_images"] == 0
    assert info["fallbacks"] == [(i, "progressive") for i in range(len(progs))]
    for i, p in enumerate(progs):
        assert np.array_equal(imgs[i].cpu().numpy(), load_image_u8(p))


def test_mixed_batch_under_native():
    _, prog, twin = named("70x46-420-q95")
    base = resize_cases()[0][1]
    datas = [prog, base, png(), None, scan_mutant(), clobber_scan(prog)]
    outs = []
    for form in FORMS:
        imgs, info = jpeg.decode_batch(datas, DEV, entropy_on=form, progressive="native")
        assert info["fallbacks"] == [(2, "not_jpeg"), (4, "corrupt"), (5, "corrupt")], form
        assert info["progressive_images"] == 1 and info["gpu_images"] == 2
        assert int(imgs[3].sum()) == 0
        for i in (2, 4, 5):
            assert np.array_equal(imgs[i].cpu().numpy(), load_image_u8(datas[i]))
        alone_p, _ = jpeg.decode_batch([prog], DEV, entropy_on=form, progressive="native")
        alone_b, _ = jpeg.decode_batch([base], DEV, entropy_on=form, progressive="native")
        assert torch.equal(imgs[0], alone_p[0]) and torch.equal(imgs[1], alone_b[0])     # unchanged by their neighbours
        outs.append(imgs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    want, _ = jpeg.decode_batch([twin], DEV)
    assert torch.equal(outs[0][0], want[0])


def test_prepared_entropy_decides_the_mode():
    _, prog, twin = named("38x30-420-q50")
    want, _ = jpeg.decode_batch([twin], DEV)
    for form in FORMS:
        ent = jpeg.entropy_batch([prog], 2, form, "native")
        imgs, info = jpeg.decode_batch([prog], DEV, entropy=ent)                  # asked for the default, prepared native
        assert info["progressive"] == "native" and info["fallbacks"] == [] and torch.equal(imgs, want)
        ent = jpeg.entropy_batch([prog], 2, form)
        imgs, info = jpeg.decode_batch([prog], DEV, entropy=ent, progressive="native")
        assert info["progressive"] == "fallback" and info["fallbacks"] == [(0, "progressive")]


@pytest.mark.parametrize("form", FORMS)
def test_gpu_jpeg_source_serves_the_twins_rows(tmp_path, form):
    rp = resize_pairs()
    pdir, tdir = tmp_path / "prog", tmp_path / "twin"
    pdir.mkdir()
    tdir.mkdir()
    for i, (_, p, t) in enumerate(rp):
        (pdir / f"test_{i}.JPEG").write_bytes(p)
        (tdir / f"test_{i}.JPEG").write_bytes(t)
    want = GpuJpegSource(DEV, root=str(tdir)).get(0, 5)
    src = GpuJpegSource(DEV, root=str(pdir), entropy_on=form, progressive="native")
    assert torch.equal(src.get(0, 5), want)                      # cold
    assert src.decoded == 6 and src.fallbacks == 0 and src.progressive_images == 6
    assert torch.equal(src.get(0, 5), want) and src.decoded == 6 and src.cache_hits == 6
    src.CHUNK = src.CHUNK_GPU = src.CHUNK_GPU_PARALLEL = 4       # more than one chunk: the prepare-ahead thread
    src.invalidate()
    assert torch.equal(src.get(0, 5), want) and src.decoded == 12 and src.fallbacks == 0
    assert src.progressive_images == 12
    old = GpuJpegSource(DEV, root=str(pdir), entropy_on=form)    # the default: every file through Pillow
    old.get(0, 5)
    assert old.fallbacks == 6 and old.progressive_images == 0 and set(old.fallback_reasons.values()) == {"progressive"}
