"""``restart="intervals"`` on the device (jpeg_entropy_rst_kernel: one restart
interval per lane, csrc/jpeg_huff_rst.h) in both device forms: statuses and
offsets equal the host decoder's and the coefficients of every accepted image
are bit-identical to it, so decode_batch and GpuJpegSource outputs are
``torch.equal`` to the host form's, fallbacks included; an image one of whose
intervals the kernel refuses is a ``"corrupt"`` fallback; the default
``restart="lane"`` is unchanged."""
import functools

import pytest
import torch
from jpeg_cases import encode, png
from jpeg_prog_cases import named
from jpeg_restart_cases import files, mutant_fill, refused_mutants, table

from idunno import ops
from idunno.runtime import jpeg
from idunno.runtime.data import GpuJpegSource

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("gpu", "gpu_parallel")
NT = 10                 # the table's files, all decoded by the interval kernel
N_RST = NT + 2          # plus the fill-byte mutant and the data-byte mutant (every marker in place: refused by a lane)
N_ACCEPTED = NT + 1


@functools.lru_cache(maxsize=None)
def batch():
    """The table's files in the table's order (15 intervals, then 130: one image's items straddle two
    wave boundaries), the fill-byte mutant, the four refused mutants, a file without a restart
    interval, a progressive file with restart markers, None and a PNG."""
    first = files()[0]
    return tuple(files() + [mutant_fill(first)] + [m for _, m in refused_mutants(first)] +
                 [encode(38, 30, "420", 75, seed=2), named("70x46-420-rst3")[1], None, png()])


@functools.lru_cache(maxsize=None)
def image_batch():
    """The batch without the file cut inside its marker: Pillow, which decodes the fallbacks of
    decode_batch in every form, raises on a truncated file (the entropy stage's verdict on it is
    checked on the whole batch by the coefficient tests)."""
    assert refused_mutants(files()[0])[3][0] == "cut"
    return batch()[:NT + 4] + batch()[NT + 5:]


def test_the_batch_is_the_one_the_issue_names():
    counts = [k for _, k in table()]
    assert len(counts) == NT and counts[0] == 15 and counts[8] == 130
    first = sum(counts[:8])                       # the 130-interval file's items: lanes [first, first + 130)
    assert first // 64 + 2 == (first + 129) // 64                 # one image's items straddle two wave boundaries
    assert len(batch()) == NT + 9 and max(len(d) for d in batch()[:-1] if d) < 20 << 10


@functools.lru_cache(maxsize=None)
def host_coefs():
    """The host decoder over the batch, computed once."""
    return jpeg.entropy_coefs(list(batch()), entropy_on="host")


def _assert_same_coefs(datas, form, want=None, **kw):
    hs, ho, hc = want or jpeg.entropy_coefs(datas, entropy_on="host")
    gs, go, gc = jpeg.entropy_coefs(datas, DEV, entropy_on=form, **kw)
    assert gs == hs and go == ho and gc.dtype == torch.int16 and gc.shape == hc.shape
    for i, d in enumerate(datas):
        if hs[i] == 0:
            n = jpeg.parse(d)["total_coefs"]
            assert torch.equal(gc[go[i]:go[i] + n], hc[ho[i]:ho[i] + n]), f"image {i}: coefficients differ"
    return gs


@pytest.mark.parametrize("form", FORMS)
def test_coefficients_are_bit_identical_to_the_host_decoder(form):
    datas = list(batch())
    pk = ops.jpeg_huff_pack(datas, form == "gpu_parallel", False, True)
    assert pk.n_rst == N_RST and sorted(set(pk.rst_items[:, 0].tolist())) == list(range(NT + 1)) + [NT + 3]
    # the three mutants whose marker the byte scan misses, and the file without a restart interval
    assert (pk.n_lane, pk.n_par) == ((3, 1) if form == "gpu_parallel" else (4, 0))
    st = _assert_same_coefs(datas, form, host_coefs(), restart="intervals")
    # every table file and the fill-byte mutant accepted, the four other mutants refused, the rest as the parse says
    assert st[:NT + 1] == [0] * (NT + 1) and st[NT + 1:NT + 5] == [3] * 4 and st[NT + 5] == 0
    assert all(s != 0 for s in st[NT + 6:])


@pytest.mark.parametrize("form", FORMS)
def test_batches_of_one(form):
    for at, k in ((7, 1), (8, 130), (0, 15)):      # the 8x8 file, more than two waves, the index past RST7
        d = files()[at]
        assert ops.jpeg_huff_pack([d], form == "gpu_parallel", False, True).rst_items.shape[0] == k
        assert _assert_same_coefs([d], form, restart="intervals") == [0]
    bad = dict(refused_mutants(files()[0]))["data-byte"]
    assert _assert_same_coefs([bad], form, restart="intervals") == [3]            # refused by a lane of the interval kernel


@pytest.mark.parametrize("form", FORMS)
def test_images_and_fallbacks_equal_the_host_form(form, tmp_path):
    datas = list(image_batch())
    want_fb = [(NT + 1 + j, "corrupt") for j in range(3)] + [(NT + 5, "progressive"), (NT + 7, "not_jpeg")]
    host, hinfo = jpeg.decode_batch(datas, DEV, entropy_on="host")
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on=form, restart="intervals")
    assert hinfo["fallbacks"] == want_fb and hinfo["restart"] == "lane" and hinfo["restart_images"] == 0
    assert ginfo["fallbacks"] == want_fb and ginfo["entropy_on"] == form
    assert ginfo["restart"] == "intervals" and ginfo["restart_images"] == N_ACCEPTED
    assert ginfo["gpu_images"] == hinfo["gpu_images"] == N_ACCEPTED + 1
    assert torch.equal(gpu, host)
    full_h, _ = jpeg.decode_batch(datas, DEV, resize=None, crop=None)
    full_g, finfo = jpeg.decode_batch(datas, DEV, resize=None, crop=None, entropy_on=form, restart="intervals")
    assert finfo["fallbacks"] == want_fb and finfo["restart_images"] == N_ACCEPTED
    for a, b in zip(full_h, full_g):
        assert (a is None and b is None) or torch.equal(a, b)
    # the host form takes the keyword and changes nothing
    same, sinfo = jpeg.decode_batch(datas, DEV, entropy_on="host", restart="intervals")
    assert sinfo["restart"] == "intervals" and sinfo["restart_images"] == 0 and torch.equal(same, host)
    for i, d in enumerate(datas):
        if d is not None:
            (tmp_path / f"test_{i}.JPEG").write_bytes(d)
    n = len(datas)
    want = GpuJpegSource(DEV, root=str(tmp_path)).get(0, n - 1)
    assert torch.equal(want, host)
    src = GpuJpegSource(DEV, root=str(tmp_path), entropy_on=form, restart="intervals")
    assert torch.equal(src.get(0, n - 1), want)
    assert src.restart_images == N_ACCEPTED and src.fallbacks == len(want_fb) and src.missing == [NT + 6]
    assert sorted(src.fallback_reasons.items()) == want_fb


@pytest.mark.parametrize("form", FORMS)
def test_the_default_is_unchanged(form):
    datas = list(batch())
    pk = ops.jpeg_huff_pack(datas, form == "gpu_parallel", False)
    assert pk.n_rst == 0 and pk.rst_items.shape[0] == 0 and pk.n_lane == NT + 5 + (form == "gpu")
    _assert_same_coefs(datas, form, host_coefs())
    _assert_same_coefs(datas, form, host_coefs(), restart="lane")
    datas = list(image_batch())
    host, _ = jpeg.decode_batch(datas, DEV, entropy_on="host")
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy_on=form)
    assert ginfo["restart"] == "lane" and ginfo["restart_images"] == 0 and torch.equal(gpu, host)
    assert [r for _, r in ginfo["fallbacks"]] == ["corrupt"] * 3 + ["progressive", "not_jpeg"]


@pytest.mark.parametrize("form", FORMS)
def test_a_prepared_entropy_stage_decides_the_mode(form):
    datas = list(image_batch())
    host, _ = jpeg.decode_batch(datas, DEV, entropy_on="host")
    ent = jpeg.entropy_batch(datas, 8, form, restart="intervals")
    assert ent.packed.restart_intervals is True and ent.packed.n_rst == N_RST
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy=ent)                       # called with the default
    assert ginfo["restart"] == "intervals" and ginfo["restart_images"] == N_ACCEPTED and ginfo["entropy_on"] == form
    assert torch.equal(gpu, host)
    ent = jpeg.entropy_batch(datas, 8, form)                                      # and the other way round
    gpu, ginfo = jpeg.decode_batch(datas, DEV, entropy=ent, restart="intervals")
    assert ginfo["restart"] == "lane" and ginfo["restart_images"] == 0 and torch.equal(gpu, host)
