"""The decoder's four opt-ins switched on together, on the GPU: the mixed batch of
jpeg_options_cases.py (every file kind the options tell apart, a PNG, a ``None``) through the
three entropy forms, with restart intervals on their own lanes and on one.  Every form must
give the coefficients each file gives alone on the host decoder with only the options it
needs, the pixels of the float64 model, and the same counters."""
import functools

import numpy as np
import pytest
import torch
from jpeg_cases import diff_stats
from jpeg_color_cases import MAX_GPU_MODEL
from jpeg_options_cases import EMPTY, NONE, NOT_JPEG, PNG, batch, datas, jpegs, strings

from idunno.runtime import jpeg

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMS = jpeg.ENTROPY_ON
ALL_ON = {"progressive": "native", "sampling": "native", "colorspace": "auto"}


@functools.lru_cache(maxsize=None)
def alone():
    """Per JPEG entry: (header, coefficients) from the host decoder, the file on its own, only its needed options on."""
    out = {}
    for i, _, d, needs, _ in jpegs():
        kw = strings(needs)
        del kw["restart"]
        out[i] = jpeg.entropy_decode(d, **kw)
    return out


@functools.lru_cache(maxsize=None)
def model():
    """Per JPEG entry: (colour space, pixels of the float64 model) under every option."""
    out = {}
    for i, _, d, _, _ in jpegs():
        h, c = jpeg.entropy_decode(d, **ALL_ON)
        out[i] = (h["colorspace"], jpeg.reference_backend(h, c))
    return out


@pytest.mark.parametrize("restart", jpeg.RESTART)
def test_coefficients_agree_in_every_form_and_with_each_file_alone(restart):
    got = [jpeg.entropy_coefs(datas(), DEV, entropy_on=form, restart=restart, **ALL_ON) for form in FORMS]
    status, offs, coefs = got[0]
    assert status == [0] * 9 + [NOT_JPEG, EMPTY] and offs[PNG] == -1 and offs[NONE] == -1
    for form, (st, of, co) in zip(FORMS[1:], got[1:]):
        assert st == status and of == offs and torch.equal(co, coefs), form
    for i, (h, c) in alone().items():
        assert np.array_equal(coefs[offs[i]:offs[i] + h["total_coefs"]].numpy(), c), batch()[i][0]
    assert coefs.numel() == sum(h["total_coefs"] for h, _ in alone().values())


@pytest.mark.parametrize("restart", jpeg.RESTART)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "entropy_on_" + f)      # no id that is a marker's name
def test_pixels_and_counters_with_every_option_on(form, restart):
    imgs, info = jpeg.decode_batch(datas(), DEV, resize=None, crop=None, entropy_on=form, restart=restart, **ALL_ON)
    assert info["fallbacks"] == [(PNG, "not_jpeg")] and imgs[NONE] is None and info["gpu_images"] == 9
    assert {k: info[k] for k in ("entropy_on", "restart", *ALL_ON)} == dict(ALL_ON, entropy_on=form, restart=restart)
    kinds = [e[3] for e in batch()]
    needs = [e[2] or () for e in batch()]
    assert info["progressive_images"] == kinds.count("progressive") == 3
    assert info["sampling_images"] == sum("sampling" in n for n in needs) == 3
    # the RGB-coded file needs no option to be taken, but is one of the option's images
    assert info["colorspace_images"] == sum(cs != 0 for cs, _ in model().values()) == 3
    assert info["restart_images"] == (kinds.count("restart") if restart == "intervals" and form != "host" else 0)
    for i, (cs, want) in model().items():
        g = imgs[i].cpu().numpy()
        assert g.shape == want.shape and g.dtype == np.uint8, batch()[i][0]
        mm, _ = diff_stats(g, want)
        print(batch()[i][0], "vs model", mm)
        assert mm <= MAX_GPU_MODEL[cs], (batch()[i][0], mm)
