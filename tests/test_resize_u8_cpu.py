"""resize_crop_u8's coefficient tables (csrc/resize_math.h through the extension's host-only
``resize_u8_plan``) against Pillow itself, without a GPU: Pillow's BILINEAR resize of an
identity image (a delta of 255 in every input column) along one axis shows every output's
weight of every input at 8 bits, and the tables must predict each of those bytes."""
import numpy as np
import pytest

from idunno import ops

GEOMETRIES = [(375, 500, 256, 224), (500, 375, 256, 224), (224, 224, 256, 224), (256, 256, 256, 256),
              (225, 300, 256, 224), (30, 40, 32, 29), (17, 1031, 16, 16), (1031, 17, 16, 16), (1, 50, 8, 8)]


@pytest.mark.parametrize("hi,wi,resize,crop", GEOMETRIES)
def test_tables_predict_pillows_response_to_a_delta(hi, wi, resize, crop):
    Image = pytest.importorskip("PIL.Image")
    plan = ops.load().resize_u8_plan(hi, wi, resize, crop)
    hr, wr, top, left = ops.resize_crop_geometry(hi, wi, resize, crop)
    for n_in, n_out, first, b, k in ((wi, wr, left, plan["bh"], plan["kh"]), (hi, hr, top, plan["bv"], plan["kv"])):
        b, k = b.numpy(), k.numpy().astype(np.int64)
        # row j of the identity image is a delta at input j; resized along the row axis only
        resp = np.asarray(Image.fromarray(np.eye(n_in, dtype=np.uint8) * 255).resize((n_out, n_in), Image.BILINEAR))
        want = resp[:, first:first + crop].T.astype(np.int64)               # [output, input]
        got = np.zeros_like(want)
        for o in range(crop):
            lo, n = b[o]
            assert 0 <= lo and 1 <= n <= k.shape[1] and lo + n <= n_in
            assert abs(int(k[o].sum()) - (1 << 22)) <= (n + 1) // 2 and not k[o, n:].any()
            got[o, lo:lo + n] = ((1 << 21) + 255 * k[o, :n]) >> 22
        assert np.array_equal(got, want)
    assert plan["lds_bytes"] <= 64 * 1024 and not plan["chunked"]
