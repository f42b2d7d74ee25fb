"""4:4:0 and 4:1:1 JPEGs for the tests of ``sampling="native"`` (seeded, no fixture files).

Pillow writes neither layout, so each file is a Pillow file of another layout whose MCUs
have the same block structure, with three fields of its frame header rewritten: width,
height and the luma sampling byte.

* 4:4:0 (luma 1x2), w x h: a 4:2:2 file of width h and height w.  Both have MCUs of
  Y Y Cb Cr, and the MCU count and every component's block count agree for every size.
* 4:1:1 (luma 4x1), W2 x H2: a 4:2:0 file w x h with as many MCUs (Y Y Y Y Cb Cr); a
  progressive one also needs every component's own block count to agree.

The pictures are scrambled, which does not matter: Pillow (libjpeg-turbo) decodes the very
same bytes and is the oracle."""
import functools

from jpeg_cases import encode


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def rewrite(data: bytes, hv: int, w: int, h: int) -> bytes:
    """``data`` with its SOF0 / SOF2 saying w x h and the first component sampled ``hv``."""
    d = bytearray(data)
    pos = 2
    while True:
        assert d[pos] == 0xFF, "marker expected"
        m, seglen = d[pos + 1], (d[pos + 2] << 8) | d[pos + 3]
        if m in (0xC0, 0xC2):
            assert d[pos + 9] == 3, "three components expected"
            d[pos + 5:pos + 7] = h.to_bytes(2, "big")
            d[pos + 7:pos + 9] = w.to_bytes(2, "big")
            d[pos + 11] = hv
            return bytes(d)
        assert m != 0xDA, "no frame header in front of the scan"
        pos += 2 + seglen


def make_440(w: int, h: int, quality: int = 75, seed: int = 0, smooth: bool = False, **kw) -> bytes:
    """A 4:4:0 file of w x h from the 4:2:2 file of h x w (kw: Pillow save options)."""
    # source MCUs 16x8 over h x w, target MCUs 8x16 over w x h: ceil(h / 16) * ceil(w / 8) either way, and
    # the components' own grids are each other's transposes
    return rewrite(encode(h, w, "422", quality, seed=seed, smooth=smooth, **kw), 0x12, w, h)


def make_411(w: int, h: int, w2: int, h2: int, quality: int = 75, seed: int = 0, smooth: bool = False, **kw) -> bytes:
    """A 4:1:1 file of w2 x h2 from the 4:2:0 file of w x h (kw: Pillow save options)."""
    assert _ceil(w2, 32) * _ceil(h2, 8) == _ceil(w, 16) * _ceil(h, 16), "MCU counts differ"
    if kw.get("progressive"):
        assert _ceil(w2, 8) * _ceil(h2, 8) == _ceil(w, 8) * _ceil(h, 8), "luma block counts differ"
        assert _ceil(_ceil(w2, 4), 8) * _ceil(h2, 8) == _ceil(_ceil(w, 2), 8) * _ceil(_ceil(h, 2), 8), \
            "chroma block counts differ"
    return rewrite(encode(w, h, "420", quality, seed=seed, smooth=smooth, **kw), 0x41, w2, h2)


def make_h1v4(w: int, h: int, quality: int = 80, seed: int = 5) -> bytes:
    """Luma 1x4 (w / 2 x 2h from a 4:2:0 file of w x h): a layout no mode takes."""
    assert w % 16 == 0 and h % 16 == 0
    return rewrite(encode(w, h, "420", quality, seed=seed, smooth=True), 0x14, w // 2, 2 * h)


SIZES_440 = [(8, 8), (16, 16), (17, 9), (67, 45), (64, 48), (70, 46), (38, 30), (54, 22), (9, 17), (3, 40), (40, 3),
             (2, 33)]
# source (4:2:0) -> targets: the exact fit, then sizes whose last MCU column and row are cut
SIZES_411 = [((64, 48), [(128, 24), (123, 21), (97, 17)]),
             ((32, 16), [(64, 8), (59, 5)]),
             ((96, 32), [(192, 16), (187, 13), (161, 9)]),
             ((16, 16), [(32, 8), (27, 5)]),
             ((80, 64), [(160, 32), (155, 29), (129, 25)])]


@functools.lru_cache(maxsize=None)
def full_res_cases():
    """The 51 (name, bytes, mode): every 4:4:0 size and every 4:1:1 target at quality 50 and 95,
    smooth and random content alternating, plus a 4:4:0 file with restart markers."""
    out = []
    i = 0
    for w, h in SIZES_440:
        for q in (50, 95):
            i += 1
            out.append((f"440-{w}x{h}-q{q}", make_440(w, h, q, seed=100 + i, smooth=i % 2 == 0), 3))
    out.append(("440-70x46-rst2", make_440(70, 46, 75, seed=7, smooth=True, restart_marker_blocks=2), 3))
    for (w, h), targets in SIZES_411:
        for q in (50, 95):
            i += 1
            for w2, h2 in targets:
                out.append((f"411-{w2}x{h2}-q{q}", make_411(w, h, w2, h2, q, seed=200 + i, smooth=i % 2 == 0), 4))
    return tuple(out)


def named(name):
    return next(c for c in full_res_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def progressive_cases():
    """(name, bytes, mode) of progressive files: the sources written with ``progressive=True``.
    A scan of one component walks that component's own grid in raster order while the
    interleaved DC scans walk MCUs, so such a file is scrambled differently from the baseline
    file of the same source and is no twin of it: Pillow on the file itself is the oracle.
    4:1:1 needs (2w, h / 2) of a source whose sides are multiples of 16."""
    out = []
    for k, (w, h) in enumerate([(8, 8), (17, 9), (70, 46), (38, 30), (9, 17), (2, 33)]):
        out.append((f"p440-{w}x{h}", make_440(w, h, (50, 95)[k % 2], seed=300 + k, smooth=k % 2 == 0, progressive=True), 3))
    out.append(("p440-70x46-rst2", make_440(70, 46, 75, seed=310, smooth=True, progressive=True,
                                            restart_marker_blocks=2), 3))
    for k, (w, h) in enumerate([(64, 48), (32, 16), (96, 32), (16, 16), (80, 64)]):
        out.append((f"p411-{2 * w}x{h // 2}", make_411(w, h, 2 * w, h // 2, (95, 50)[k % 2], seed=320 + k,
                                                       smooth=k % 2 == 1, progressive=True), 4))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def resize_cases():
    """(name, bytes, mode) of the resize + crop tests: smooth images at quality 90."""
    return (("440-250x333", make_440(250, 333, 90, seed=50, smooth=True), 3),
            ("440-333x250", make_440(333, 250, 90, seed=51, smooth=True), 3),
            ("411-640x120", make_411(320, 240, 640, 120, 90, seed=52, smooth=True), 4),
            ("411-512x192", make_411(256, 384, 512, 192, 90, seed=53, smooth=True), 4))


def check_files():
    """The six (name, bytes) of the stand-alone sanitizer program: one 4:4:0 and one 4:1:1 file,
    each plain, with restart markers and progressive."""
    a = dict(quality=75, seed=401, smooth=True)
    b = dict(quality=85, seed=402, smooth=False)
    return [("440", make_440(38, 30, **a)),
            ("440-rst", make_440(38, 30, restart_marker_blocks=2, **a)),
            ("440-prog", make_440(38, 30, progressive=True, **a)),
            ("411", make_411(32, 32, 64, 16, **b)),
            ("411-rst", make_411(32, 32, 64, 16, restart_marker_blocks=1, **b)),
            ("411-prog", make_411(32, 32, 64, 16, progressive=True, **b))]
