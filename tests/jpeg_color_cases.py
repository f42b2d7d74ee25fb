"""RGB-coded, CMYK and YCCK JPEGs for the tests of ``colorspace="auto"`` (seeded, no fixture files).

Pillow writes CMYK files (ids ``C,M,Y,K``, every component 1x1, an Adobe APP14 with
transform 0 right after SOI) and, with ``keep_rgb=True``, 4:4:4 RGB files (ids ``R,G,B``,
Adobe transform 0, no JFIF).  Every other kind is one of those, or an ordinary YCbCr
file, with a marker segment rewritten, cut out or put in; the entropy-coded bytes stay
as they are.  The pictures of the rewritten files have odd colours, which does not
matter: Pillow (libjpeg-turbo) decodes the very same bytes and is the oracle.

Each case is ``(name, bytes, colorspace)`` with the colour space the parser must find:
0 YCbCr, 1 RGB, 2 CMYK, 3 YCCK."""
import functools
import io

import numpy as np
from PIL import Image

from jpeg_cases import MAX_MODEL, MEAN_BOUND, encode, pixels

YCBCR, RGB, CMYK, YCCK = 0, 1, 2, 3
KIND = {YCBCR: "ycbcr", RGB: "rgb", CMYK: "cmyk", YCCK: "ycck"}

# Maximum error of the float64 model against Pillow, per colour space.  libjpeg's integer IDCT is
# within one level of the exact one per plane (the premise of tests/test_jpeg_gpu.py).  RGB hands that
# level on: 1.  f = nk - round(c nk / 255) over all (c, nk) with |dc| <= 1, |dnk| <= 1 moves by at most
# 2 (CMYK); with |dc| <= 3, the YCbCr bound MAX_MODEL, and |dnk| <= 1 by at most 4 (YCCK).  Both are
# checked exhaustively in test_jpeg_color_cpu.py.  The resize passes are convex combinations rounded
# to uint8 twice and keep a bound (tests/test_jpeg_gpu.py).
MAX_PIL = {YCBCR: MAX_MODEL, RGB: 1, CMYK: 2, YCCK: 4}
# The GPU against the model: at most one level of one plane (an fp32 / fp64 rounding tie in the IDCT),
# propagated as above: one level of RGB, two of CMYK / YCCK; YCbCr keeps the project's bound of 1.
MAX_GPU_MODEL = {YCBCR: 1, RGB: 1, CMYK: 2, YCCK: 2}
# Mean error of the model against Pillow.  Measured worst over full_res_cases(), progressive_cases() and
# resize_cases() (full resolution and resized), Pillow 12.2.0: YCbCr 0.050, RGB 0.042, CMYK 0.033, YCCK
# 0.044 (maxima 3, 1, 2, 4): all under the project's MEAN_BOUND (0.13), which therefore holds for every
# colour space; the maxima above are the sharper check.
MEAN_PIL = {YCBCR: MEAN_BOUND, RGB: MEAN_BOUND, CMYK: MEAN_BOUND, YCCK: MEAN_BOUND}

ADOBE_RGB = b"\xFF\xEE\x00\x0EAdobe\x00\x64\x00\x00\x00\x00\x00"      # APP14, transform 0

SIZES = [(8, 8), (17, 9), (67, 45), (2, 33), (40, 3)]


def pixels4(w: int, h: int, seed: int, smooth: bool = False) -> np.ndarray:
    """Four channels; the fourth (K) smooth or random like the other three."""
    a = pixels(w, h, seed, smooth)
    k = pixels(w, h, seed + 7919, smooth)[:, :, :1]
    return np.ascontiguousarray(np.concatenate([a, k], 2))


def encode_cmyk(w: int, h: int, quality: int = 75, seed: int = 0, smooth: bool = False, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels4(w, h, seed, smooth), "CMYK").save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def encode_rgb444(w: int, h: int, quality: int = 75, seed: int = 0, smooth: bool = False, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels(w, h, seed, smooth), "RGB").save(buf, "JPEG", quality=quality, keep_rgb=True, **kw)
    return buf.getvalue()


def segments(data: bytes):
    """(marker, start, end) of every segment in front of the first scan's data, SOS included."""
    pos = 2
    while True:
        assert data[pos] == 0xFF, "marker expected"
        m, seglen = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        yield m, pos, pos + 2 + seglen
        if m == 0xDA:
            return
        pos += 2 + seglen


def cut(data: bytes, marker: int) -> bytes:
    """``data`` without its segments of this marker (0xE0: JFIF, 0xEE: Adobe)."""
    out, at = bytearray(data[:2]), 2
    for m, a, b in segments(data):
        if m != marker:
            out += data[a:b]
        at = b
    assert len(out) < at, "no such segment"
    return bytes(out) + data[at:]


def set_transform(data: bytes, transform: int) -> bytes:
    i = data.index(b"Adobe")
    d = bytearray(data)
    d[i + 11] = transform
    return bytes(d)


def jfif_to_adobe(data: bytes, transform: int = 0) -> bytes:
    """The JFIF APP0 replaced by an Adobe APP14."""
    (a, b), = [(a, b) for m, a, b in segments(data) if m == 0xE0]
    return set_transform(data[:a] + ADOBE_RGB + data[b:], transform)


def add_adobe(data: bytes, transform: int = 0) -> bytes:
    """An Adobe APP14 put in right after the JFIF APP0."""
    (a, b), = [(a, b) for m, a, b in segments(data) if m == 0xE0]
    return set_transform(data[:b] + ADOBE_RGB + data[b:], transform)


def rgb_ids(data: bytes) -> bytes:
    """The component ids of every frame and scan header rewritten 1, 2, 3 -> R, G, B (all scans of a
    progressive file)."""
    d = bytearray(data)
    ids = {1: ord("R"), 2: ord("G"), 3: ord("B")}
    pos = 2
    while pos + 4 <= len(d):
        if d[pos] != 0xFF or d[pos + 1] in (0x00, 0xFF) or 0xD0 <= d[pos + 1] <= 0xD9:
            pos += 1                                   # entropy-coded data, RSTn, EOI
            continue
        m, seglen = d[pos + 1], (d[pos + 2] << 8) | d[pos + 3]
        if m in (0xC0, 0xC2):
            for c in range(d[pos + 9]):
                d[pos + 10 + 3 * c] = ids[d[pos + 10 + 3 * c]]
        elif m == 0xDA:
            for c in range(d[pos + 4]):
                d[pos + 5 + 2 * c] = ids[d[pos + 5 + 2 * c]]
        pos += 2 + seglen
    return bytes(d)


def make(kind: str, w: int, h: int, quality: int = 75, seed: int = 0, smooth: bool = False, **kw):
    """One (bytes, colorspace) of the named recipe; kw: Pillow save options."""
    a = dict(quality=quality, seed=seed, smooth=smooth, **kw)
    if kind == "cmyk":
        return encode_cmyk(w, h, **a), CMYK
    if kind == "ycck":                                  # the same bytes with the transform byte set to 2
        return set_transform(encode_cmyk(w, h, **a), 2), YCCK
    if kind == "cmyk-noadobe":
        return cut(encode_cmyk(w, h, **a), 0xEE), CMYK
    if kind == "rgb444":
        return encode_rgb444(w, h, **a), RGB
    if kind in ("rgb422", "rgb420"):                    # keep_rgb with subsampling: Pillow raises
        return jfif_to_adobe(encode(w, h, kind[3:], **a)), RGB
    if kind == "rgb-ids":                               # no marker at all, the ids decide
        return rgb_ids(cut(encode(w, h, "420", **a), 0xE0)), RGB
    # files that must stay YCbCr
    if kind == "ids-jfif":                              # RGB ids, JFIF kept
        return rgb_ids(encode(w, h, "422", **a)), YCBCR
    if kind == "adobe0-jfif":                           # Adobe transform 0 next to JFIF
        return add_adobe(encode(w, h, "420", **a), 0), YCBCR
    if kind == "adobe1":
        return jfif_to_adobe(encode(w, h, "444", **a), 1), YCBCR
    if kind == "nomarker":                              # ids 1, 2, 3 and nothing else
        return cut(encode(w, h, "420", **a), 0xE0), YCBCR
    raise ValueError(kind)


NEW_KINDS = ["cmyk", "ycck", "cmyk-noadobe", "rgb444", "rgb422", "rgb420", "rgb-ids"]
YCBCR_KINDS = ["ids-jfif", "adobe0-jfif", "adobe1", "nomarker"]


@functools.lru_cache(maxsize=None)
def full_res_cases():
    """(name, bytes, colorspace): every new kind at every size at quality 50 and 95, smooth and random
    content alternating, a CMYK and a YCCK file with restart markers, and the four kinds that stay YCbCr."""
    out = []
    i = 0
    for kind in NEW_KINDS:
        for w, h in SIZES:
            for q in (50, 95):
                i += 1
                out.append((f"{kind}-{w}x{h}-q{q}", *make(kind, w, h, q, seed=500 + i, smooth=i % 2 == 0)))
    out.append(("cmyk-67x45-rst2", *make("cmyk", 67, 45, 75, seed=481, smooth=True, restart_marker_blocks=2)))
    out.append(("ycck-40x3-rst2", *make("ycck", 40, 3, 85, seed=482, restart_marker_blocks=2)))
    out.append(("rgb420-67x45-rst2", *make("rgb420", 67, 45, 75, seed=483, smooth=True, restart_marker_blocks=2)))
    for k, kind in enumerate(YCBCR_KINDS):
        out.append((f"{kind}-67x45", *make(kind, 67, 45, 75, seed=490 + k, smooth=k % 2 == 0)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def progressive_cases():
    """(name, bytes, colorspace) of progressive files, with the baseline file of the same pixels and
    quality: (name, progressive bytes, colorspace, baseline bytes)."""
    out = []
    spec = [("cmyk", 17, 9, 50, {}), ("cmyk", 67, 45, 95, {}), ("ycck", 2, 33, 75, {}), ("ycck", 67, 45, 50, {}),
            ("cmyk-noadobe", 40, 3, 95, {}), ("cmyk", 67, 45, 75, {"restart_marker_blocks": 2}),
            ("rgb444", 17, 9, 75, {}), ("rgb420", 67, 45, 75, {}), ("rgb-ids", 40, 3, 75, {})]
    for k, (kind, w, h, q, kw) in enumerate(spec):
        a = dict(quality=q, seed=600 + k, smooth=k % 2 == 0, **kw)
        prog, cs = make(kind, w, h, progressive=True, **a)
        base, _ = make(kind, w, h, **a)
        out.append((f"p-{kind}-{w}x{h}" + ("-rst2" if kw else ""), prog, cs, base))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def resize_cases():
    """(name, bytes, colorspace) of the resize + crop tests: smooth images at quality 90."""
    return (("cmyk-333x250", *make("cmyk", 333, 250, 90, seed=60, smooth=True)),
            ("ycck-250x333", *make("ycck", 250, 333, 90, seed=61, smooth=True)),
            ("rgb420-333x250", *make("rgb420", 333, 250, 90, seed=62, smooth=True)),
            ("rgb422-250x333", *make("rgb422", 250, 333, 90, seed=63, smooth=True)))


def refusals():
    """(name, bytes, reason under colorspace="auto")."""
    return (("cmyk-subsampled", encode_cmyk(40, 32, 80, seed=70, smooth=True, subsampling=2), "sampling"),
            ("cmyk-transform1", set_transform(encode_cmyk(40, 32, 80, seed=71, smooth=True), 1), "components"))


def check_files():
    """The five (name, bytes) of the stand-alone sanitizer program."""
    a = dict(quality=75, seed=701, smooth=True)
    return [("cmyk", make("cmyk", 38, 30, **a)[0]),
            ("cmyk-rst", make("cmyk", 38, 30, restart_marker_blocks=2, **a)[0]),
            ("cmyk-prog", make("cmyk", 38, 30, progressive=True, **a)[0]),
            ("ycck", make("ycck", 27, 21, quality=85, seed=702)[0]),
            ("rgb-ids", make("rgb-ids", 38, 30, **a)[0])]
