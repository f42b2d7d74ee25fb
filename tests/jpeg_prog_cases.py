"""Progressive JPEGs and their baseline twins for the tests of ``progressive="native"``
(seeded, no fixture files).  Pillow writes identical quantised coefficients for
``progressive=True`` and for the baseline file of the same pixels, quality,
subsampling and restart setting, so a twin decoded by the untouched baseline host
decoder is the expected output of every progressive decode, bit for bit."""
import functools

from jpeg_cases import encode, resize_cases

# sizes whose padded block grid is larger than the component's own (all but 8x8): a scan of one
# component must walk the own grid
SIZES = [(8, 8), (17, 9), (70, 46), (38, 30), (54, 22), (33, 19)]


def pair(w, h, sub="420", quality=75, seed=0, smooth=False, **kw):
    """(progressive file, baseline twin) of the same pixels and settings."""
    return (encode(w, h, sub, quality, seed=seed, smooth=smooth, progressive=True, **kw),
            encode(w, h, sub, quality, seed=seed, smooth=smooth, **kw))


@functools.lru_cache(maxsize=None)
def pairs():
    """The 39 (name, progressive, twin): every size x {4:4:4, 4:2:2, 4:2:0} x {quality 50 smooth,
    quality 95 noise}, one grey, one with restart markers in every scan, one 200x150 at quality 30
    (EOB runs of hundreds of blocks)."""
    out = []
    for i, (w, h) in enumerate(SIZES):
        for j, sub in enumerate(("444", "422", "420")):
            for q, smooth in ((50, True), (95, False)):
                out.append((f"{w}x{h}-{sub}-q{q}", *pair(w, h, sub, q, seed=300 + 10 * i + j, smooth=smooth)))
    out.append(("33x19-grey", *pair(33, 19, "grey", 75, seed=401)))
    out.append(("70x46-420-rst3", *pair(70, 46, "420", 75, seed=402, restart_marker_blocks=3)))
    out.append(("200x150-420-q30", *pair(200, 150, "420", 30, seed=403, smooth=True)))
    return tuple(out)


def named(name):
    return next(p for p in pairs() if p[0] == name)


def check_pairs():
    """The eight (name, progressive, twin) of the stand-alone sanitizer program."""
    return [named("8x8-444-q50"), named("17x9-420-q95"), named("38x30-420-q50"), named("54x22-422-q95"),
            named("33x19-grey"), named("70x46-420-rst3"),
            ("24x24-444-q100", *pair(24, 24, "444", 100, seed=404)), named("200x150-420-q30")]


@functools.lru_cache(maxsize=None)
def resize_pairs():
    """(name, progressive, twin) of ``resize_cases``' sizes and settings."""
    spec = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (120, 90, "420"), (500, 375, "420"),
            (280, 260, "grey")]
    assert len(spec) == len(resize_cases())
    return tuple((f"{w}x{h}-{sub}", *pair(w, h, sub, 90, seed=50 + i, smooth=True)) for i, (w, h, sub) in enumerate(spec))


def patch_refinement_ah(data: bytes) -> bytes:
    """The file with the first refinement scan's Ah raised by one, so that Ah != Al + 1."""
    d = bytearray(data)
    at = 0
    while True:
        at = d.index(b"\xff\xda", at)
        ns = d[at + 4]
        ahal = at + 5 + 2 * ns + 2
        if d[ahal] >> 4:
            d[ahal] += 0x10
            return bytes(d)
        at += 2


def clobber_scan(data: bytes, which: int = 4) -> bytes:
    """The file with the entropy-coded bytes of scan ``which`` (an AC scan in Pillow's script)
    overwritten by one bits (FF 00 pairs: no marker among them).  No Huffman table assigns the
    all-ones code, so the scan's first symbol is refused."""
    d = bytearray(data)
    at = 0
    for _ in range(which + 1):
        at = d.index(b"\xff\xda", at) + 2
    start = at + (d[at] << 8 | d[at + 1])
    end = start
    while not (d[end] == 0xFF and d[end + 1] not in (0x00, 0xFF) and not 0xD0 <= d[end + 1] <= 0xD7):
        end += 1
    assert end - start >= 8
    d[start:end] = (b"\xff\x00" * (end - start))[:end - start - 1] + b"\x00"
    return bytes(d)
