"""One mixed batch for the tests of the decoder's options taken together (seeded, no fixture
files): every file kind the four opt-ins tell apart, a PNG and a ``None``.

Each entry is ``(name, bytes | None, needs, kind)``: ``needs`` the options without which the
parser refuses the file, a subset of {"progressive", "sampling", "colorspace"}; ``kind`` what
routes it in the packer: "baseline", "restart", "progressive" or "four" (four components,
baseline).  The RGB-coded file needs nothing: without ``colorspace`` it is taken for YCbCr."""
import functools
import itertools

import jpeg_color_cases
import jpeg_sampling_cases
from jpeg_cases import encode, png
from jpeg_entropy_cases import rst1
from jpeg_prog_cases import pair

PARSER_OPTIONS = ("progressive", "sampling", "colorspace")
P, S, C = PARSER_OPTIONS
PNG, NONE = 9, 10                      # their places in the batch
NOT_JPEG, EMPTY = 2, 1                 # their statuses, whatever the options


@functools.lru_cache(maxsize=None)
def batch():
    return (("420-17x9", encode(17, 9, "420", 75, seed=1), frozenset(), "baseline"),
            ("420-70x46-rst1", rst1(), frozenset(), "restart"),
            ("p420-17x9", pair(17, 9, seed=2)[0], frozenset({P}), "progressive"),
            ("440-17x9-q95", jpeg_sampling_cases.named("440-17x9-q95")[1], frozenset({S}), "baseline"),
            ("440-70x46-rst2", jpeg_sampling_cases.named("440-70x46-rst2")[1], frozenset({S}), "restart"),
            ("p440", jpeg_sampling_cases.progressive_cases()[0][1], frozenset({P, S}), "progressive"),
            ("cmyk-17x9", jpeg_color_cases.make("cmyk", 17, 9)[0], frozenset({C}), "four"),
            ("rgb420-17x9", jpeg_color_cases.make("rgb420", 17, 9)[0], frozenset(), "baseline"),
            ("p-cmyk", jpeg_color_cases.progressive_cases()[0][1], frozenset({P, C}), "progressive"),
            ("png", png(), None, None),
            ("none", None, None, None))


def datas():
    return [e[1] for e in batch()]


def jpegs():
    """(index, name, bytes, needs, kind) of the JPEG entries."""
    return [(i, *e) for i, e in enumerate(batch()) if e[2] is not None]


def subsets(names):
    return [frozenset(c) for k in range(len(names) + 1) for c in itertools.combinations(names, k)]


def verdict(needs, enabled):
    """(status is 0, reason) the parser must give a file that needs ``needs`` under ``enabled``."""
    missing = needs - enabled
    return not missing, "ok" if not missing else "progressive" if P in missing else "sampling" if S in missing else "components"


def strings(enabled):
    """The keyword arguments of runtime/jpeg.py for a set of enabled options ("restart" among them)."""
    return {"progressive": "native" if P in enabled else "fallback", "restart": "intervals" if "restart" in enabled else "lane",
            "sampling": "native" if S in enabled else "fallback", "colorspace": "auto" if C in enabled else "ycbcr"}
