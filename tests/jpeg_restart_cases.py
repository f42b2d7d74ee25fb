"""Baseline JPEGs with a restart interval for the tests of ``restart="intervals"``
(seeded, no fixture files): the files, how many intervals each holds, and the
mutants made at a file's first RST0."""
import functools

from jpeg_cases import encode

# (w, h, sub, Pillow save option, intervals): every file is encode(w, h, sub, 75, seed=1, **kw)
SPEC = [
    (70, 46, "420", {"restart_marker_blocks": 1}, 15),      # the index wraps past RST7
    (70, 46, "420", {"restart_marker_blocks": 3}, 5),       # intervals cross MCU rows (mcux = 5)
    (70, 46, "420", {"restart_marker_blocks": 4}, 4),       # a short last interval
    (70, 46, "420", {"restart_marker_blocks": 100}, 1),     # DRI without markers
    (54, 22, "422", {"restart_marker_blocks": 2}, 6),
    (17, 9, "444", {"restart_marker_blocks": 1}, 6),
    (33, 19, "grey", {"restart_marker_blocks": 2}, 8),
    (8, 8, "444", {"restart_marker_blocks": 1}, 1),
    (200, 150, "420", {"restart_marker_blocks": 1}, 130),   # more than two waves
    (200, 150, "420", {"restart_marker_rows": 1}, 10),
]


@functools.lru_cache(maxsize=None)
def table():
    """((file, intervals), ...) in the order of SPEC."""
    return tuple((encode(w, h, sub, 75, seed=1, **kw), k) for w, h, sub, kw, k in SPEC)


def files():
    return [d for d, _ in table()]


def small_files():
    """The table without the two 200x150 files (the stand-alone program's inputs)."""
    return [d for (d, _), s in zip(table(), SPEC) if (s[0], s[1]) != (200, 150)]


def markers(data: bytes):
    """Offsets of the in-sequence RSTn markers of the scan, by the reader's byte rules
    (FF 00 data, FF FF fill), up to the first other marker."""
    p = data.index(b"\xff\xda")
    p += 2 + (data[p + 2] << 8 | data[p + 3])
    out = []
    while p + 1 < len(data):
        if data[p] != 0xFF:
            p += 1
        elif data[p + 1] == 0xFF:
            p += 1
        elif data[p + 1] == 0x00:
            p += 2
        elif data[p + 1] == 0xD0 + (len(out) & 7):
            out.append(p)
            p += 2
        else:
            break
    return out


def first_rst0(data: bytes) -> int:
    return data.index(b"\xff\xd0", data.index(b"\xff\xda"))


def mutant_fill(data: bytes) -> bytes:
    """An extra FF in front of the first RST0 (a fill byte): still accepted."""
    at = first_rst0(data)
    return data[:at] + b"\xff" + data[at:]


def refused_mutants(data: bytes):
    """(name, bytes) of the four files the host decoder refuses: RST0 replaced by RST1, the
    marker removed, a 55 byte in front of it, the file cut one byte into it."""
    at = first_rst0(data)
    return [("rst1", data[:at + 1] + b"\xd1" + data[at + 2:]),
            ("removed", data[:at] + data[at + 2:]),
            ("data-byte", data[:at] + b"\x55" + data[at:]),
            ("cut", data[:at + 1])]
