"""Inputs shared by the tests of the device entropy stage (seeded, no fixture files)."""
from jpeg_cases import encode


def rst1() -> bytes:
    """70x46 4:2:0, a restart marker after every MCU: 14 markers, the index wraps past RST7."""
    return encode(70, 46, "420", 75, seed=11, restart_marker_blocks=1)


def noise_q100() -> bytes:
    """Random noise at quality 100: Huffman codes longer than the 9-bit lookahead table."""
    return encode(48, 40, "444", 100, seed=12)


def scan_mutant() -> bytes:
    """A good file whose scan is cut short by an EOI marker written into its middle:
    both decoders run out of data and refuse it as corrupt."""
    d = bytearray(encode(64, 48, "420", 75, seed=13, smooth=True))
    at = d.index(b"\xff\xda") + (len(d) - d.index(b"\xff\xda")) // 2
    d[at:at + 2] = b"\xff\xd9"
    return bytes(d)
