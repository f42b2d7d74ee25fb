"""Seeded Pillow-encoded JPEG inputs shared by the JPEG tests (no fixture files)."""
import io

import numpy as np
from PIL import Image

# the issue's sizes: 70x46, 38x30 and 54x22 are even sizes whose half is no multiple of 8
# (the chroma planes must be cut to their downsampled size before upsampling)
FULL_SIZES = [(8, 8), (16, 16), (17, 9), (67, 45), (64, 48), (70, 46), (38, 30), (54, 22)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}

# bounds of the issue at full resolution and after resize + crop
MAX_MODEL, MAX_GPU, MEAN_BOUND = 3, 4, 0.13


def pixels(w: int, h: int, seed: int, smooth: bool = False) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 6.28, 3)
    a = [127.5 + 100 * np.sin(xx / (7.0 + 3 * c) + ph[c]) * np.cos(yy / (11.0 - 2 * c)) for c in range(3)]
    return np.clip(np.stack(a, 2) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(w: int, h: int, sub: str = "420", quality: int = 75, seed: int = 0, smooth: bool = False, **kw) -> bytes:
    """One JPEG; ``sub`` "444" / "422" / "420" / "grey"; kw: Pillow save options."""
    a = pixels(w, h, seed, smooth)
    buf = io.BytesIO()
    if sub == "grey":
        Image.fromarray(a[:, :, 0], "L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a, "RGB").save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[sub], **kw)
    return buf.getvalue()


def full_res_cases():
    """(name, bytes): every size x {4:4:4, 4:2:2, 4:2:0} x quality {50, 95}, one
    grey image, one with restart markers, one with optimised tables."""
    out = []
    for i, (w, h) in enumerate(FULL_SIZES):
        for j, sub in enumerate(SUBSAMPLING):
            for q in (50, 95):
                out.append((f"{w}x{h}-{sub}-q{q}", encode(w, h, sub, q, seed=100 * i + 10 * j + q, smooth=(i + j) % 2 == 0)))
    out.append(("67x45-grey", encode(67, 45, "grey", 75, seed=7)))
    out.append(("70x46-420-rst3", encode(70, 46, "420", 75, seed=8, restart_marker_blocks=3)))
    out.append(("67x45-422-opt", encode(67, 45, "422", 75, seed=9, optimize=True)))
    return out


def resize_cases():
    """(name, bytes) of the resize + crop test, smooth images at quality 90."""
    spec = [(333, 250, "420"), (250, 333, "422"), (256, 256, "444"), (120, 90, "420"), (500, 375, "420"),
            (280, 260, "grey")]
    return [(f"{w}x{h}-{sub}", encode(w, h, sub, 90, seed=50 + i, smooth=True)) for i, (w, h, sub) in enumerate(spec)]


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def progressive() -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels(48, 40, 3, True), "RGB").save(buf, "JPEG", quality=80, progressive=True)
    return buf.getvalue()


def cmyk() -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels(40, 32, 4, True), "RGB").convert("CMYK").save(buf, "JPEG", quality=80)
    return buf.getvalue()


def png() -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels(300, 280, 5, True), "RGB").save(buf, "PNG")
    return buf.getvalue()


def diff_stats(a: np.ndarray, b: np.ndarray):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int(d.max()), float(d.mean())
