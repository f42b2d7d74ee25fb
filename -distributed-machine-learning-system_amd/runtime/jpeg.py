"""JPEG decode for the image data path: native entropy decode on host threads,
IDCT + chroma upsampling + colour conversion + resize + crop on the GPU.

    bytes --(csrc/runtime/jpeg_entropy.cpp, std::threads, no GIL)--> int16 DCT
    coefficients --(HbmStager: pinned ping-pong, side stream)--> HBM
    --(kernels/jpeg_decode.hip: jpeg_idct, jpeg_resize_crop)--> uint8 [B,224,224,3]

With ``entropy_on="gpu"`` (opt-in) the Huffman streams are decoded on the device
as well, one lane per image, and the file bytes cross PCIe instead of the
coefficients (an eighth of the size):

    bytes --(csrc/runtime/jpeg_huff_pack.cpp: parse + pack, no GIL)--> packed
    bytes + tables + descriptors --(HbmStager)--> HBM --(kernels/jpeg_entropy.hip:
    memset, jpeg_entropy_kernel)--> int16 coefficients in HBM --> the same two kernels

``entropy_on="gpu_parallel"`` (opt-in as well) decodes one image on the many
lanes of a workgroup instead (self-synchronising sub-streams, csrc/jpeg_huff_par.h,
jpeg_entropy_par_kernel), so a small query no longer waits for one lane to walk
a whole stream; files with restart markers keep the one-lane kernel in the same
batch (unless ``restart="intervals"``, below).

``progressive="native"`` (opt-in, default ``"fallback"``) takes progressive
files in all three forms.  One marker walk over the whole file
(csrc/runtime/jpeg_entropy.cpp) turns its SOS segments into a scan script, and
one core (csrc/jpeg_huff_prog.h: DC / AC, first / refinement, EOB runs, restart
intervals) decodes it scan by scan into the same coefficient layout: on the
host threads, or on the device with one lane per image (jpeg_entropy_prog_kernel,
also under ``"gpu_parallel"``: there is no sub-stream form for progressive
scans).  Everything after the entropy stage is unchanged.

``restart="intervals"`` (opt-in, default ``"lane"``) decodes a baseline file
with a restart interval one interval per lane in both device forms
(csrc/jpeg_huff_rst.h, jpeg_entropy_rst_kernel): after every ``RSTn`` the
reader is byte-aligned, the DC predictors are zero and the MCU number is
known, so the packer finds the markers with one byte scan and every interval
is decoded by the serial decoder's own loop from the serial decoder's own
state.  With ``"lane"`` such a file is walked by one lane of the one-lane
kernel, whatever the form.

``sampling="native"`` (opt-in, default ``"fallback"``) takes two more chroma
layouts in all three forms: 4:4:0 (luma 1x2, what a 4:2:2 file becomes after
a lossless 90 degree rotation) as ``mode`` 3 and 4:1:1 (luma 4x1) as ``mode``
4.  The entropy cores take any sampling factors from the header; the colour
stage upsamples mode 3 with libjpeg's vertical triangle filter and mode 4 by
replication, as libjpeg-turbo does, on planes that an fp64 IDCT pass
(jpeg_idct_exact_kernel) has rewritten so that near-ties round as the model's.

``colorspace="auto"`` (opt-in, default ``"ycbcr"``) reads the colour model of a
file as libjpeg does: a three-component file with a JFIF APP0 is YCbCr; else
an Adobe APP14 decides (transform 0: RGB, else YCbCr); else the component
ids (``R``, ``G``, ``B``: RGB, anything else: YCbCr).  A four-component file
whose components are all sampled 1x1 is CMYK (no Adobe segment, or transform
0) or YCCK (transform 2).  RGB-coded files are decoded wherever their YCbCr
twins are; four-component files take the one-lane kernel (the progressive
kernel when progressive) in both device forms.  The colour stage of the
resize kernel hands RGB planes on as they are (planes 1 and 2 upsampled like
chroma) and converts CMYK / YCCK with the integer formula of Pillow's
``convert("RGB")``, on planes the fp64 IDCT pass has rewritten.  Under
the default ``"ycbcr"`` nothing of this is read: a four-component file is a
``"components"`` fallback, and an RGB-coded three-component file is decoded
as YCbCr, which gives wrong colours without a fallback being reported.

The chain reproduces what ``load_image_u8`` gets from libjpeg-turbo + Pillow
(fancy upsampling, YCbCr -> RGB, BILINEAR resize in two rounded passes, centre
crop) to within the tolerances of tests/test_jpeg_gpu.py.  Files the native
decoder does not take (progressive unless ``progressive="native"``,
non-interleaved baseline, arithmetic, 12-bit, CMYK / YCCK unless
``colorspace="auto"``, 4:4:0 / 4:1:1 unless
``sampling="native"``, any other odd sampling,
corrupt, not a JPEG at all) are decoded by ``load_image_u8`` on the host and
reported in ``info["fallbacks"]``; on a CPU device every image takes that
path.  ``reference_backend`` is the float64 numpy model of the GPU chain.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, replace

import numpy as np
import torch

from .data import HbmStager, load_image_u8

_STAGERS: dict = {}


def _C():
    from .. import ops

    ops.load()
    return ops


PROGRESSIVE = ("fallback", "native")
RESTART = ("lane", "intervals")
SAMPLING = ("fallback", "native")
COLORSPACE = ("ycbcr", "auto")
ENTROPY_ON = ("host", "gpu", "gpu_parallel")
# header["colorspace"]: what the samples of a file are
CS_YCBCR, CS_RGB, CS_CMYK, CS_YCCK = 0, 1, 2, 3

_ALLOWED = {"entropy_on": ENTROPY_ON, "progressive": PROGRESSIVE, "restart": RESTART, "sampling": SAMPLING,
            "colorspace": COLORSPACE}


def _check(name: str, value: str) -> str:
    if value not in _ALLOWED[name]:
        raise ValueError(f"{name} must be one of {_ALLOWED[name]}, not {value!r}")
    return value


@dataclass(frozen=True)
class Options:
    """What the decoder takes beyond the default (the module docstring says what
    each value means), validated on construction.  The ``native_*`` /
    ``restart_intervals`` properties are the booleans of the same names that
    ``ops.jpeg_parse``, ``ops.jpeg_entropy_batch`` and ``ops.jpeg_huff_pack`` take."""
    progressive: str = "fallback"
    restart: str = "lane"
    sampling: str = "fallback"
    colorspace: str = "ycbcr"

    def __post_init__(self):
        for name in ("progressive", "restart", "sampling", "colorspace"):
            _check(name, getattr(self, name))

    native_progressive = property(lambda self: self.progressive == "native")
    restart_intervals = property(lambda self: self.restart == "intervals")
    native_sampling = property(lambda self: self.sampling == "native")
    native_colorspace = property(lambda self: self.colorspace == "auto")

    @property
    def parse_flags(self) -> dict:
        """The keyword arguments of ``ops.jpeg_parse`` / ``ops.jpeg_entropy_batch`` (``restart`` plays no part there)."""
        return {"native_progressive": self.native_progressive, "native_sampling": self.native_sampling,
                "native_colorspace": self.native_colorspace}


def parse(data: bytes, progressive: str = "fallback", sampling: str = "fallback", colorspace: str = "ycbcr"):
    """Header of a JPEG the native decoder takes (dict: W, H, ncomp, mode,
    comp[i] = h, v, bw, bh, coef_off, q, progressive, nscans, colorspace), or
    the reason (str) it does not.  A progressive file is ``"progressive"``
    unless ``progressive="native"``; a 4:4:0 or 4:1:1 file is ``"sampling"``
    unless ``sampling="native"`` (then ``mode`` 3 or 4).  With
    ``colorspace="auto"`` the header's ``colorspace`` is 0 (YCbCr or grey), 1
    (RGB), 2 (CMYK) or 3 (YCCK) and a four-component file sampled 1x1 is taken;
    with the default ``"ycbcr"`` it is always 0, a four-component file is
    ``"components"`` and an RGB-coded file is decoded as YCbCr."""
    opts = Options(progressive=progressive, sampling=sampling, colorspace=colorspace)
    st, reason, hdr = _C().jpeg_parse(bytes(data), **opts.parse_flags)
    return hdr if st == 0 else reason


def entropy_decode(data: bytes, progressive: str = "fallback", sampling: str = "fallback", colorspace: str = "ycbcr"):
    """(header, int16 coefficients) of one image by the native host decoder, or
    the reason (str) it was refused.  ``colorspace``: as for ``parse``."""
    opts = Options(progressive=progressive, sampling=sampling, colorspace=colorspace)
    data = bytes(data)
    status, _, coefs, offs = _C().jpeg_entropy_batch([data], 1, **opts.parse_flags)
    if status[0] != 0:
        return _refusal(_C(), data, status[0], opts)
    return parse(data, progressive, sampling, colorspace), coefs.numpy()


# ---- float64 model of the GPU chain ------------------------------------------------

def _idct_matrix() -> np.ndarray:
    x = np.arange(8)[:, None]
    u = np.arange(8)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[:, 0] *= np.sqrt(0.5)
    return m                       # [sample, frequency]


def _round_u8(a: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(a + 0.5), 0, 255)


def _upsample_h2v1(p: np.ndarray) -> np.ndarray:
    p = p.astype(np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _upsample_h2v2(p: np.ndarray) -> np.ndarray:
    p = p.astype(np.int32)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    t = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    t[0::2] = 3 * p + above
    t[1::2] = 3 * p + below
    left = np.concatenate([t[:, :1], t[:, :-1]], 1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int32)
    out[:, 0::2] = (3 * t + left + 8) >> 4
    out[:, 1::2] = (3 * t + right + 7) >> 4
    out[:, 0] = (4 * t[:, 0] + 8) >> 4
    out[:, -1] = (4 * t[:, -1] + 7) >> 4
    return out


def _upsample_h1v2(p: np.ndarray) -> np.ndarray:
    p = p.astype(np.int32)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    out[0::2] = (3 * p + above + 1) >> 2
    out[1::2] = (3 * p + below + 2) >> 2
    return out


def _muldiv255(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Pillow's MULDIV255 on integer arrays: a * b / 255 rounded half up."""
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def reference_backend(header: dict, coeffs: np.ndarray) -> np.ndarray:
    """Full-resolution RGB uint8 [H, W, 3] from a header and its coefficients:
    exact IDCT in float64, planes cut to their downsampled size, libjpeg's
    fancy upsampling (mode 4, h4v1: replication, libjpeg has no filter for
    it), colour conversion rounded half up.  ``header["colorspace"]`` picks
    the colour stage: YCbCr (0; a header parsed under the default always says
    so), RGB (1: the upsampled planes as they are), CMYK (2) and YCCK (3) as
    Pillow converts them, ``nk - MULDIV255(c, nk)`` with ``nk`` the fourth
    plane and ``c`` 255 minus a plane (CMYK) or the R', G', B' of planes 0..2
    (YCCK), in integers."""
    W, H = header["W"], header["H"]
    hmax, vmax = header["hmax"], header["vmax"]
    m = _idct_matrix()
    planes = []
    for c in header["comp"]:
        bw, bh = c["bw"], c["bh"]
        f = np.asarray(coeffs[c["coef_off"]:c["coef_off"] + bw * bh * 64], np.float64).reshape(bh, bw, 8, 8)
        f = f * np.asarray(c["q"], np.float64).reshape(8, 8)
        px = np.einsum("yv,abvu,xu->aybx", m, f, m).reshape(bh * 8, bw * 8)
        cw, ch = -(-W * c["h"] // hmax), -(-H * c["v"] // vmax)
        planes.append(_round_u8(px + 128.0)[:ch, :cw])
    y = planes[0]
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    up = {0: lambda p: p, 1: _upsample_h2v1, 2: _upsample_h2v2, 3: _upsample_h1v2,
          4: lambda p: np.repeat(p, 4, 1)}[header["mode"]]
    cs = header.get("colorspace", CS_YCBCR)
    if cs == CS_RGB and header["mode"] in (1, 2) and planes[1].shape[1] <= 2:
        # libjpeg filters a half-width plane only when it is more than two samples wide, else it
        # replicates; a YCbCr pixel dilutes the difference, an RGB plane is the pixel
        up = lambda p, v=header["mode"]: np.repeat(np.repeat(p, 2, 1), v, 0)
    p1, p2 = up(planes[1])[:H, :W], up(planes[2])[:H, :W]
    if cs == CS_RGB:
        return np.stack([y, p1, p2], 2).astype(np.uint8)
    if cs == CS_CMYK:
        nk = planes[3].astype(np.int64)
        return np.stack([nk - _muldiv255(255 - p.astype(np.int64), nk) for p in (y, p1, p2)], 2).astype(np.uint8)
    cb = p1.astype(np.float64) - 128.0
    cr = p2.astype(np.float64) - 128.0
    rgb = _round_u8(np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], 2))
    if cs == CS_YCCK:
        nk = planes[3].astype(np.int64)[:, :, None]
        rgb = nk - _muldiv255(rgb.astype(np.int64), nk)
    return rgb.astype(np.uint8)


def _bilinear_weights(n_in: int, n_out: int) -> np.ndarray:
    """Pillow's BILINEAR as a [n_out, n_in] matrix (rows sum to 1)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    w = np.zeros((n_out, n_in))
    for i in range(n_out):
        centre = (i + 0.5) * scale
        lo, hi = max(0, int(centre - fs + 0.5)), min(n_in, int(centre + fs + 0.5))
        x = np.arange(lo, hi)
        k = np.maximum(0.0, 1.0 - np.abs((x - centre + 0.5) / fs))
        w[i, lo:hi] = k / k.sum()
    return w


def resize_geometry(w: int, h: int, resize: int, crop: int):
    """(nw, nh, left, top) by the expressions of ``load_image_u8``."""
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nh, nw = resize, int(resize * w / h)
    return nw, nh, int(round((nw - crop) / 2.0)), int(round((nh - crop) / 2.0))


def reference_resize_crop(rgb: np.ndarray, resize: int = 256, crop: int = 224) -> np.ndarray:
    """The model's Resize + CenterCrop: horizontal pass, then vertical pass, each
    rounded half up to uint8; a pass between equal sizes is the identity."""
    h, w = rgb.shape[:2]
    nw, nh, left, top = resize_geometry(w, h, resize, crop)
    a = rgb.astype(np.float64)
    if nw != w:
        a = _round_u8(np.einsum("ox,yxc->yoc", _bilinear_weights(w, nw), a))
    if nh != h:
        a = _round_u8(np.einsum("oy,yxc->oxc", _bilinear_weights(h, nh), a))
    out = np.zeros((crop, crop, 3), np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(top + crop, nh), max(left, 0), min(left + crop, nw)
    out[y0 - top:y1 - top, x0 - left:x1 - left] = a[y0:y1, x0:x1].astype(np.uint8)
    return out


# ---- the batch decoder ----------------------------------------------------------------

def _pil_full(data: bytes) -> np.ndarray:
    import io

    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def _stager(device: torch.device) -> HbmStager:
    st = _STAGERS.get(device)
    if st is None:
        st = _STAGERS[device] = HbmStager(device)
    return st


_DEVICE_FORMS = ("gpu", "gpu_parallel")
_UNSYNCED = 100           # kJpegHuffUnsynced: the sub-stream kernel's rounds hit their cap (device-only status)


def _refusal(C, data: bytes, status: int, opts: Options) -> str:
    """Why an entry is a fallback: the parse's reason (under the options the batch
    was decoded with), else what the entropy stage said."""
    st, reason, _ = C.jpeg_parse(data, **opts.parse_flags)
    if st != 0:
        return reason
    return "unsynced" if status == _UNSYNCED else "corrupt"


def _header_column(hdr, byte_offset: int) -> np.ndarray:
    """One int field of every row of ``hdr`` (uint8 [n, sizeof(JpegHeader)]) by its
    byte offset in the struct (``W`` 0, ``H`` 4, ``ops.JPEG_HEADER_*_OFFSET``)."""
    return hdr.numpy().view(np.int32)[:, byte_offset // 4]


@dataclass(frozen=True)
class Entropy:
    """What ``entropy_batch`` prepared and ``decode_batch(..., entropy=)`` takes."""
    form: str                 # the ``entropy_on`` it was prepared in
    datas: list               # the entries as ``bytes | None``
    options: Options          # what it was prepared with (the host form does nothing with ``restart``)
    status: list              # per entry: the host decoder's verdict; in the device forms the parse's
    hdr: torch.Tensor         # uint8 [n, sizeof(JpegHeader)]
    offs: list                # first coefficient of each entry whose header parsed, else -1
    coef_elems: int           # int16 elements of the batch's coefficients
    coefs: torch.Tensor | None    # host form: the coefficients (CPU)
    packed: object | None         # device forms: the ``JpegHuffPacked`` of ``ops.jpeg_huff_pack``
    seconds: float            # wall seconds of the decode (host form) or of parse + pack


def entropy_batch(datas, threads: int = 8, entropy_on: str = "host", progressive: str = "fallback",
                  restart: str = "lane", sampling: str = "fallback", colorspace: str = "ycbcr"):
    """The host half of ``decode_batch`` for a GPU device: the native Huffman
    decode of a list of ``bytes | None`` on ``threads`` threads (the GIL is
    released, so a caller may run it under the previous batch's copy and
    kernels).  With ``entropy_on="gpu"`` or ``"gpu_parallel"`` it only parses the
    headers and packs bytes, tables and descriptors for the entropy kernels (one
    thread, GIL released as well).  ``progressive="native"`` takes progressive
    files in either form; ``restart="intervals"`` packs one work item per
    restart interval for the interval kernel in the two device forms (the host
    form is unchanged by it); ``sampling="native"`` takes 4:4:0 and 4:1:1 files
    in every form; ``colorspace="auto"`` classifies RGB-coded files and takes
    1x1 CMYK / YCCK files in every form (under the default every
    three-component file counts as YCbCr, an RGB-coded one included).  Returns
    an ``Entropy``, which remembers the form and the options."""
    _check("entropy_on", entropy_on)
    opts = Options(progressive, restart, sampling, colorspace)
    datas = [None if d is None else bytes(d) for d in datas]
    t0 = time.perf_counter()
    if entropy_on in _DEVICE_FORMS:
        packed = _C().jpeg_huff_pack(datas, entropy_on == "gpu_parallel", opts.native_progressive,
                                     opts.restart_intervals, opts.native_sampling, opts.native_colorspace)
        return Entropy(entropy_on, datas, opts, list(packed.status), packed.hdr, list(packed.offs),
                       int(packed.coef_total), None, packed, time.perf_counter() - t0)
    status, hdr, coefs, offs = _C().jpeg_entropy_batch(datas, int(threads), **opts.parse_flags)
    return Entropy("host", datas, opts, list(status), hdr, list(offs), coefs.numel(), coefs, None,
                   time.perf_counter() - t0)


def _entropy_on_device(C, packed, device, cur, stager: HbmStager, info: dict):
    """Packed bytes through the stager's side stream, memset, entropy kernel on
    ``cur``: (device coefficients int16, device status int32 [n]); fills
    ``h2d_s`` / ``h2d_bytes`` / ``entropy_s`` of ``info`` once the caller has
    synchronised, through the returned closure."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record(stager.stream)
    dev_bytes, done = stager._stage(packed.bytes.numpy(), (packed.byte_total,))
    ev[1].record(stager.stream)
    if done is not None:
        cur.wait_event(done)
    dev_bytes.record_stream(cur)
    dev_coefs = torch.empty(packed.coef_total, dtype=torch.int16, device=device)
    dev_status = torch.zeros(packed.n, dtype=torch.int32, device=device)
    C.jpeg_entropy_zero(dev_coefs)
    ev[2].record(cur)
    if packed.parallel:
        # the rounds' per-sub-stream state of the images too long for LDS; no need to zero it
        scratch = torch.empty(max(int(packed.scratch_total), 1), dtype=torch.int32, device=device)
        C.jpeg_entropy_gpu_parallel(packed, dev_bytes, dev_coefs, dev_status, scratch)
    else:
        C.jpeg_entropy_gpu(packed, dev_bytes, dev_coefs, dev_status)
    ev[3].record(cur)

    def times():
        info["h2d_s"] = ev[0].elapsed_time(ev[1]) * 1e-3
        info["h2d_bytes"] = int(packed.byte_total)
        info["entropy_s"] = ev[2].elapsed_time(ev[3]) * 1e-3
    return dev_coefs, dev_status, times


def entropy_coefs(datas, device="cpu", entropy_on: str = "host", threads: int = 8, progressive: str = "fallback",
                  restart: str = "lane", sampling: str = "fallback", colorspace: str = "ycbcr"):
    """Debug helper: the entropy stage alone.  ``(status, offs, coefs)``: one
    status per entry (0: decoded), the first coefficient of each entry whose
    header parsed in ``coefs`` (-1: none) and the batch's int16 coefficients as a CPU tensor,
    from the host decoder or, with ``entropy_on="gpu"`` / ``"gpu_parallel"`` on a
    GPU ``device``, from the entropy kernels.  The four options: as for
    ``entropy_batch``."""
    _check("entropy_on", entropy_on)
    Options(progressive, restart, sampling, colorspace)
    if entropy_on in _DEVICE_FORMS:
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"entropy_on={entropy_on!r} needs a GPU device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
    ent = entropy_batch(datas, threads, entropy_on, progressive, restart, sampling, colorspace)
    if ent.packed is None:
        return ent.status, ent.offs, ent.coefs
    status, coefs = ent.status, torch.zeros(ent.coef_elems, dtype=torch.int16)
    if ent.packed.n_gpu:
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream(device)
            dev_coefs, dev_status, _ = _entropy_on_device(_C(), ent.packed, device, cur, _stager(device), {})
            cur.synchronize()
            coefs = dev_coefs.cpu()
            for i, st in enumerate(dev_status.cpu().tolist()):
                if status[i] == 0:
                    status[i] = int(st)
    return status, ent.offs, coefs


def decode_batch(datas, device, resize: int | None = 256, crop: int | None = 224, threads: int = 8,
                 stager: HbmStager | None = None, entropy=None, entropy_on: str = "host",
                 progressive: str = "fallback", restart: str = "lane", sampling: str = "fallback",
                 colorspace: str = "ycbcr"):
    """Decode a list of ``bytes | None`` into a uint8 tensor [B, crop, crop, 3] on
    ``device`` (``None`` entries: zero images).  With ``resize=None`` nothing is
    resized or cropped and the result is a list of [H, W, 3] tensors (``None``
    for a ``None`` entry).  Returns ``(images, info)``; ``info["fallbacks"]``
    lists ``(index, reason)`` of the entries ``load_image_u8`` decoded on the
    host, ``entropy_s`` / ``h2d_s`` / ``idct_s`` / ``resize_s`` / ``kernel_s``
    the seconds of the native Huffman decode (wall), the coefficient copy and
    the kernels (device events).  ``entropy``: the result of ``entropy_batch``
    on the same ``datas``, when the caller ran that ahead.

    ``entropy_on="gpu"`` moves the Huffman decode to the device (default
    ``"host"``; ignored on a CPU device, and when ``entropy`` was prepared the
    form it was prepared in decides): the host only parses headers and packs,
    ``h2d_s`` is then the copy of the file bytes (``info["h2d_bytes"]``),
    ``entropy_s`` the entropy kernel's device-event time and ``pack_s`` the
    host's parse + pack (wall).  An image the kernel flags is a ``"corrupt"``
    fallback exactly like one the host decoder refuses.  ``info["entropy_on"]``
    names the form in effect (on a CPU device: the one asked for; nothing
    native runs there).

    ``entropy_on="gpu_parallel"`` is the same with one workgroup per image
    (sub-streams that synchronise themselves, csrc/jpeg_huff_par.h); files with
    restart markers take the one-lane kernel inside the same batch.  An image
    whose sub-streams did not synchronise within the kernel's round cap is an
    ``"unsynced"`` fallback.

    ``progressive``, ``restart``, ``sampling`` and ``colorspace``: the module
    docstring says what each value takes and which kernel decodes it.  When
    ``entropy`` was prepared, the form and the options it was prepared with
    decide, not the arguments here, and ``info["entropy_on"]``,
    ``info["progressive"]``, ``info["restart"]``, ``info["sampling"]`` and
    ``info["colorspace"]`` name what is in effect; only ``info["restart"]`` of
    an ``entropy`` prepared in the host form is the one asked for here (the
    host form does nothing with it).  On a CPU device nothing native runs.

    ``progressive="native"`` (default ``"fallback"``: a progressive file goes
    to ``load_image_u8`` with the reason ``"progressive"``) decodes progressive
    files of a supported layout (8-bit, 1 or 3 components, 4:4:4 / 4:2:2 /
    4:2:0, Huffman, at most ``JPEG_PROG_MAX_SCANS`` scans) natively in every
    ``entropy_on`` form.  They hold the coefficients of their baseline twins,
    so the IDCT and resize kernels see no difference.  A progressive file the
    decoder or kernel refuses is then a ``"corrupt"`` fallback, one with more
    scans a ``"multiscan"`` one.  ``info["progressive_images"]`` counts the
    progressive files decoded natively.  Non-interleaved baseline files
    (``"multiscan"``), arithmetic coding, 12-bit samples and CMYK remain
    fallbacks.

    ``restart="intervals"`` (default ``"lane"``: a baseline file with a restart
    interval is walked by one lane of the one-lane kernel in both device forms)
    decodes such a file one restart interval per lane in ``"gpu"`` and
    ``"gpu_parallel"``; the packer finds the ``RSTn`` markers, and a file that
    lacks one stays with the one-lane kernel, which refuses it.  An image one of
    whose intervals is refused is a ``"corrupt"`` fallback like any other.
    Progressive files with restart markers stay on the progressive kernel.
    ``info["restart_images"]`` counts the images the interval kernel decoded
    and did not flag.

    ``sampling="native"`` (default ``"fallback"``: a 4:4:0 or 4:1:1 file goes
    to ``load_image_u8`` with the reason ``"sampling"``) decodes those two
    layouts (header ``mode`` 3 and 4) natively in every ``entropy_on`` form,
    baseline, restart-interval and progressive alike.  Every other layout
    stays a ``"sampling"`` fallback.  ``info["sampling_images"]`` counts the
    mode-3 and mode-4 images decoded natively and not flagged.

    ``colorspace="auto"`` (default ``"ycbcr"``) decodes RGB-coded files and
    four-component files sampled 1x1 (CMYK, YCCK), baseline or (with
    ``progressive="native"``) progressive, with or without restart markers.
    A four-component file with an Adobe transform other than 0 or 2 stays a
    ``"components"`` fallback and any other four-component sampling is a
    ``"sampling"`` one; four-component files take the one-lane kernel (or the
    progressive one) under ``"gpu"``, ``"gpu_parallel"`` and
    ``restart="intervals"`` alike.  Under the default every four-component
    file is a ``"components"`` fallback and an RGB-coded three-component file
    is decoded as YCbCr: its colours are wrong and no fallback is reported.
    ``info["colorspace_images"]`` counts the RGB / CMYK / YCCK images decoded
    natively and not flagged."""
    _check("entropy_on", entropy_on)
    opts = Options(progressive, restart, sampling, colorspace)
    device = torch.device(device)
    full = resize is None
    n = len(datas)
    if entropy is None:
        form = entropy_on
        datas = [None if d is None else bytes(d) for d in datas]
    else:
        # the form and the options the entropy stage was prepared with decide
        form, datas = entropy.form, entropy.datas
        opts = entropy.options if form in _DEVICE_FORMS else replace(entropy.options, restart=restart)
    on_gpu = form in _DEVICE_FORMS
    info = {"fallbacks": [], "entropy_s": 0.0, "h2d_s": 0.0, "idct_s": 0.0, "resize_s": 0.0, "kernel_s": 0.0,
            "gpu_images": 0, "entropy_on": form, "progressive": opts.progressive, "progressive_images": 0,
            "restart": opts.restart, "restart_images": 0, "sampling": opts.sampling, "sampling_images": 0,
            "colorspace": opts.colorspace, "colorspace_images": 0}
    host = (lambda d: _pil_full(d)) if full else (lambda d: load_image_u8(d, resize, crop))
    if device.type != "cuda":
        # no GPU: every image through Pillow, nothing of the native path
        info["fallbacks"] = [(i, "cpu_device") for i, d in enumerate(datas) if d is not None]
        imgs = [None if d is None else torch.from_numpy(host(d).copy()) for d in datas]
        if full:
            return imgs, info
        out = torch.zeros((n, crop, crop, 3), dtype=torch.uint8)
        for i, t in enumerate(imgs):
            if t is not None:
                out[i] = t
        return out, info

    C = _C()
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if entropy is None:
        entropy = entropy_batch(datas, threads, form, opts.progressive, opts.restart, opts.sampling, opts.colorspace)
    info["pack_s" if on_gpu else "entropy_s"] = entropy.seconds
    status, hdr, offs, coef_elems = list(entropy.status), entropy.hdr, entropy.offs, entropy.coef_elems
    coefs, packed = entropy.coefs, entropy.packed
    ws, hs = _header_column(hdr, 0), _header_column(hdr, 4)      # JpegHeader starts with int W, H
    geom = None
    if not full:
        seen: dict = {}                           # datasets repeat a few sizes: one evaluation per size
        rows = [(0, 0, 0, 0)] * n
        for i in range(n):
            if status[i] == 0:
                wh = (int(ws[i]), int(hs[i]))
                g = seen.get(wh)
                if g is None:
                    g = seen[wh] = resize_geometry(wh[0], wh[1], resize, crop)
                rows[i] = g
        geom = torch.tensor(rows, dtype=torch.int64).view(n, 4)
    with torch.cuda.device(device):
        cur = torch.cuda.current_stream(device)
        plan = C.jpeg_plan(hdr, status, offs, coef_elems, geom, 0 if full else int(crop), device)
        out = torch.zeros(max(plan.out_bytes, 0) if full else n * crop * crop * 3, dtype=torch.uint8, device=device)
        if plan.n_gpu:
            stager = stager or _stager(device)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            if on_gpu:
                dev_coefs, dev_status, entropy_times = _entropy_on_device(C, packed, device, cur, stager, info)
            else:
                ev[0].record(stager.stream)
                dev_coefs, done = stager._stage(coefs.numpy(), (coefs.numel() * 2,))
                ev[1].record(stager.stream)
                cur.wait_event(done)
                dev_coefs.record_stream(cur)
            planes = torch.empty(plan.plane_bytes, dtype=torch.uint8, device=device)
            ev[2].record(cur)
            C.jpeg_idct(plan, dev_coefs.view(torch.int16), planes)
            ev[3].record(cur)
            C.jpeg_resize_crop(plan, planes, out)
            ev[4].record(cur)
            ev[4].synchronize()
            info["gpu_images"] = int(plan.n_gpu)
            if on_gpu:
                entropy_times()
                # the kernel's verdicts: a flagged image was planned and run through the two kernels on
                # whatever it decoded before the flag (bounded, like any coefficients); the fallback loop
                # below overwrites its output
                for i, st in enumerate(dev_status.cpu().tolist()):
                    if status[i] == 0 and st != 0:
                        status[i] = int(st)
                        info["gpu_images"] -= 1
                if packed.n_rst:
                    # column 0 of the work items: the entries the interval kernel took
                    info["restart_images"] = sum(1 for i in set(packed.rst_items[:, 0].tolist()) if status[i] == 0)
            else:
                info["h2d_s"] = ev[0].elapsed_time(ev[1]) * 1e-3
            info["idct_s"] = ev[2].elapsed_time(ev[3]) * 1e-3
            info["resize_s"] = ev[3].elapsed_time(ev[4]) * 1e-3
            info["kernel_s"] = info["idct_s"] + info["resize_s"]
        imgs = []
        if not full:
            out = out.view(n, crop, crop, 3)
        for i, d in enumerate(datas):
            if d is None:
                imgs.append(None)
                continue
            if status[i] != 0:
                info["fallbacks"].append((i, _refusal(C, d, status[i], opts)))
                t = torch.from_numpy(host(d).copy()).to(device)
                if full:
                    imgs.append(t)
                else:
                    out[i].copy_(t)
            elif full:
                h, w = int(hs[i]), int(ws[i])
                o = plan.out_off[i]
                imgs.append(out[o:o + h * w * 3].view(h, w, 3))
        if n:
            # one pass over the header rows for the three counters: an option's images are those it is on
            # for, that were decoded natively and not flagged, and whose header field says so (progressive
            # is 0 / 1, mode 0..4, colorspace 0..3, never negative: "set" is ">= 1", modes 3 and 4 ">= 3")
            taken = np.array([status[i] == 0 and datas[i] is not None for i in range(n)])
            for key, on, offset, least in (
                    ("progressive_images", opts.native_progressive, C.JPEG_HEADER_PROGRESSIVE_OFFSET, 1),
                    ("sampling_images", opts.native_sampling, C.JPEG_HEADER_MODE_OFFSET, 3),
                    ("colorspace_images", opts.native_colorspace, C.JPEG_HEADER_COLORSPACE_OFFSET, 1)):
                if on:
                    info[key] = int(np.count_nonzero(taken & (_header_column(hdr, offset) >= least)))
        # the result is complete when it is returned, whatever the batch held (the zero fill and
        # the fallbacks' copies too): a holder may hand it to a consumer on any other stream
        cur.synchronize()
    return (imgs if full else out), info
