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
resize kernel hands RGB planes on as they are and converts CMYK / YCCK with
Pillow's integer formula, on planes the fp64 IDCT pass has rewritten.  Under
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

import numpy as np
import torch

from .data import HbmStager, load_image_u8

_STAGERS: dict = {}


def _C():
    from .. import ops

    ops.load()
    return ops


PROGRESSIVE = ("fallback", "native")


def _check_progressive(progressive: str) -> str:
    if progressive not in PROGRESSIVE:
        raise ValueError(f"progressive must be one of {PROGRESSIVE}, not {progressive!r}")
    return progressive


RESTART = ("lane", "intervals")


def _check_restart(restart: str) -> str:
    if restart not in RESTART:
        raise ValueError(f"restart must be one of {RESTART}, not {restart!r}")
    return restart


SAMPLING = ("fallback", "native")


def _check_sampling(sampling: str) -> str:
    if sampling not in SAMPLING:
        raise ValueError(f"sampling must be one of {SAMPLING}, not {sampling!r}")
    return sampling


COLORSPACE = ("ycbcr", "auto")
# header["colorspace"]: what the samples of a file are
CS_YCBCR, CS_RGB, CS_CMYK, CS_YCCK = 0, 1, 2, 3


def _check_colorspace(colorspace: str) -> str:
    if colorspace not in COLORSPACE:
        raise ValueError(f"colorspace must be one of {COLORSPACE}, not {colorspace!r}")
    return colorspace


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
    native = _check_progressive(progressive) == "native"
    samp = _check_sampling(sampling) == "native"
    color = _check_colorspace(colorspace) == "auto"
    st, reason, hdr = _C().jpeg_parse_colorspace(bytes(data), native, samp, color)
    return hdr if st == 0 else reason


def entropy_decode(data: bytes, progressive: str = "fallback", sampling: str = "fallback", colorspace: str = "ycbcr"):
    """(header, int16 coefficients) of one image by the native host decoder, or
    the reason (str) it was refused.  ``colorspace``: as for ``parse``."""
    native = _check_progressive(progressive) == "native"
    samp = _check_sampling(sampling) == "native"
    color = _check_colorspace(colorspace) == "auto"
    data = bytes(data)
    status, _, coefs, offs = _C().jpeg_entropy_batch([data], 1, native, samp, color)
    if status[0] != 0:
        st, reason, _ = _C().jpeg_parse_colorspace(data, native, samp, color)
        return reason if st != 0 else "corrupt"
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


ENTROPY_ON = ("host", "gpu", "gpu_parallel")
_DEVICE_FORMS = ("gpu", "gpu_parallel")
_UNSYNCED = 100           # kJpegHuffUnsynced: the sub-stream kernel's rounds hit their cap (device-only status)


def _refusal(C, data: bytes, status: int, native: bool = False, samp: bool = False, color: bool = False) -> str:
    """Why an entry is a fallback: the parse's reason (in the progressive, sampling and colorspace
    modes the batch was decoded in), else what the entropy stage said."""
    st, reason, _ = C.jpeg_parse_colorspace(data, native, samp, color)
    if st != 0:
        return reason
    return "unsynced" if status == _UNSYNCED else "corrupt"


def _check_entropy_on(entropy_on: str) -> str:
    if entropy_on not in ENTROPY_ON:
        raise ValueError(f"entropy_on must be one of {ENTROPY_ON}, not {entropy_on!r}")
    return entropy_on


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
    three-component file counts as YCbCr, an RGB-coded one included).  Returns what ``decode_batch(..., entropy=)`` takes; the
    result remembers the options."""
    _check_entropy_on(entropy_on)
    native = _check_progressive(progressive) == "native"
    intervals = _check_restart(restart) == "intervals"
    samp = _check_sampling(sampling) == "native"
    color = _check_colorspace(colorspace) == "auto"
    datas = [None if d is None else bytes(d) for d in datas]
    t0 = time.perf_counter()
    if entropy_on in _DEVICE_FORMS:
        packed = _C().jpeg_huff_pack(datas, entropy_on == "gpu_parallel", native, intervals, samp, color)
        return entropy_on, datas, packed, time.perf_counter() - t0
    status, hdr, coefs, offs = _C().jpeg_entropy_batch(datas, int(threads), native, samp, color)
    return datas, status, hdr, coefs, offs, time.perf_counter() - t0, progressive, sampling, colorspace


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
    GPU ``device``, from the entropy kernels.  ``progressive="native"``:
    progressive files are decoded too, in every form.  ``restart="intervals"``:
    the device forms decode restart-interval files one interval per lane.
    ``sampling="native"``: 4:4:0 and 4:1:1 files are decoded too, in every form.
    ``colorspace="auto"``: 1x1 CMYK / YCCK files are decoded too, in every form
    (on the one-lane or the progressive kernel in the device forms)."""
    _check_entropy_on(entropy_on)
    native = _check_progressive(progressive) == "native"
    intervals = _check_restart(restart) == "intervals"
    samp = _check_sampling(sampling) == "native"
    color = _check_colorspace(colorspace) == "auto"
    C = _C()
    datas = [None if d is None else bytes(d) for d in datas]
    if entropy_on == "host":
        status, _, coefs, offs = C.jpeg_entropy_batch(datas, int(threads), native, samp, color)
        return list(status), list(offs), coefs
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"entropy_on={entropy_on!r} needs a GPU device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    packed = C.jpeg_huff_pack(datas, entropy_on == "gpu_parallel", native, intervals, samp, color)
    status = list(packed.status)
    coefs = torch.zeros(packed.coef_total, dtype=torch.int16)
    if packed.n_gpu:
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream(device)
            dev_coefs, dev_status, _ = _entropy_on_device(C, packed, device, cur, _stager(device), {})
            cur.synchronize()
            coefs = dev_coefs.cpu()
            for i, st in enumerate(dev_status.cpu().tolist()):
                if status[i] == 0:
                    status[i] = int(st)
    return status, list(packed.offs), coefs


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

    ``progressive="native"`` (default ``"fallback"``: a progressive file goes
    to ``load_image_u8`` with the reason ``"progressive"``) decodes progressive
    files of a supported layout (8-bit, 1 or 3 components, 4:4:4 / 4:2:2 /
    4:2:0, Huffman, at most ``JPEG_PROG_MAX_SCANS`` scans) natively in every
    ``entropy_on`` form: on the host threads with the scan core of
    csrc/jpeg_huff_prog.h, on the device with jpeg_entropy_prog_kernel, one
    lane per image in both device forms (no sub-stream form for progressive
    scans).  They hold the coefficients of their baseline twins, so the IDCT
    and resize kernels see no difference.  A progressive file the decoder or
    kernel refuses is then a ``"corrupt"`` fallback, one with more scans a
    ``"multiscan"`` one.  ``info["progressive"]`` names the mode in effect
    (when ``entropy`` was prepared, the one it was prepared in; on a CPU device
    the one asked for, and nothing native runs), ``info["progressive_images"]``
    counts the progressive files decoded natively.  Non-interleaved baseline
    files (``"multiscan"``), arithmetic coding, 12-bit samples and CMYK remain
    fallbacks.

    ``restart="intervals"`` (default ``"lane"``: a baseline file with a restart
    interval is walked by one lane of the one-lane kernel in both device forms)
    decodes such a file one restart interval per lane
    (jpeg_entropy_rst_kernel, csrc/jpeg_huff_rst.h) in ``"gpu"`` and
    ``"gpu_parallel"``; the packer finds the ``RSTn`` markers, and a file that
    lacks one stays with the one-lane kernel, which refuses it.  An image one of
    whose intervals is refused is a ``"corrupt"`` fallback like any other.
    Progressive files with restart markers stay on the progressive kernel.
    ``info["restart"]`` names the mode in effect (when ``entropy`` was prepared
    in a device form, the one it was prepared in; on a CPU device and in the
    host form the one asked for, and nothing changes there),
    ``info["restart_images"]`` counts the images the interval kernel decoded
    and did not flag.

    ``sampling="native"`` (default ``"fallback"``: a 4:4:0 or 4:1:1 file goes
    to ``load_image_u8`` with the reason ``"sampling"``) decodes 3-component
    files whose chroma components are 1x1 and whose luma is 1x2 (4:4:0, header
    ``mode`` 3) or 4x1 (4:1:1, ``mode`` 4) natively in every ``entropy_on``
    form, baseline, restart-interval and progressive alike: the entropy cores
    take the factors from the header, the resize kernel upsamples mode 3 with
    libjpeg's vertical triangle filter and mode 4 by replication.  Every other
    layout stays a ``"sampling"`` fallback.  ``info["sampling"]`` names the
    mode in effect (when ``entropy`` was prepared, the one it was prepared in;
    on a CPU device the one asked for, and nothing native runs),
    ``info["sampling_images"]`` counts the mode-3 and mode-4 images decoded
    natively and not flagged.

    ``colorspace="auto"`` (default ``"ycbcr"``) reads each file's colour model
    as libjpeg does.  Three components: YCbCr when the file has a JFIF APP0;
    else RGB for an Adobe APP14 with transform 0 and YCbCr for any other
    transform; else RGB for the component ids ``R``, ``G``, ``B`` and YCbCr
    otherwise.  Four components, all sampled 1x1, baseline or (with
    ``progressive="native"``) progressive, with or without restart markers:
    CMYK without an Adobe segment or with transform 0, YCCK with transform 2;
    any other transform stays a ``"components"`` fallback and any other
    four-component sampling is a ``"sampling"`` one.  RGB-coded files go
    through whichever entropy kernel their YCbCr twins take; four-component
    files take the one-lane kernel (or the progressive one) under ``"gpu"``,
    ``"gpu_parallel"`` and ``restart="intervals"`` alike.  The resize kernel
    hands RGB planes on as they are (planes 1 and 2 upsampled like chroma) and
    converts CMYK / YCCK as Pillow's ``convert("RGB")`` does, in integers.
    Under the default ``"ycbcr"`` every four-component file is a
    ``"components"`` fallback and an RGB-coded three-component file is decoded
    as YCbCr: its colours are wrong and no fallback is reported.
    ``info["colorspace"]`` names the mode in effect (when ``entropy`` was
    prepared, the one it was prepared in; on a CPU device the one asked for,
    and nothing native runs), ``info["colorspace_images"]`` counts the RGB /
    CMYK / YCCK images decoded natively and not flagged."""
    _check_entropy_on(entropy_on)
    _check_progressive(progressive)
    _check_restart(restart)
    _check_sampling(sampling)
    _check_colorspace(colorspace)
    device = torch.device(device)
    full = resize is None
    n = len(datas)
    form = entropy_on if entropy is None else (entropy[0] if isinstance(entropy[0], str) else "host")
    on_gpu = form in _DEVICE_FORMS
    if entropy is None:
        datas = [None if d is None else bytes(d) for d in datas]
    else:
        # the form and the mode the entropy stage was prepared in decide
        datas = entropy[1] if on_gpu else entropy[0]
        progressive = ("native" if entropy[2].native_progressive else "fallback") if on_gpu else entropy[6]
        if on_gpu:
            restart = "intervals" if entropy[2].restart_intervals else "lane"
            sampling = "native" if entropy[2].native_sampling else "fallback"
            colorspace = "auto" if entropy[2].native_colorspace else "ycbcr"
        else:
            sampling = entropy[7]
            colorspace = entropy[8]
    native = progressive == "native"
    samp = sampling == "native"
    color = colorspace == "auto"
    info = {"fallbacks": [], "entropy_s": 0.0, "h2d_s": 0.0, "idct_s": 0.0, "resize_s": 0.0, "kernel_s": 0.0,
            "gpu_images": 0, "entropy_on": form, "progressive": progressive, "progressive_images": 0,
            "restart": restart, "restart_images": 0, "sampling": sampling, "sampling_images": 0,
            "colorspace": colorspace, "colorspace_images": 0}
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
    packed = None
    if on_gpu:
        _, _, packed, info["pack_s"] = entropy if entropy is not None else entropy_batch(datas, threads, form,
                                                                                         progressive, restart, sampling,
                                                                                         colorspace)
        status, hdr, offs, coef_elems = list(packed.status), packed.hdr, packed.offs, packed.coef_total
    else:
        _, status, hdr, coefs, offs, info["entropy_s"] = (entropy if entropy is not None else
                                                          entropy_batch(datas, threads, "host", progressive,
                                                                        sampling=sampling, colorspace=colorspace))[:6]
        status = list(status)
        coef_elems = coefs.numel()
    geom = None
    if not full:
        hv = hdr.numpy().view(np.int32)           # JpegHeader starts with int W, H
        seen: dict = {}                           # datasets repeat a few sizes: one evaluation per size
        rows = [(0, 0, 0, 0)] * n
        for i in range(n):
            if status[i] == 0:
                wh = (int(hv[i, 0]), int(hv[i, 1]))
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
                info["fallbacks"].append((i, _refusal(C, d, status[i], native, samp, color)))
                t = torch.from_numpy(host(d).copy()).to(device)
                if full:
                    imgs.append(t)
                else:
                    out[i].copy_(t)
            elif full:
                h, w = int(hdr[i].numpy().view(np.int32)[1]), int(hdr[i].numpy().view(np.int32)[0])
                o = plan.out_off[i]
                imgs.append(out[o:o + h * w * 3].view(h, w, 3))
        if native and n:
            prog = hdr.numpy().view(np.int32)[:, C.JPEG_HEADER_PROGRESSIVE_OFFSET // 4]
            info["progressive_images"] = sum(1 for i in range(n) if status[i] == 0 and datas[i] is not None and prog[i])
        if samp and n:
            mode = hdr.numpy().view(np.int32)[:, C.JPEG_HEADER_MODE_OFFSET // 4]
            info["sampling_images"] = sum(1 for i in range(n) if status[i] == 0 and datas[i] is not None and mode[i] >= 3)
        if color and n:
            cs = hdr.numpy().view(np.int32)[:, C.JPEG_HEADER_COLORSPACE_OFFSET // 4]
            info["colorspace_images"] = sum(1 for i in range(n) if status[i] == 0 and datas[i] is not None and cs[i] != 0)
        # the result is complete when it is returned, whatever the batch held (the zero fill and
        # the fallbacks' copies too): a holder may hand it to a consumer on any other stream
        cur.synchronize()
    return (imgs if full else out), info
