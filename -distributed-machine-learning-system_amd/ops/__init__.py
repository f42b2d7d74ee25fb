"""Functional wrappers around the gfx950 HIP kernels (``idunno._C``).

Tensors are NHWC fp16 (or, for the reference-precision path, fp32) activations
on the current GPU.  Every function runs on
PyTorch's current HIP stream, so sequences of these ops can be captured into a
hipGraph with ``torch.cuda.graph``.
"""
from __future__ import annotations

from ._ext import available, load, so_path

__all__ = [
    "available", "load", "so_path", "conv2d", "linear", "preprocess", "resize_crop", "resize_crop_geometry",
    "maxpool2d", "global_avgpool", "softmax_top1", "softmax_topk", "pick_tile", "pick_tile_f32", "synth_images", "stem_fused",
    "conv2d_wino", "wino_supported", "preprocess_pack3", "conv2d_pack3",
    "conv3x3_grouped", "conv3x3_grouped_split", "conv3x3_grouped_ok",
    "conv1x1_dual", "conv1x1_dual_split", "conv1x1_fused_next", "conv2d_split", "conv2d_split_tail", "conv2d_split_tail_ok", "linear_split", "stem_split", "stem_u8_f16", "alex_stem_split", "alex_stem_u8_f16", "preprocess_pack3_split", "conv2d_pack3_split", "split_from_f32", "f32_from_split", "maxpool2d_split", "pick_tile_split",
    "jpeg_parse", "jpeg_entropy_batch", "jpeg_plan", "jpeg_idct", "jpeg_resize_crop",
    "jpeg_huff_pack", "jpeg_entropy_zero", "jpeg_entropy_gpu", "jpeg_entropy_gpu_parallel", "jpeg_huff_par_rounds",
    "JPEG_PAR_SUB_BITS", "JPEG_PAR_THREADS", "JPEG_PAR_MAX_ROUNDS",
]


def conv2d_split(x, w, bias, acc_scale: float, kh: int, kw: int, stride: int, pad: int, relu: bool,
                 residual=None, out_f32: bool = False, tile: int = -1, out=None, ksplit: int = -1, route: int = 0):
    """fp32-accurate conv on split-fp16 activations ([.., 2C] halfs, hi/lo per
    32 channels; models.packed.to_split) and weights (pack_split_weight):
    hi*hi + hi*lo + lo*hi on the f16 MFMA.  Output split (or fp32 with
    ``out_f32``).  ``tile`` forces a kernel (-1: the shape's default), ``ksplit``
    forces split-K slices (-1: auto for the default tile), ``route`` opts out of
    the specialised kernels (bit 0 band 3x3, bit 1 row-streaming 64->64, bit 2
    streaming 1x1; bit 3 restores the round-5 small-M rules for A/Bs) -- kernel
    choice depends on these arguments only."""
    return load().conv2d_split(x, w, bias, residual, kh, kw, stride, pad, relu, acc_scale, out_f32, tile, out,
                               ksplit, route)


def conv2d_split_dual(x, w, bias, acc_scale: float, acc_scale2: float, nsplit: int, kh: int, kw: int,
                      stride: int, pad: int, relu: bool, center_only: bool = True, tile: int = -1):
    """Two split convs of one input in one launch: output channels [0, nsplit)
    are conv 1 (``relu``, ``acc_scale``), the rest conv 2 (no ReLU,
    ``acc_scale2``; K over the centre tap only with ``center_only`` -- a 1x1
    stride-s conv is the centre tap of the 3x3 stride-s pad-1 conv).  Returns
    the [B, Ho, Wo, 2*Cout] split tensor; ``y[..., :2*nsplit]`` and
    ``y[..., 2*nsplit:]`` are the two convs' outputs (strided views that the
    split convs read in place)."""
    return load().conv2d_split_dual(x, w, bias, kh, kw, stride, pad, relu, acc_scale, acc_scale2, nsplit,
                                    center_only, tile)


def conv2d_split_tail(y, x2, w, bias, acc_scale: float, stride2: int, relu: bool, tile: int = -1):
    """A basic block's second 3x3/s1/p1 conv with the block's 1x1 pad-0
    downsample as a K tail: act(conv3x3(y, W2) + conv1x1/stride2(x2, Wd) + bias)
    as ONE GEMM over K = [9 taps of y | x2's channels at the strided pixel], so
    the identity stays in the fp32 accumulators (never stored, re-read or
    rounded).  ``w`` = [Cout, 9*2C + 2Cx] split weights with one ``acc_scale``
    (models.packed.pack_split_tail_weight), ``bias`` the two biases' sum.
    ``tile``: 36 (128 x 128) or 42 (128 x 160); -1 the shape's default.  Not
    ``conv2d_split_dual``, which fuses the downsample into the FIRST conv and
    still writes the identity."""
    return load().conv2d_split_tail(y, x2, w, bias, acc_scale, stride2, relu, tile)


def conv2d_split_tail_ok(b: int, ho: int, wo: int, c: int, cx: int, cout: int, mode: int = 1) -> bool:
    """Whether ``conv2d_split_tail`` is supported AND the default for this
    block shape (the rule lives in the library: conv_glds.hip
    conv_split_tail_default): false where the unfused conv would take split-K
    (small M).  ``mode`` 2: every supported shape (tests at small batches, A/B
    arm); 3: the rule, but not where the band kernel is the unfused default
    (W 28: the other arm of the layer-2 A/B); 0: never."""
    return bool(load().conv2d_split_tail_ok(b, ho, wo, c, cx, cout, mode))


def conv3x3_grouped(x, w, bias, groups: int, stride: int, relu: bool):
    """Grouped 3x3 pad-1 conv (stride 1 or 2) + bias (+ReLU) on NHWC fp16
    [B, H, W, C] (conv3x3_grouped.hip; f32 accumulation).  C % 32 == 0 and
    C / groups in {4, 8, 16, 32, 64}; ``w`` = models.packed.pack_grouped_weight
    ([C, 9 * CB] block-local fp16)."""
    return load().conv3x3_grouped(x, w, bias, int(groups), int(stride), bool(relu))


def conv3x3_grouped_split(x, w, bias, acc_scale: float, groups: int, stride: int, relu: bool):
    """The same conv, fp32-accurate, on split-fp16 activations [B, H, W, 2C] and
    weights (models.packed.pack_grouped_split_weight: [C, 2 * 9 * CB],
    ``acc_scale``): hi*hi + hi*lo + lo*hi in f32; split output, range-guarded."""
    return load().conv3x3_grouped_split(x, w, bias, float(acc_scale), int(groups), int(stride), bool(relu))


def conv3x3_grouped_ok(c: int, groups: int, stride: int) -> bool:
    """Whether the grouped 3x3 kernel takes ``c`` channels in ``groups`` groups at ``stride``."""
    return bool(load().conv3x3_grouped_ok(int(c), int(groups), int(stride)))


def preprocess_pack3_split(img_u8, kw: int, stride: int, pad: int, start=None, batch: int = -1,
                           start_offset: int = 0, window: int = -1, sub: int = 0):
    """uint8 [B,H,W,3] -> split-fp16 packed-row stem input [B, H, 2*nc, wp]."""
    return load().preprocess_pack3_split(img_u8, kw, stride, pad, start, batch, start_offset, window, sub)


def conv2d_pack3_split(x3, w, bias, acc_scale: float, width: int, kh: int, kw: int, stride: int, pad: int,
                       relu: bool, tile: int = -1):
    """fp32-accurate RGB stem conv on split packed rows (conv_glds P3+SPLIT),
    fp32 output; ``w``, ``acc_scale`` = models.packed.pack_split_weight_p3(w)."""
    return load().conv2d_pack3_split(x3, w, bias, width, kh, kw, stride, pad, relu, acc_scale, tile)


def stem_split(img_u8, w, bias, psum, acc_scale: float, start=None, batch: int = -1, start_offset: int = 0,
               window: int = -1, sub: int = 0):
    """fp32-accurate fused ResNet stem on split fp16: uint8 [B,224,224,3] ->
    split [B,56,56,128] (normalise, conv 7x7/2 + bias, ReLU, max pool 3x3/2);
    ``w, acc_scale, bias, psum`` = models.packed.pack_stem_split(w, b)."""
    return load().stem_split(img_u8, w, bias, psum, acc_scale, start, batch, start_offset, window, sub)


def alex_stem_split(img_u8, w, bias, psum, acc_scale: float, start=None, batch: int = -1, start_offset: int = 0,
                    window: int = -1, sub: int = 0, form: int = -1):
    """fp32-accurate fused AlexNet stem on split fp16: uint8 [B,224,224,3] ->
    split [B,27,27,128] (normalise, conv 11x11/4 pad 2 + bias, ReLU, max pool
    3x3/2); ``w, acc_scale, bias, psum`` = models.packed.pack_alex_stem_split(w, b).
    ``form``: the kernel form, -1 the default (phased), 0 one-half workgroups
    (one per CU), 1 phased."""
    return load().alex_stem_split(img_u8, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, form)


def alex_stem_u8_f16(img_u8, w, bias, psum, acc_scale: float, start=None, batch: int = -1, start_offset: int = 0,
                     window: int = -1, sub: int = 0, form: int = -1):
    """fp16 fused AlexNet stem in the exact-u8 form (hi MFMA only): uint8
    [B,224,224,3] -> fp16 [B,27,27,64]; operands as ``alex_stem_split``.
    ``form``: -1 the default (one-half workgroups), 0 one-half workgroups (two
    per CU), 1 phased."""
    return load().alex_stem_u8_f16(img_u8, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, form)


def stem_u8_f16(img_u8, w, bias, psum, acc_scale: float, start=None, batch: int = -1, start_offset: int = 0,
                window: int = -1, sub: int = 0):
    """fp16 fused ResNet stem in the exact-u8 form: uint8 [B,224,224,3] -> fp16
    [B,56,56,64]; the weights of models.packed.pack_stem_split (hi parts used)."""
    return load().stem_u8_f16(img_u8, w, bias, psum, acc_scale, start, batch, start_offset, window, sub)


def split_linear_splits(m: int, k: int, n: int) -> int:
    """Split-K factor for a split-fp16 FC layer: ~1024 blocks of the default
    tile, slices of >= 512 input features, at most 8."""
    tiles = -(-m // 64) * (n // 128) if n % 128 == 0 else -(-m // 128) * -(-n // 64)
    s = 1
    while s < 8 and tiles * s < 1024 and k % (64 * s) == 0 and k // (2 * s) >= 512:
        s *= 2
    return s


def linear_split(x, w, bias, acc_scale: float, relu: bool = False, out_f32: bool = False, splits: int | None = None):
    """fp32-accurate y = act(x @ w.T + bias) on split fp16: x [M, 2K] split,
    w [N, 2K] split (models.packed.pack_split_weight of [N, K, 1, 1]); output
    split [M, 2N], or fp32 [M, N] with ``out_f32``.  K slices in one launch."""
    m, k2 = x.shape
    s = split_linear_splits(m, k2 // 2, w.shape[0]) if splits is None else splits
    return load().linear_split(x, w, bias, acc_scale, relu, out_f32, s, -1)


def split_from_f32(x):
    """fp32 [.., C] -> split-fp16 [.., 2C] on the GPU."""
    return load().split_from_f32(x)


def f32_from_split(x):
    """split-fp16 [.., 2C] -> fp32 [.., C] on the GPU."""
    return load().f32_from_split(x)


def maxpool2d_split(x, k: int, s: int, pad: int, out=None):
    """NHWC max pool of fp32 or split input into the split layout."""
    return load().maxpool2d_split(x, k, s, pad, out)


def pick_tile_split(m: int, cout: int) -> int:
    return int(load().pick_tile_split(m, cout))


def conv2d(x, w, bias, kh: int, kw: int, stride: int, pad: int, relu: bool,
           residual=None, out_f32: bool = False, tile: int = -1, out=None, ksplit: int = -1, route: int = 0):
    """Implicit-GEMM MFMA convolution with fused bias / residual / ReLU
    (into ``out`` when given: a contiguous NHWC tensor, e.g. a batch slice).

    fp16 activations -> f16 MFMA kernels (f32 accumulate); fp32 activations
    -> the reference-precision kernel on the f32-input MFMA (conv_f32.hip)."""
    import torch

    if x.dtype == torch.float32:
        return load().conv2d_nhwc_f32(x, w, bias, residual, kh, kw, stride, pad, relu, tile, out)
    return load().conv2d_nhwc(x, w, bias, residual, kh, kw, stride, pad, relu, out_f32, tile, out, ksplit, route)


def conv1x1_dual(x1, x2, w, bias, stride: int, relu: bool):
    """ResNet bottleneck tail as one GEMM (fp16): act([x1 | x2 at stride] . w^T
    + bias), w = [W_expand | W_downsample] (packed 1x1 weights side by side),
    bias = b_expand + b_downsample."""
    return load().conv1x1_dual(x1, x2, w, bias, stride, relu)


def conv1x1_fused_next(x1, w, bias, w2, b2, residual=None, x2=None, stride: int = 1, relu: bool = True):
    """Bottleneck tail and the next block's reduce 1x1 in one pass (fp16):
    y = act(x1 . w^T + bias + residual) -- or with ``x2`` (block input, at
    ``stride``) the dual form act([x1 | x2] . w^T + bias) -- and
    z = relu(y . w2^T + b2).  Returns (y, z)."""
    y, z = load().conv1x1_fused_next(x1, x2, w, bias, residual, w2, b2, stride, relu)
    return y, z


def conv1x1_dual_split(x1, x2, w, bias, acc_scale: float, stride: int, relu: bool):
    """Split-fp16 (fp32-accurate) form of ``conv1x1_dual``: split activations,
    w = pack_split_weight of [W_expand | W_downsample] (one ``acc_scale``)."""
    return load().conv1x1_dual_split(x1, x2, w, bias, acc_scale, stride, relu)


def conv2d_wino(x, u, bias, relu: bool, residual=None, variant: int = 0):
    """fp32 3x3/stride-1/pad-1 conv by fused Winograd F(2x2,3x3) (conv_wino_f32.hip);
    ``u`` = models.packed.wino_weight(w) [16, Cout, Cin]."""
    return load().conv2d_wino_f32(x, u, bias, residual, relu, variant)


def preprocess_pack3(img_u8, kw: int, stride: int, pad: int, start=None, batch: int = -1, start_offset: int = 0,
                     window: int = -1, sub: int = 0, f16: bool = False):
    """uint8 [B,H,W,3] -> packed-row stem input [B, H, nc, wp], fp32 (``f16``:
    fp16) (window args as ``preprocess``)."""
    return load().preprocess_pack3(img_u8, kw, stride, pad, start, batch, start_offset, window, sub, f16)


def conv2d_pack3(x3, w, bias, width: int, kh: int, kw: int, stride: int, pad: int, relu: bool, tile: int = -1):
    """RGB stem conv on packed rows (fp32: conv_f32 mode 2; fp16: conv_glds
    pack3); ``w`` = models.packed.pack_conv_weight_p3(w, dtype)."""
    return load().conv2d_pack3(x3, w, bias, width, kh, kw, stride, pad, relu, tile)


def wino_supported(h: int, w: int, cin: int, cout: int) -> bool:
    return cin % 16 == 0 and cout % 32 == 0 and bool(load().wino_supported(h, w, cin, cout))


# fp16 FC layers: K split into slices in ONE launch (conv_glds grid = tiles x
# slices, fp32 partials + combine) when the unsplit GEMM has few blocks.  The
# round-1 version issued one launch per slice and never paid
# (profiles/r1_v8_ab_linear_split.log); in one launch AlexNet fc6 101 -> 67 us,
# fc7 54 -> 37, fc8 40 -> 20 at B=500 (profiles/r2_v22_fc_f16_sweep.md).
# None = f16_linear_splits(); an int forces that split.
LINEAR_SPLITS: int | None = None


def f16_linear_splits(m: int, k: int, n: int) -> int:
    """Split factor for an fp16 FC layer: ~512 blocks of the default tile,
    at most 4 slices, slices of >= 1024 (short K does not pay the combine)."""
    tiles = (n // 128) * -(-m // 64) if n % 128 == 0 else -(-n // 64) * -(-m // 128)
    s = 1
    while s < 4 and tiles * s < 512 and k % (64 * 2 * s) == 0 and k // (2 * s) >= 1024:
        s *= 2
    return s


def f32_linear_splits(m: int, k: int, n: int) -> int:
    """Split-K factor for an fp32 FC layer: enough K slices (one launch, fp32
    partials + combine) for ~1024 blocks of 128x64 tiles, K slices >= 256.
    Measured (tools/fc_f32_sweep.py, profiles/r2_v16_fc_f32_sweep.md): AlexNet
    fc6 430 -> 339 us, fc8 178 -> 50 us; ResNet18 fc 26 -> 14 us; ResNet50 fc
    94 -> 54 us."""
    tiles = -(-n // 128) * -(-m // 64)
    s = 1
    while s < 8 and tiles * s < 1024 and k % (16 * 2 * s) == 0 and k // (2 * s) >= 256:
        s *= 2
    return s


def linear(x, w, bias, relu: bool = False, out_f32: bool = False, splits: int | None = None):
    """y = x @ w.T + bias: the conv kernel as a 1x1 conv on a 1x1 image, or
    with ``splits`` > 1 as split-K partial GEMMs + one combine kernel
    (fp32 ``x``: the f32 conv kernel, fp32 out)."""
    import torch

    b, k = x.shape
    n = w.shape[0]
    if x.dtype == torch.float32:
        s = f32_linear_splits(b, k, n) if splits is None else splits
        if s > 1:
            return load().linear_f32_splitk(x, w, bias, relu, s, -1)
        y = load().conv2d_nhwc_f32(x.view(b, 1, 1, k), w, bias, None, 1, 1, 1, 0, relu, -1, None)
        return y.view(b, n)
    if splits is None:
        splits = LINEAR_SPLITS if LINEAR_SPLITS is not None else f16_linear_splits(b, k, n)
    if splits > 1:
        return load().linear_splitk(x, w, bias, relu, out_f32, splits, -1)
    y = load().conv2d_nhwc(x.view(b, 1, 1, k), w, bias, None, 1, 1, 1, 0, relu, out_f32, -1, None)
    return y.view(b, n)


def preprocess(img_u8, start=None, batch: int = -1, start_offset: int = 0, window: int = -1, sub: int = 0,
               f32: bool = False):
    """uint8 [B,H,W,3] -> normalised fp16 (``f32``: fp32) [B,H,W,4] (4th channel zero).
    With ``start`` (int64 GPU scalar) and ``batch``, reads images
    [*start - start_offset, ... + batch) of the shard ``img_u8`` (device-side
    window; ``start`` may be a global image index and ``start_offset`` the
    shard's first global index).  A window of ``window`` images may be done
    in parts: this call covers images [sub, sub + batch) of it."""
    return load().preprocess(img_u8, start, batch, start_offset, window, sub, f32)


def resize_crop(img_u8, resize: int = 256, crop: int = 224):
    """Resize(shorter side) + CenterCrop + normalise, fused."""
    return load().resize_crop(img_u8, resize, crop)


def resize_crop_geometry(hi: int, wi: int, resize: int = 256, crop: int = 224):
    """(Hr, Wr, top, left) that ``resize_crop`` uses for an ``hi`` x ``wi`` image:
    the resized size and the centre crop's offsets (round half to even, as
    torchvision's CenterCrop).  Host only, needs no GPU."""
    return tuple(int(v) for v in load().resize_crop_geometry(int(hi), int(wi), int(resize), int(crop)))


def stem_fused(img_u8, w, bias, start=None, batch: int = -1, start_offset: int = 0, window: int = -1,
               sub: int = 0):
    """ResNet stem in one kernel: uint8 [B,H,W,3] -> fp16 [B,H/4,W/4,64]
    (optionally a device-side window of a shard, see ``preprocess``)."""
    return load().stem_fused(img_u8, w, bias, start, batch, start_offset, window, sub)


def maxpool2d(x, k: int = 3, s: int = 2, pad: int = 1, out=None):
    return load().maxpool2d_nhwc(x, k, s, pad, out)


def global_avgpool(x):
    return load().global_avgpool_nhwc(x)


def softmax_top1(logits, packed=None, ovf=None):
    """Returns (class int32 [B], probability fp32 [B]); with ``packed`` (int32
    [>= B, 2]) also writes (class, prob bits) pairs into it.  A set split
    range-guard flag ``ovf`` marks every row class -2 (OVERFLOW_CLASS)."""
    cls, prob = load().softmax_top1(logits, packed, ovf)
    return cls, prob


def softmax_topk(logits, k: int, ovf=None):
    """Returns (class int32 [B, k], probability fp32 [B, k]) of fp32 logits
    [B, N], 1 <= k <= min(N, 16): entry j of a row is the j-th element of a
    stable descending sort (value descending, then index ascending -- not
    ``torch.topk``'s tie order), -inf entries last at probability 0.  Column 0
    is ``softmax_top1`` bit for bit.  A set split range-guard flag ``ovf``
    marks every entry class -2 (OVERFLOW_CLASS)."""
    cls, prob = load().softmax_topk(logits, int(k), ovf)
    return cls, prob


OVERFLOW_CLASS = -2      # softmax_top1 / softmax_topk's mark: a split activation left fp16's range


def set_split_guard(flag=None):
    """Split launches of this thread write their range-guard flag (int32
    device tensor) here; None turns the guard off."""
    load().set_split_guard(flag)


def pick_tile(m: int, cout: int) -> int:
    return int(load().pick_tile(m, cout))


def pick_tile_f32(m: int, cout: int, k: int, small: bool = False) -> int:
    """Default fp32 tile for an implicit GEMM of M pixels x Cout x K (= KH*KW*C)."""
    return int(load().pick_tile_f32(m, cout, k, small))


def synth_images(seed: int, start: int, n: int, device, hw: int = 224):
    """Deterministic synthetic uint8 images [n, hw, hw, 3] generated on the GPU
    (bit-identical to ``idunno.runtime.data.synth_images_cpu``)."""
    import torch

    return load().synth_images(int(seed), int(start), int(n), int(hw), torch.device(device))


# ---- JPEG decode (runtime/jpeg.py drives these) ---------------------------------------

# The ``native_progressive`` / ``restart_intervals`` / ``native_sampling`` / ``native_colorspace``
# flags below are the members of ``JpegOptions`` (csrc/runtime/jpeg_entropy.h), where each is
# documented; all default to ``False``.

def jpeg_parse(data: bytes, native_progressive: bool = False, native_sampling: bool = False,
               native_colorspace: bool = False):
    """Markers of a JPEG up to SOS: (status, reason, header dict or None);
    status 0 = a file the native decoder takes: baseline 4:4:4 / 4:2:2 / 4:2:0,
    with ``native_progressive`` a progressive file (walked up to EOI), with
    ``native_sampling`` a 4:4:0 or 4:1:1 frame (``mode`` 3 or 4), with
    ``native_colorspace`` a four-component frame sampled 1x1.  The header's
    ``colorspace`` (0 YCbCr or grey, 1 RGB, 2 CMYK, 3 YCCK) is read from the
    JFIF / Adobe markers and the component ids only with ``native_colorspace``;
    else it is 0 and every three-component file counts as YCbCr, an RGB-coded
    one included."""
    return load().jpeg_parse(data, bool(native_progressive), bool(native_sampling), bool(native_colorspace))


def jpeg_entropy_batch(datas, threads: int = 8, native_progressive: bool = False, native_sampling: bool = False,
                       native_colorspace: bool = False):
    """Huffman-decode a list of ``bytes | None`` on ``threads`` native threads
    (GIL released): (status per entry, headers, int16 coefficients on the
    host, first coefficient of each entry or -1).  The flags: as for
    ``jpeg_parse``; what it takes is decoded too."""
    return load().jpeg_entropy_batch(datas, int(threads), bool(native_progressive), bool(native_sampling),
                                     bool(native_colorspace))


# the sub-stream kernel's constants, then the progressive decoder's: the scan cap of one file
# (csrc/jpeg_huff_prog.h) and where a header row keeps its ``progressive``, ``mode`` and ``colorspace`` ints
_JPEG_PAR_CONSTANTS = ("JPEG_PAR_SUB_BITS", "JPEG_PAR_THREADS", "JPEG_PAR_MAX_ROUNDS", "JPEG_PROG_MAX_SCANS",
                       "JPEG_HEADER_PROGRESSIVE_OFFSET", "JPEG_HEADER_MODE_OFFSET", "JPEG_HEADER_COLORSPACE_OFFSET")


def __getattr__(name: str):
    # the sub-stream kernel's constants (csrc/jpeg_huff_par.h): bits per sub-stream, threads per
    # workgroup (= per image) and the cap on synchronisation rounds, read from the built library
    if name in _JPEG_PAR_CONSTANTS:
        return int(getattr(load(), name))
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def jpeg_huff_pack(datas, parallel: bool = False, native_progressive: bool = False,
                   restart_intervals: bool = False, native_sampling: bool = False, native_colorspace: bool = False):
    """Parse a list of ``bytes | None`` and pack the accepted entries for the
    device entropy stage (GIL released): a ``JpegHuffPacked`` with the parse
    ``status``, ``hdr`` and ``offs`` of ``jpeg_entropy_batch`` and the packed
    ``bytes`` (host uint8 tensor, ``byte_total``), ``coef_total``, ``n_gpu``.
    ``native_progressive``: progressive files are packed too (``n_prog``
    entries, one scan descriptor per scan) for the progressive kernel, which
    ``jpeg_entropy_gpu`` / ``jpeg_entropy_gpu_parallel`` launch next to theirs.
    ``restart_intervals``: baseline files with a restart interval whose
    ``RSTn`` markers the packer finds (``n_rst`` entries) get one work item per
    interval in ``rst_items`` (int32 ``[items, 4]``: entry, first byte, first
    MCU, interval index) for the interval kernel, which the same two calls
    launch; ``n_lane`` keeps counting the entries of the one-lane kernel.
    ``native_sampling`` and ``native_colorspace``: as for ``jpeg_parse``; 4:4:0
    and 4:1:1 files are packed like every other file of their kind, RGB-coded
    files like their YCbCr twins, and 1x1 CMYK / YCCK files always for the
    one-lane kernel or, when progressive, the progressive one.  The batch
    remembers the four flags in attributes of the same names."""
    return load().jpeg_huff_pack(datas, bool(parallel), bool(native_progressive), bool(restart_intervals),
                                 bool(native_sampling), bool(native_colorspace))


def jpeg_entropy_zero(coefs):
    """Async memset of a device int16 coefficient buffer on the current stream."""
    load().jpeg_entropy_zero(coefs)


def jpeg_entropy_gpu(packed, dev_bytes, coefs, status):
    """Huffman-decode a packed batch on the device, one lane per image: the
    packed bytes in HBM -> int16 coefficients (zeroed by the caller), int32
    status per accepted entry.  Descriptors are checked against the buffers."""
    load().jpeg_entropy_gpu(packed, dev_bytes, coefs, status)


def jpeg_entropy_gpu_parallel(packed, dev_bytes, coefs, status, scratch):
    """The same for a batch packed with ``parallel=True``: one workgroup of
    ``JPEG_PAR_THREADS`` threads per image on self-synchronising sub-streams of
    ``JPEG_PAR_SUB_BITS`` bits; the entries with restart markers go to the
    one-lane kernel in the same call.  ``scratch``: int32, at least
    ``packed.scratch_total`` elements.  A status of 100 is an image whose
    sub-streams had not synchronised after ``JPEG_PAR_MAX_ROUNDS`` rounds."""
    load().jpeg_entropy_gpu_parallel(packed, dev_bytes, coefs, status, scratch)


def jpeg_huff_par_rounds(datas):
    """Measurement helper: the synchronisation rounds the sub-stream kernel
    needs for each entry of a list of ``bytes | None``, found by running the
    same rounds on the host (-1: an entry that kernel does not take, 0: not
    converged within ``JPEG_PAR_MAX_ROUNDS``)."""
    return load().jpeg_huff_par_rounds(datas)


def jpeg_plan(hdr, status, offs, coef_elems: int, geom, crop: int, device):
    """Validate a decoded batch against its buffers and build the device
    descriptor tables; ``geom`` int64 [n, 4] = (rw, rh, left, top) or None for
    full resolution."""
    import torch

    return load().jpeg_plan(hdr, status, offs, int(coef_elems), geom, int(crop), torch.device(device))


def jpeg_idct(plan, coefs, planes):
    """Dequantise + 8x8 IDCT of a planned batch: int16 coefficients in HBM ->
    uint8 component planes (``plan.plane_bytes``)."""
    load().jpeg_idct(plan, coefs, planes)


def jpeg_resize_crop(plan, planes, out):
    """Component planes -> RGB uint8 in ``out`` (``plan.out_bytes``): chroma
    upsampling, colour conversion, BILINEAR resize, centre crop."""
    load().jpeg_resize_crop(plan, planes, out)
