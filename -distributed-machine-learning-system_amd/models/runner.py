"""``HipRunner``: a packed ``Program`` (``packed.py``) on the gfx950 kernels --
per-model routing, fusion decisions and hipGraph capture."""
from __future__ import annotations

import contextlib
import os
import threading
from dataclasses import dataclass

import torch

from .packed import (Program, expand_grouped_weight, pack_conv_weight, pack_split_tail_weight, pack_split_weight,
                     program_flops, unpack_grouped_weight, unpack_split_weight)

_CAPTURE_LOCK = threading.Lock()


@contextlib.contextmanager
def _capture_nosync(g, device, pool=None):
    """``torch.cuda.graph(g, capture_error_mode="thread_local")`` without the
    device-wide synchronize (and gc / empty_cache) that context manager does
    first: a runtime that captures a graph for a new send slot while an RCCL
    collective of an earlier round is pending on a paused or dead member would
    wait for that collective -- until the backend's timeout (120 s) when the
    member was killed (bench --rehearse-rccl worker failover, round 5).  Work
    queued on the current stream is ordered before the capture by a stream
    dependency instead."""
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        g.capture_begin(pool=pool, capture_error_mode="thread_local")
        try:
            yield
        finally:
            g.capture_end()
    torch.cuda.current_stream(device).wait_stream(s)


@dataclass(frozen=True)
class _Images:
    """The images of one forward: the batch ``img``, or with ``start`` (int64
    GPU scalar) the ``batch`` images from *start - start_offset of the
    HBM-resident shard ``img``; ``window`` / ``sub`` make that images
    [sub, sub + batch) of a window of ``window`` images."""
    img: torch.Tensor
    start: torch.Tensor | None = None
    batch: int = -1
    start_offset: int = 0
    window: int = -1
    sub: int = 0

    @property
    def n(self) -> int:
        return self.batch if self.start is not None else self.img.shape[0]

    @property
    def where(self) -> tuple:
        """The ops' trailing ``start, batch, start_offset, window, sub`` arguments."""
        return self.start, self.batch, self.start_offset, self.window, self.sub

    def part(self, sub: int, m: int) -> "_Images":
        """Images [sub, sub + m) of these: a sub-window of the shard, else a slice of the batch.
        Parts do not nest: ``sub`` counts from the window's start."""
        assert self.window == -1 and self.sub == 0, "a part of a part"
        if self.start is not None:
            return _Images(self.img, self.start, m, self.start_offset, self.n, sub)
        return _Images(self.img[sub:sub + m])


def _is_1x1(c, stride: int | None = None) -> bool:
    """A 1x1 pad-0 conv (of this stride, when given)."""
    return c.kh == c.kw == 1 and c.pad == 0 and (stride is None or c.stride == stride)


class HipRunner:
    """Runs a packed Program through the gfx950 kernels.

    ``forward(img_u8)`` takes uint8 [B,224,224,3] on the GPU and returns
    (class int32 [B], prob fp32 [B]).  ``capture(batch)`` records the whole
    forward into a hipGraph (torch.cuda.CUDAGraph == hipGraph on ROCm) with a
    static input buffer, removing per-kernel launch overhead.
    """

    # the kernel-choice switches a captured graph depends on: ``_variant()`` reads
    # them into every graph's cache key, so a switch set after a capture never
    # replays the other choice's graph
    GRAPH_SWITCHES = ("split", "split_front", "split_streams", "winograd", "wino_variant", "pack3", "pack3_f16",
                      "side_down", "stem_parts", "front_split", "fuse_stem", "batch_parts", "fuse_down",
                      "fuse_down_1x1", "fuse_next_1x1", "stem_u8", "route", "fuse_down_tail", "astem_form",
                      "grouped_dense")

    def __init__(self, program: Program, device=None, fuse_stem: bool = True, front_split: int | None = None,
                 winograd: bool = True, wino_variant: int | None = None, pack3: bool = True):
        from .. import ops

        ops.load()
        self.ops = ops
        self.fuse_stem = fuse_stem
        # fp32 3x3/s1 convs through the fused Winograd F(2x2,3x3) kernel (2.25x
        # fewer f32-MFMA products than the direct conv; conv_wino_f32.hip)
        self.winograd = winograd
        self.pack3 = pack3           # fp32 RGB stems on packed rows (conv_f32.hip mode 2)
        self.pack3_f16 = False       # fp16 AlexNet conv1 on packed rows (measured net-neutral, see _logits)
        self.side_down = False       # downsample conv on a second stream (A/B: tools/ab_flag.py --attr)
        # fused AlexNet stem kernel form (ops.alex_stem_split / alex_stem_u8_f16): -1 the default, 0 one-half
        # workgroups, 1 phased (A/B: tools/ab_flag.py --attr astem_form --values 0,1 --model alexnet)
        self.astem_form = -1
        self.stem_parts: int | None = None   # fp32 ResNet: stem + maxpool on batch parts (None = 1)
        # fp32 ResNets: residual stages on split-fp16 convs (conv_glds SPLIT:
        # hi*hi + hi*lo + lo*hi on the f16 MFMA, fp32-accurate) instead of the
        # f32-MFMA Winograd / direct kernels; False = the all-f32-MFMA path
        self.split = True
        # split path: fused stem + layer1 on this many batch parts (None = 1;
        # A/B: tools/ab_flag.py --attr split_front --values 1,2)
        self.split_front: int | None = None
        # split path: the batch as this many streams' halves (None = 1; A/B:
        # tools/ab_flag.py --attr split_streams --values 1,2)
        self.split_streams: int | None = None
        self._side: dict = {}
        # None = measured default (tools/wino_ablate.py, profiles/r2_v6_wino_variants.md):
        # variant 3 -- 4-wave blocks of 64 tiles, one 58-KiB LDS stage, two blocks
        # per CU -- is the fastest on every ResNet layer shape (same-box A/B:
        # 0.86-0.88x the 8-wave variant's time at 56/28/14, 0.67x at 7x7)
        self.wino_variant = wino_variant
        # >1: stem + the full-resolution blocks (ResNet layer1) run on this many
        # batch parts, each part's activations small enough to stay in the
        # 256 MiB Infinity Cache between the stem and the end of layer1.
        # None = measured default (tools/bench_split.py, profiles/r1_v8_front_split.log):
        # 2 parts for ResNet18/34 at >= 256 images (+1.3 %), else 1 (ResNet50: -0.6 %)
        self.front_split = front_split
        # >1: the WHOLE ResNet forward on this many batch parts, each part's
        # activations small enough to stay in the 256 MiB Infinity Cache from
        # producer to consumer (the memory-bound ResNet50 bottlenecks read every
        # 4x-wide tensor twice: next block's 1x1 reduce and its residual add).
        # None = 1
        self.batch_parts: int | None = None
        # split path: a stride-2 block's 1x1/2 downsample in the same launch as
        # its FIRST conv, the 3x3/2 (the downsample is that conv's centre tap; one
        # input read, one launch).  The identity is still written to memory and
        # read back as the second conv's residual.  Measured slower (-2.1 / -3.1 %
        # whole forward, profiles/r3_dual_downsample.md), so off by default
        self.fuse_down = False
        self._dual: dict = {}
        # split path: the downsample as a K tail of the block's SECOND 3x3 conv
        # (ops.conv2d_split_tail: one GEMM over [9 taps of y | x at the strided
        # pixel]) -- no downsample launch, the identity never exists in memory.
        # A different fusion from fuse_down above.  0 / False: off (the separate
        # downsample + residual epilogue, the launch sequence before this fusion);
        # 1 / True: where the library's rule says so (ops.conv2d_split_tail_ok: not
        # at split-K batches); 2: every supported block (also over split-K: tests,
        # A/B arm); 3: the rule, but ResNet layer2 stays on the band kernel + streaming
        # downsample (A/B arm).  ResNet18 b400 +3.2 %, b50 +1.8 % (docs/KERNELS.md)
        self.fuse_down_tail = 1
        self._tail: dict = {}
        # fp16 bottleneck blocks with a 1x1 downsample: the expansion 1x1 and the
        # downsample as ONE GEMM over [y | x] (ops.conv1x1_dual), so the
        # downsample's output (the residual) never reaches HBM
        self.fuse_down_1x1 = True
        self._dual1: dict = {}
        # fp16 ResNet50 layer1: a block's tail kernel also computes the next
        # block's reduce 1x1 from its output tile on chip (ops.conv1x1_fused_next)
        self.fuse_next_1x1 = True
        # fp16 ResNet stem in the exact-u8 form (stem_split_kernel<.., F16>: uint8 input exact, hi MFMA only);
        # off: the normalised-fp16 stem_fused_kernel is faster (ResNet18 -3.7 %, ResNet50 -1.8 %,
        # profiles/r3_ab_stem_u8_f16.md)
        self.stem_u8 = False
        # per-runner kernel routing for whole-graph A/Bs (ops.conv2d_split ``route``: bit 0 no
        # band-staged 3x3, bit 1 no row-streaming 64->64, bit 2 no streaming 1x1); 0 = defaults.
        # The kernel library itself has no process-global switches (VERDICT r4 weakness 4).
        self.route = 0
        # grouped 3x3 convs (ResNeXt) as the dense conv on the block-diagonal expansion of their
        # weights (ops.conv2d / conv2d_split direct kernels, no Winograd) instead of the grouped
        # kernel: the A/B baseline and an independent cross-check (tools/ab_flag.py --attr grouped_dense)
        self.grouped_dense = False
        self._gdense: dict = {}
        self.device = torch.device(device or "cuda")
        self.p = program.to(self.device)
        self._graphs: dict[int, tuple] = {}
        # memory pool shared by this runner's captures (None: one private pool per
        # graph).  Sharing is safe only where every replay is stream-ordered on ONE
        # stream and a graph's outputs are consumed before another graph of the
        # pool replays (its intermediates may reuse their memory): HipExecutor
        # sets it (one private stream, outputs copied out or written to the
        # caller's buffer in the same stream order)
        self.graph_pool = None
        # split range guard: the split kernels set this flag
        # when an activation leaves fp16's range (|v| >= 65504 has no finite hi
        # half); softmax_top1 then marks the batch (class -2) and the eager
        # paths rerun it on the all-f32 kernels, which have fp32's range
        self._ovf = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.overflow_fallback = True
        self.overflow_reruns = 0
        self._capturing = False
        # replay captured graphs with a bare hipGraphLaunch (ops.graph_launch) instead of
        # torch.cuda.CUDAGraph.replay (tools/system_launch_probe.py measures both)
        self.direct_launch = os.environ.get("IDUNNO_DIRECT_LAUNCH", "0") == "1"

    # -- eager forward ------------------------------------------------------
    def _guarded(self) -> bool:
        return self.p.dtype == "fp32" and self.split and self._split_ok()

    def logits(self, img_u8: torch.Tensor, start: torch.Tensor | None = None, batch: int = -1,
               start_offset: int = 0) -> torch.Tensor:
        """fp32 logits.  With ``start`` (int64 GPU scalar) and ``batch``,
        ``img_u8`` is a whole HBM-resident shard and the images
        [*start - start_offset, ... + batch) are classified (device-side window).

        On the split path the range guard is armed; outside a graph capture a
        forward that tripped it is recomputed on the all-f32 kernels (one host
        read of the flag per eager call)."""
        ims = _Images(img_u8, start, batch, start_offset)
        if not self._guarded():
            return self._logits(ims)
        self._ovf.zero_()
        self.ops.set_split_guard(self._ovf)
        try:
            out = self._logits(ims)
        finally:
            self.ops.set_split_guard(None)
        if self.overflow_fallback and not self._capturing and int(self._ovf.item()):
            out = self.logits_f32_exact(img_u8, start, batch, start_offset)
            # these logits have fp32's range: a following softmax_top1 must not
            # mark the batch OVERFLOW_CLASS (forward() passes the flag on)
            self._ovf.zero_()
        return out

    def logits_f32_exact(self, img_u8, start=None, batch: int = -1, start_offset: int = 0):
        """The same forward on the all-f32-MFMA kernels (fp32 range)."""
        self.overflow_reruns += 1
        was = self.split
        self.split = False
        try:
            return self._logits(_Images(img_u8, start, batch, start_offset))
        finally:
            self.split = was

    def _logits(self, ims: _Images) -> torch.Tensor:
        o, p, img_u8 = self.ops, self.p, ims.img
        native = tuple(img_u8.shape[1:3]) == (224, 224)
        if ims.start is not None and not native:
            raise ValueError("device-side windows need 224x224 shards")
        parts = self.batch_parts or 1
        if p.kind == "resnet" and native and parts > 1 and ims.n >= 2 * parts:
            return self._logits_in_parts(ims, parts)
        if p.dtype == "fp32":
            return self._logits_f32(ims, native)
        s = p.stem
        fused = (self.fuse_stem and native and p.kind == "resnet" and s.small and s.kh == 7 and s.kw == 7
                 and s.stride == 2 and s.pad == 3 and s.cout == 64)
        first = p.features[0][1] if p.kind != "resnet" else None
        feats = p.features
        # AlexNet: uint8 -> conv1 + ReLU + max pool in one phased MFMA kernel (alex_stem.hip)
        if first is not None and native and self._alex_stem_fusable(first, feats[1:]):
            x = o.alex_stem_u8_f16(img_u8, first.fs, first.fs_bias, first.fs_psum, first.fs_scale, *ims.where,
                                   form=self.astem_form)
            feats = feats[2:]
        elif first is not None and native and self.pack3_f16 and first.p3 is not None:
            # AlexNet conv1 (11x11/4) on packed fp16 rows through conv_glds (K 448
            # vs 704 for NHWC4 on the register-staged conv_igemm): conv 290 -> 220
            # us at B=500, but the packed-row preprocess costs 133 vs 46 us, so it
            # is off by default (profiles/r2_v21_alexnet_f16_pack3.md)
            x3 = o.preprocess_pack3(img_u8, first.kw, first.stride, first.pad, *ims.where, f16=True)
            x = o.conv2d_pack3(x3, first.p3, first.b, img_u8.shape[2], first.kh, first.kw, first.stride, first.pad,
                               first.relu)
            feats = feats[1:]
        elif not fused:
            x = o.preprocess(img_u8, *ims.where) if native else o.resize_crop(img_u8, 256, 224)
        if p.kind == "resnet":
            split = self.front_split if self.front_split is not None else \
                (2 if p.name in ("resnet18", "resnet34") and ims.n >= 256 else 1)
            nfront = self._front_blocks() if fused and split > 1 else 0
            if nfront:
                x = self._front_parts(ims, nfront, split, self._stem16, self._block, 1)
            elif fused:
                x = self._stem16(ims)
            else:
                x = o.conv2d(x, s.w, s.b, s.kh, s.kw, s.stride, s.pad, s.relu)
                x = o.maxpool2d(x, 3, 2, 1)
            x = self._blocks(p.blocks[nfront:], x)
            x = o.global_avgpool(x)
        else:
            for k, v in feats:
                if k == "conv":
                    x = o.conv2d(x, v.w, v.b, v.kh, v.kw, v.stride, v.pad, v.relu)
                else:
                    x = o.maxpool2d(x, *v)
            x = x.reshape(x.shape[0], -1)
        for i, fc in enumerate(p.fcs):
            last = i == len(p.fcs) - 1
            x = o.linear(x, fc.w, fc.b, relu=fc.relu, out_f32=last)
        return x

    def _alex_stem_fusable(self, first, feats) -> bool:
        """conv1 has the fused-stem operands and ``feats`` (what follows it)
        starts with the 3/2/0 max pool the fused AlexNet stem kernels include."""
        return bool(self.fuse_stem and first.fs is not None and first.kh == 11 and first.relu and feats
                    and feats[0][0] == "pool" and tuple(feats[0][1]) == (3, 2, 0))

    def _head(self, x):
        """fp32 ResNet head on the pooled features: the FC layers.  The caller pools
        (``x = global_avgpool(x)``, rebinding its name), so the last block's output
        goes back to the allocator before the FC allocates, as it always did: a
        captured graph bakes those addresses in."""
        for fc in self.p.fcs:
            x = self.ops.linear(x, fc.w, fc.b, relu=fc.relu)
        return x

    def _logits_f32(self, ims: _Images, native):
        """Reference-precision forward: every activation, weight and product in
        fp32 (conv_f32.hip on the f32-input MFMA, elementwise_f32.hip)."""
        o, p = self.ops, self.p
        if not native:
            raise ValueError("the fp32 path takes 224x224 inputs (resize on host first)")
        first = p.stem if p.kind == "resnet" else p.features[0][1]
        nb = ims.n
        if p.kind == "resnet" and self.split and self._split_ok():
            # fused split stem (uint8 -> normalise -> conv7x7/2 -> ReLU -> max
            # pool, split out; or stem conv + max pool into the split layout)
            # -> split residual stages (the last conv writes fp32) -> fp32 avgpool / FC
            fused = self.fuse_stem and first.fs is not None and first.relu
            if fused and (self.split_streams or 1) > 1 and nb >= 64 and ims.img.is_cuda:
                return self._split_dual_stream(ims)
            parts = self.split_front or 1
            nfront = self._front_blocks() if fused and parts > 1 and nb >= 2 * parts else 0
            if nfront:
                x = self._front_parts(ims, nfront, parts, self._stem_split, self._block_split, 2)
            elif fused:
                x = self._stem_split(ims)
            else:
                x = o.maxpool2d_split(self._stem_f32(first, ims), 3, 2, 1)
            for i, blk in enumerate(p.blocks[nfront:], nfront):
                x = self._block_split(blk, x, last=i == len(p.blocks) - 1)
            x = o.global_avgpool(x)
            return self._head(x)
        parts = self.stem_parts if self.stem_parts is not None else 1
        if p.kind == "resnet" and parts > 1 and nb >= 2 * parts:
            # stem + maxpool on batch parts: a part's 112x112x64 stem output
            # (nb/parts x 3.2 MB) stays in the 256-MB Infinity Cache between the
            # conv's stores and the pool's reads instead of round-tripping HBM
            n = -(-nb // parts)
            x = None
            for sub in range(0, nb, n):
                m = min(n, nb - sub)
                y = self._stem_f32(first, ims.part(sub, m))
                if x is None:
                    x = torch.empty((nb, (y.shape[1] + 1) // 2, (y.shape[2] + 1) // 2, y.shape[3]),
                                    dtype=y.dtype, device=y.device)
                o.maxpool2d(y, 3, 2, 1, out=x[sub:sub + m])
            for blk in p.blocks:
                x = self._block(blk, x)
            x = o.global_avgpool(x)
            return self._head(x)
        if p.kind == "alexnet" and self.split and self._split_ok():
            return self._alexnet_split(first, ims)
        x = self._stem_f32(first, ims)
        if p.kind == "resnet":
            x = o.maxpool2d(x, 3, 2, 1)
            for blk in p.blocks:
                x = self._block(blk, x)
            x = o.global_avgpool(x)
            return self._head(x)
        for k, v in p.features[1:]:
            x = self._conv(v, x) if k == "conv" else o.maxpool2d(x, *v)
        x = x.reshape(x.shape[0], -1)
        for fc in p.fcs:
            x = o.linear(x, fc.w, fc.b, relu=fc.relu)
        return x

    def _logits_in_parts(self, ims: _Images, parts: int):
        """The whole forward on ``parts`` consecutive batch parts (same
        numbers as one pass: every op is per image)."""
        nb = ims.n
        n = -(-nb // parts)
        outs = []
        keep = self.batch_parts
        self.batch_parts = 1
        try:
            for sub in range(0, nb, n):
                m = min(n, nb - sub)
                if ims.start is None:
                    outs.append(self._logits(ims.part(sub, m)))
                else:       # a window of its own from a shifted start scalar, not a sub-window
                    outs.append(self._logits(_Images(ims.img, ims.start + sub, m, ims.start_offset)))
        finally:
            self.batch_parts = keep
        return torch.cat(outs, 0)

    def _stem_f32(self, first, ims: _Images):
        """fp32 RGB stem conv (+ReLU) of a window / part of the images."""
        o, img_u8 = self.ops, ims.img
        if self.split and first.sp3 is not None:
            # split-fp16 packed rows (fp32-accurate) on the f16 MFMA, fp32 output
            x3 = o.preprocess_pack3_split(img_u8, first.kw, first.stride, first.pad, *ims.where)
            return o.conv2d_pack3_split(x3, first.sp3, first.b, first.s_scale, img_u8.shape[2], first.kh, first.kw,
                                        first.stride, first.pad, first.relu)
        if self.pack3 and first.p3 is not None:
            # packed rows: K 176 vs 224 for the 7x7/2, 400 vs 528 for the 11x11/4
            x3 = o.preprocess_pack3(img_u8, first.kw, first.stride, first.pad, *ims.where)
            return o.conv2d_pack3(x3, first.p3, first.b, img_u8.shape[2], first.kh, first.kw, first.stride,
                                  first.pad, first.relu)
        x = o.preprocess(img_u8, *ims.where, f32=True)
        return o.conv2d(x, first.w, first.b, first.kh, first.kw, first.stride, first.pad, first.relu)

    def _grouped_dense(self, c, kind: str):
        """The dense block-diagonal expansion of a grouped conv (``groups`` x its
        weights: up to 75 MB fp16 / 151 MB fp32 for one resnext101_32x8d layer,
        read from HBM by every launch), packed for the direct kernels of ``kind``:
        "f16" -> pack_conv_weight, "split" -> (pack_split_weight, acc_scale), "f32" ->
        pack_conv_weight fp32.  Built on first use, cached on the runner."""
        key = (id(c), kind)
        if key not in self._gdense:
            w = unpack_grouped_weight(c).cpu() if c.w.dim() != 4 else c.w.cpu()
            dense = expand_grouped_weight(w.double() if kind == "split" else w.float(), c.groups)
            if kind == "split":
                sw, scale = pack_split_weight(dense)
                self._gdense[key] = (sw.to(self.device), scale)
            else:
                self._gdense[key] = pack_conv_weight(dense, "fp16" if kind == "f16" else "fp32")[0].to(self.device)
        return self._gdense[key]

    def _conv_grouped(self, c, x):
        """A grouped 3x3 conv on fp16 or fp32 activations.  fp16: the grouped
        kernel, or with ``grouped_dense`` the dense conv on the expansion.  fp32
        (the all-f32-MFMA path and the range-guard rerun, which have no grouped
        kernel): always the dense fp32 expansion on the direct f32 kernel -- groups x
        the weight bytes and MFMA work (see ``_grouped_dense``)."""
        if x.dtype == torch.float32:
            return self.ops.conv2d(x, self._grouped_dense(c, "f32"), c.b, 3, 3, c.stride, 1, c.relu)
        if self.grouped_dense:
            return self.ops.conv2d(x, self._grouped_dense(c, "f16"), c.b, 3, 3, c.stride, 1, c.relu,
                                   route=self.route | self._f16_route(x.shape[0]))
        return self.ops.conv3x3_grouped(x, c.w, c.b, c.groups, c.stride, c.relu)

    def _conv(self, c, x, residual=None, out=None):
        if c.groups > 1:
            assert residual is None and out is None, "a grouped conv is a bottleneck's middle conv"
            return self._conv_grouped(c, x)
        if c.wino is not None and self.winograd and out is None and x.dtype == torch.float32 \
                and self.ops.wino_supported(x.shape[1], x.shape[2], c.cin, c.cout):
            var = self.wino_variant if self.wino_variant is not None else 3
            return self.ops.conv2d_wino(x, c.wino, c.b, c.relu, residual, var)
        return self.ops.conv2d(x, c.w, c.b, c.kh, c.kw, c.stride, c.pad, c.relu, residual=residual, out=out,
                               route=self.route | self._f16_route(x.shape[0]))

    def _f16_route(self, nb: int) -> int:
        """Measured per-model default on top of ``route``: ResNet50 fp16 at
        B >= 768 skips the band-staged 3x3 at W 28 (+1.2 % at B = 1024, -0.4 % at
        B = 400; ResNet18 fp16 keeps it: -0.7 % / -2.2 % without it at B = 400 /
        1024; profiles/r6q_ab_r50_route_0_1.log, profiles/r6r_*)."""
        return 1 if self.p.name == "resnet50" and nb >= 768 else 0

    def _blocks(self, blocks, x):
        """fp16 residual stages; with ``fuse_next_1x1`` a bottleneck block whose
        successor starts with a 1x1 reduce hands that conv's output over from
        its own tail kernel (ops.conv1x1_fused_next), and the successor skips it."""
        pre = None
        for i, blk in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            x, pre = self._block_next(blk, x, pre, nxt)
        return x

    def _next_ok(self, blk, x, nxt) -> tuple | None:
        """(K2, stride) of a fusable tail + next reduce, else None."""
        if not (self.fuse_next_1x1 and nxt is not None and x.dtype == torch.float16 and x.is_cuda):
            return None
        last, d, r = blk.convs[-1], blk.down, nxt.convs[0]
        if not (_is_1x1(last, 1) and _is_1x1(r, 1) and r.relu and last.relu and r.cin == last.cout):
            return None
        k2, stride = 0, 1
        if d is not None:
            if not (self.fuse_down_1x1 and _is_1x1(d)):
                return None
            k2, stride = d.cin, d.stride
        ho = (x.shape[1] - 1) // stride + 1
        ok = self.ops.load().conv1x1_fused_next_ok(last.cin, k2, last.cout, r.cout, x.shape[0] * ho * ho)
        return (k2, stride) if ok else None

    def _block_next(self, blk, x, pre, nxt):
        """(block output, the next block's first-conv output or None); ``pre`` =
        this block's first-conv output, already computed by the previous tail."""
        fused = self._next_ok(blk, x, nxt)
        if pre is None and fused is None:
            return self._block(blk, x), None
        y = pre if pre is not None else self._conv(blk.convs[0], x)
        for c in blk.convs[1:-1]:
            y = self._conv(c, y)
        if fused is None:
            last = blk.convs[-1]
            if self._dual1_ok(blk, x, None):
                w, b = self._dual1_weights(blk)
                return self.ops.conv1x1_dual(y, x, w, b, blk.down.stride, last.relu), None
            idt = x if blk.down is None else self._conv(blk.down, x)
            return self._conv(last, y, residual=idt), None
        r = nxt.convs[0]
        if blk.down is not None:
            w, b = self._dual1_weights(blk)
            out, z = self.ops.conv1x1_fused_next(y, w, b, r.w, r.b, x2=x, stride=fused[1])
        else:
            out, z = self.ops.conv1x1_fused_next(y, blk.convs[-1].w, blk.convs[-1].b, r.w, r.b, residual=x)
        return out, z

    def _dual1_ok(self, blk, x, out) -> bool:
        d, last = blk.down, blk.convs[-1]
        if not (self.fuse_down_1x1 and out is None and d is not None and x.dtype == torch.float16 and x.is_cuda):
            return False
        if not (_is_1x1(last, 1) and _is_1x1(d) and not last.small and not d.small):
            return False
        ho = (x.shape[1] - 1) // d.stride + 1
        return bool(self.ops.load().conv1x1_dual_ok(last.cin, d.cin, last.cout, x.shape[0] * ho * ho))

    def _dual1_weights(self, blk):
        key = id(blk)
        if key not in self._dual1:
            last, d = blk.convs[-1], blk.down
            self._dual1[key] = (torch.cat([last.w, d.w], 1).contiguous(), (last.b + d.b).contiguous())
        return self._dual1[key]

    def _block(self, blk, x, out=None):
        """One residual block; the last conv fuses +identity and ReLU (into ``out``).
        With ``side_down`` the 1x1 downsample conv runs on a second stream,
        concurrently with the block's first conv (a fork/join that hipGraph
        capture keeps as two parallel branches)."""
        if self._dual1_ok(blk, x, out):
            y = x
            for c in blk.convs[:-1]:
                y = self._conv(c, y)
            w, b = self._dual1_weights(blk)
            return self.ops.conv1x1_dual(y, x, w, b, blk.down.stride, blk.convs[-1].relu)
        idt = x
        join = None
        if blk.down is not None:
            if self.side_down and x.is_cuda:
                cur = torch.cuda.current_stream(x.device)
                side = self._side_stream(x.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    idt = self._conv(blk.down, x)
                x.record_stream(side)          # x / idt cross streams: keep the allocator honest
                idt.record_stream(cur)
                join = side
            else:
                idt = self._conv(blk.down, x)
        y = x
        for c in blk.convs[:-1]:
            y = self._conv(c, y)
        if join is not None:
            torch.cuda.current_stream(x.device).wait_stream(join)
        return self._conv(blk.convs[-1], y, residual=idt, out=out)

    def _split_ok(self) -> bool:
        p = self.p
        if p.kind == "alexnet":
            return all(v.sw is not None for k, v in p.features[1:] if k == "conv") and \
                all(f.sw is not None for f in p.fcs)
        return all(c.sw is not None for b in p.blocks for c in [*b.convs, *([b.down] if b.down else [])])

    def _alexnet_split(self, first, ims: _Images):
        """fp32-accurate AlexNet: the fused split stem (uint8 -> conv1 + ReLU + max
        pool in one kernel, alex_stem.hip; without it: split packed-row conv1 with
        fp32 out, then the pool into the split layout) -> split convs 2-5 -> split
        FCs (split-K), fp32 logits."""
        o, p = self.ops, self.p
        feats = p.features[1:]
        if self._alex_stem_fusable(first, feats):
            x = o.alex_stem_split(ims.img, first.fs, first.fs_bias, first.fs_psum, first.fs_scale, *ims.where,
                                  form=self.astem_form)
            feats = feats[1:]
        else:
            x = self._stem_f32(first, ims)
        for k, v in feats:
            x = self._conv_split(v, x) if k == "conv" else o.maxpool2d_split(x, *v)
        x = x.reshape(x.shape[0], -1)         # split [B, 6*6*2*256]: the split layout of the NHWC flatten
        for i, fc in enumerate(p.fcs):
            x = o.linear_split(x, fc.sw, fc.b, fc.s_scale, relu=fc.relu, out_f32=i == len(p.fcs) - 1)
        return x

    def _conv_split(self, c, x, residual=None, out_f32=False, out=None):
        if c.groups > 1:
            assert residual is None and out is None and not out_f32, "a grouped conv is a bottleneck's middle conv"
            if self.grouped_dense:
                sw, scale = self._grouped_dense(c, "split")
                return self.ops.conv2d_split(x, sw, c.b, scale, 3, 3, c.stride, 1, c.relu, route=self.route)
            return self.ops.conv3x3_grouped_split(x, c.sw, c.b, c.s_scale, c.groups, c.stride, c.relu)
        return self.ops.conv2d_split(x, c.sw, c.b, c.s_scale, c.kh, c.kw, c.stride, c.pad, c.relu, residual,
                                     out_f32, out=out, route=self.route)

    def _dual_ok(self, blk) -> bool:
        d, c0 = blk.down, blk.convs[0] if blk.convs else None
        return (self.fuse_down and d is not None and len(blk.convs) == 2 and c0.kh == 3 and c0.kw == 3
                and c0.pad == 1 and _is_1x1(d, c0.stride)
                and d.cin == c0.cin and d.cout == c0.cout and c0.relu and not d.relu
                and c0.sw is not None and d.sw is not None and c0.cout % 32 == 0)

    def _dual_weights(self, blk):
        """[2 Cout, 9*2C] split weights: the 3x3 conv's rows, then the 1x1
        downsample's rows in the centre-tap K block (zeros elsewhere)."""
        key = id(blk)
        got = self._dual.get(key)
        if got is None:
            c0, d = blk.convs[0], blk.down
            c2 = c0.sw.shape[1] // 9
            w = torch.zeros((2 * c0.cout, c0.sw.shape[1]), dtype=c0.sw.dtype, device=c0.sw.device)
            w[:c0.cout] = c0.sw
            w[c0.cout:, 4 * c2:5 * c2] = d.sw
            got = self._dual[key] = (w, torch.cat([c0.b, d.b]).contiguous())
        return got

    def _block_split(self, blk, x, last: bool = False, out=None):
        """Residual block on split-fp16 activations; with ``last`` the block's
        output is fp32 (for the avgpool / FC head); into ``out`` when given."""
        if self._dual_ok(blk):
            c0, d = blk.convs[0], blk.down
            w, b = self._dual_weights(blk)
            both = self.ops.conv2d_split_dual(x, w, b, c0.s_scale, d.s_scale, c0.cout, 3, 3, c0.stride, 1, True)
            y, idt = both[..., :2 * c0.cout], both[..., 2 * c0.cout:]
            return self._conv_split(blk.convs[1], y, residual=idt, out_f32=last, out=out)
        if not last and out is None and self._tail_ok(blk, x):
            c0, c1, d = blk.convs[0], blk.convs[1], blk.down
            y = self._conv_split(c0, x)
            w, b, scale = self._tail_weights(blk)
            return self.ops.conv2d_split_tail(y, x, w, b, scale, d.stride, c1.relu)
        if not last and out is None and self._dual1_split_ok(blk, x):
            y = x
            for c in blk.convs[:-1]:
                y = self._conv_split(c, y)
            w, b, scale = self._dual1_split_weights(blk)
            return self.ops.conv1x1_dual_split(y, x, w, b, scale, blk.down.stride, blk.convs[-1].relu)
        idt = x if blk.down is None else self._conv_split(blk.down, x)
        y = x
        for c in blk.convs[:-1]:
            y = self._conv_split(c, y)
        return self._conv_split(blk.convs[-1], y, residual=idt, out_f32=last, out=out)

    def _tail_ok(self, blk, x) -> bool:
        """A basic block (two 3x3 convs) with a 1x1 pad-0 downsample whose shape
        the library fuses by default (fuse_down_tail)."""
        d = blk.down
        if not (int(self.fuse_down_tail) and d is not None and len(blk.convs) == 2 and x.is_cuda):
            return False
        c0, c1 = blk.convs
        if not (c1.kh == c1.kw == 3 and c1.stride == 1 and c1.pad == 1 and _is_1x1(d)
                and not d.relu and d.cout == c1.cout and c1.cin == c0.cout and d.cin == c0.cin
                and c1.sw is not None and d.sw is not None and c0.sw is not None):
            return False
        ho = (x.shape[1] + 2 * c0.pad - c0.kh) // c0.stride + 1
        wo = (x.shape[2] + 2 * c0.pad - c0.kw) // c0.stride + 1
        if ho != (x.shape[1] - 1) // d.stride + 1 or wo != (x.shape[2] - 1) // d.stride + 1:
            return False
        return self.ops.conv2d_split_tail_ok(x.shape[0], ho, wo, c1.cin, d.cin, c1.cout, int(self.fuse_down_tail))

    def _tail_weights(self, blk):
        """[W2 | Wd] as ONE split weight (one exponent from the max |w| over
        both), bias = the two biases' sum; built once per block."""
        key = id(blk)
        if key not in self._tail:
            c1, d = blk.convs[1], blk.down
            sw, scale = pack_split_tail_weight(unpack_split_weight(c1).cpu(), unpack_split_weight(d).cpu())
            self._tail[key] = (sw.to(self.device), (c1.b + d.b).contiguous(), scale)
        return self._tail[key]

    def _dual1_split_ok(self, blk, x) -> bool:
        d, last = blk.down, blk.convs[-1]
        if not (self.fuse_down_1x1 and d is not None and x.is_cuda and last.sw is not None and d.sw is not None):
            return False
        if not (_is_1x1(last, 1) and _is_1x1(d)):
            return False
        ho = (x.shape[1] - 1) // d.stride + 1
        return bool(self.ops.load().conv1x1_dual_split_ok(last.cin, d.cin, last.cout, x.shape[0] * ho * ho))

    def _dual1_split_weights(self, blk):
        """[W3 | Wds] re-packed as ONE split weight (one accumulator scale)."""
        key = ("split", id(blk))
        if key not in self._dual1:
            last, d = blk.convs[-1], blk.down
            w = torch.cat([unpack_split_weight(last).cpu(), unpack_split_weight(d).cpu()], 1)
            sw, scale = pack_split_weight(w)
            self._dual1[key] = (sw.to(self.device), (last.b + d.b).contiguous(), scale)
        return self._dual1[key]

    def _stem_split(self, ims: _Images):
        """Fused split ResNet stem (uint8 -> conv 7x7/2 + ReLU + max pool, split out)."""
        s = self.p.stem
        return self.ops.stem_split(ims.img, s.fs, s.fs_bias, s.fs_psum, s.fs_scale, *ims.where)

    def _split_part(self, ims: _Images):
        """Whole split ResNet forward of these images."""
        x = self._stem_split(ims)
        for i, blk in enumerate(self.p.blocks):
            x = self._block_split(blk, x, last=i == len(self.p.blocks) - 1)
        x = self.ops.global_avgpool(x)
        return self._head(x)

    def _split_dual_stream(self, ims: _Images):
        """The batch as two halves on two streams (fork/join, kept as parallel
        branches by hipGraph capture): one half's blocks fill the other's
        partial last wave of workgroups (layers 3-4 run 1.6-2.4 waves of blocks)."""
        img_u8, nb = ims.img, ims.n
        cur = torch.cuda.current_stream(img_u8.device)
        side = self._side_stream(img_u8.device)
        side.wait_stream(cur)
        n0 = nb // 2
        l0 = self._split_part(ims.part(0, n0))
        with torch.cuda.stream(side):
            l1 = self._split_part(ims.part(n0, nb - n0))
        img_u8.record_stream(side)
        l1.record_stream(cur)
        cur.wait_stream(side)
        return torch.cat([l0, l1])

    def _front_parts(self, ims: _Images, nfront, parts, stem, block, width):
        """``stem`` + the first ``nfront`` (full-resolution) blocks through
        ``block`` on ``parts`` batch parts, so a part's activations can stay in
        the 256-MB Infinity Cache between kernels; the last block of each part
        writes its slice of the full-batch output (``width`` halfs per channel:
        1 fp16, 2 split)."""
        B = ims.n
        n = -(-B // parts)
        out = None
        for sub in range(0, B, n):
            nb = min(n, B - sub)
            x = stem(ims.part(sub, nb))
            for blk in self.p.blocks[:nfront - 1]:
                x = block(blk, x)
            blk = self.p.blocks[nfront - 1]
            if out is None:
                out = torch.empty((B, x.shape[1], x.shape[2], width * blk.convs[-1].cout), dtype=torch.float16,
                                  device=x.device)
            block(blk, x, out=out[sub:sub + nb])
        return out

    def _side_stream(self, device):
        st = self._side.get(device)
        if st is None:
            st = self._side[device] = torch.cuda.Stream(device=device)
        return st

    def _front_blocks(self) -> int:
        """Leading blocks that keep the stem's resolution (ResNet layer1)."""
        n = 0
        for blk in self.p.blocks:
            if any(c.stride != 1 for c in blk.convs) or (blk.down is not None and blk.down.stride != 1):
                break
            n += 1
        return n

    def _stem16(self, ims: _Images):
        """fp16 fused ResNet stem: the exact-u8 form (``stem_u8``) or the normalised-fp16 kernel."""
        o, s = self.ops, self.p.stem
        if self.stem_u8 and s.fs is not None:
            return o.stem_u8_f16(ims.img, s.fs, s.fs_bias, s.fs_psum, s.fs_scale, *ims.where)
        return o.stem_fused(ims.img, s.w, s.b, *ims.where)

    def forward(self, img_u8: torch.Tensor, start: torch.Tensor | None = None, batch: int = -1,
                start_offset: int = 0, packed: torch.Tensor | None = None, topk: int | None = None):
        """(class int32 [B], prob fp32 [B]); with ``packed`` the fused
        softmax-top1 also writes (class, prob bits) pairs into it.  An integer
        ``topk`` returns [B, topk] tensors instead (``ops.softmax_topk``: stable
        descending order, column 0 the top-1 result); not together with ``packed``."""
        topk = self._check_topk(topk, packed)
        z = self.logits(img_u8, start, batch, start_offset)
        if topk is not None:
            return self.ops.softmax_topk(z, topk, self._ovf if self._guarded() else None)
        return self.ops.softmax_top1(z, packed, self._ovf if self._guarded() else None)

    __call__ = forward

    # -- hipGraph -------------------------------------------------------------
    def _variant(self) -> tuple:
        """The values of ``GRAPH_SWITCHES`` (part of every graph's cache key)."""
        return tuple(int(self.fuse_down_tail) if n == "fuse_down_tail" else getattr(self, n)
                     for n in self.GRAPH_SWITCHES)

    def _capture_key(self, batch: int, packed=None, slot: int = 0, topk: int | None = None):
        if topk is not None:        # its own graphs; topk=None keeps the key it always had
            return (("topk", int(topk), batch, slot), self._variant())
        return ((batch if slot == 0 else (batch, slot)) if packed is None else ("pk", batch, packed.data_ptr()),
                self._variant())

    def _window_key(self, shard, batch, start, start_offset, packed):
        return ("win", shard.data_ptr(), tuple(shard.shape), batch, None if start is None else start.data_ptr(),
                start_offset, None if packed is None else packed.data_ptr(), self._variant())

    def has_graph(self, batch: int, packed=None, slot: int = 0, topk: int | None = None) -> bool:
        """Whether ``capture(batch, packed=, slot=, topk=)`` would replay an existing graph."""
        return self._capture_key(batch, packed, slot, self._check_topk(topk, packed)) in self._graphs

    def has_window(self, shard: torch.Tensor, batch: int, packed: torch.Tensor | None = None) -> bool:
        """A window graph over ``shard`` (own start scalar) is already captured."""
        return self._window_key(shard, batch, None, 0, packed) in self._graphs

    def _check_topk(self, topk, packed=None):
        """``topk`` as an int (or None).  The packed (RCCL round) format stays top-1 pairs."""
        if topk is None:
            return None
        if isinstance(topk, bool) or int(topk) != topk:
            raise ValueError(f"topk must be an integer or None, got {topk!r}")
        topk = int(topk)
        if packed is not None:
            raise ValueError("topk and packed cannot be combined: the packed result format is top-1 pairs")
        if not 1 <= topk <= min(16, self.p.num_classes):
            raise ValueError(f"topk must be in [1, {min(16, self.p.num_classes)}], got {topk}")
        return topk

    def _capture_graph(self, key, run, keep) -> None:
        """Warm ``run()`` (a forward on static buffers) up twice, capture it into
        a hipGraph and store (graph, ``keep`` = its static input, outputs) under ``key``."""
        with _CAPTURE_LOCK:  # one capture at a time per process; other threads keep launching
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._capturing = True        # warm-up launches: no flag reads (a capture follows)
                try:
                    for _ in range(2):
                        run()
                finally:
                    self._capturing = False
            torch.cuda.current_stream(self.device).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            self._capturing = True
            try:
                with _capture_nosync(g, self.device, self.graph_pool):
                    sout = run()
            finally:
                self._capturing = False
        self._graphs[key] = (g, keep, sout)

    def capture(self, batch: int, hw: int = 224, packed: torch.Tensor | None = None, slot: int = 0,
                topk: int | None = None):
        """Capture forward for a fixed batch; returns (static_in, replay_fn).
        With ``packed`` the graph also writes (class, prob bits) pairs into
        that caller-owned buffer (e.g. a collective round's send buffer).
        ``slot`` > 0 captures an independent copy (own static buffers), so two
        forwards of the same batch size can be in flight.  An integer ``topk``
        captures its own graph, whose replay returns [batch, topk] tensors."""
        topk = self._check_topk(topk, packed)
        key = self._capture_key(batch, packed, slot, topk)
        if key not in self._graphs:
            sin = torch.zeros(batch, hw, hw, 3, dtype=torch.uint8, device=self.device)
            self._capture_graph(key, lambda: self.forward(sin, packed=packed, topk=topk), sin)
        g, sin, sout = self._graphs[key]
        return sin, self._replayer(g, sout, packed)

    def capture_window(self, shard: torch.Tensor, batch: int, start: torch.Tensor | None = None,
                       start_offset: int = 0, packed: torch.Tensor | None = None, topk: int | None = None):
        """hipGraph of forward over a device-side window of ``shard``.

        Returns (start, replay): write the first image index into the int64
        GPU scalar ``start`` (a stream-ordered device op, e.g. from an RCCL
        broadcast of the query descriptor), then ``replay()`` -> (cls, prob).
        No host round trip and no staging copy of the images.  A caller-owned
        ``start`` (e.g. the start field of this rank's row of the broadcast
        descriptor table) is read in place, minus ``start_offset``; with
        ``packed`` the graph also writes (class, prob bits) pairs there (the
        gather's send buffer).  Window graphs serve the collective rounds,
        whose result format is top-1 pairs: an integer ``topk`` is refused."""
        if topk is not None:
            raise ValueError("capture_window has no top-k form: window graphs write the rounds' top-1 pairs")
        key = self._window_key(shard, batch, start, start_offset, packed)
        if key not in self._graphs:
            own = torch.zeros(1, dtype=torch.int64, device=self.device) if start is None else start
            self._capture_graph(key, lambda: self.forward(shard, own, batch, start_offset, packed), own)
        g, start, sout = self._graphs[key]
        return start, self._replayer(g, sout, shard, packed)

    def _replayer(self, g, sout, *keep):
        """Replay closure that keeps this runner (its HBM-resident weights) and
        the captured inputs alive: the graph holds raw device pointers, so a
        caller that drops the runner and keeps only the closure must not let
        the weights go back to the allocator."""
        direct = self.direct_launch and hasattr(g, "raw_cuda_graph_exec")
        launch = self.ops.load().graph_launch if direct else None

        def replay():
            # several nodes may share a process (and a GPU): a replay while another
            # thread is capturing fails on ROCm ("prepare for replay during
            # capturing stage"), so replays and captures are mutually exclusive
            with _CAPTURE_LOCK:
                if direct:
                    launch(g.raw_cuda_graph_exec())      # hipGraphLaunch on the current stream only
                else:
                    g.replay()
            return sout
        replay._keep = (self, keep)
        return replay

    def close(self) -> None:
        """Destroy the captured graphs now, under the capture lock (a graph
        destroyed by another thread's garbage collection while a capture is
        active aborts the process: hipErrorStreamCaptureUnsupported)."""
        with _CAPTURE_LOCK:
            self._graphs.clear()
            import gc

            gc.collect()

    def flops_per_image(self) -> float:
        """Useful (unpadded) FLOPs for one 224x224 image."""
        return program_flops(self.p)
