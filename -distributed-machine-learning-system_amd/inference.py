"""Single-process inference entry point — the reference's L4 API
``deeplearning(filename, modelname, start_image, end_image)``
(alexnet_resnet.py:12-92) re-built on resident models.

    results, seconds = deeplearning("resnet18", "resnet18", 0, 399)
    # results: [("test_0.JPEG", "<category>", prob), ...]  (end inclusive)

Differences from the reference, all deliberate:
  * the model is built once per (model, device) and cached, not re-loaded from
    torch.hub on every call (A6); weights are random-init unless ``weights``
    names a checkpoint file on disk (nothing is downloaded);
  * images ``./<filename>/test_<i>.JPEG`` are decoded in memory and never
    rewritten on disk (A14); when the directory does not exist the
    deterministic synthetic 224x224x3 dataset of the cluster is used instead;
  * the chunk runs as batched forwards of ``batch`` images (``batch=1`` keeps
    the reference's one-image-at-a-time behaviour) — on the HIP kernels when a
    GPU is present, else on the fp32 PyTorch modules (CPU plumbing path,
    BASELINE.json config 1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import torch

from .models.checkpoint import file_key
from .models.reference import canonical
from .runtime.data import GpuJpegSource, JpegSource, SyntheticSource
from .runtime.executor import HipExecutor, TorchExecutor
from .runtime.jobstate import class_names

_EXECUTORS: dict = {}
# (device, directory, entropy_on, progressive, restart, colorspace, sampling) -> GpuJpegSource: its decoded images stay resident across calls, keyed by
# index only; after replacing files of a directory call drop_gpu_sources()
_GPU_SOURCES: dict = {}
_LOCK = threading.Lock()


def _executor(device: torch.device, seed: int, model: str | None = None, weights=None):
    if weights is None:
        key, wmap = (str(device), seed), None
    else:
        # (abspath, size, mtime_ns): a replaced checkpoint file gets a fresh executor
        key, wmap = (str(device), seed, model, file_key(weights)), {model: os.fspath(weights)}
    with _LOCK:
        ex = _EXECUTORS.get(key)
        if ex is None:
            ex = (HipExecutor(device, seed=seed, weights=wmap) if device.type == "cuda"
                  else TorchExecutor(device, seed=seed, weights=wmap))
            _EXECUTORS[key] = ex
    return ex


def drop_gpu_sources() -> None:
    """Forget the images ``decoder="gpu"`` calls keep resident in HBM."""
    with _LOCK:
        _GPU_SOURCES.clear()


def deeplearning(filename: str, modelname: str, start_image: int, end_image: int, *,
                 device: str | torch.device | None = None, batch: int | None = None, seed: int = 0,
                 data_seed: int = 1234, root: str = ".", decoder: str = "pil", entropy_on: str = "host",
                 progressive: str = "fallback", restart: str = "lane", topk: int = 1, weights=None,
                 classes: str | None = None, sampling: str = "fallback", colorspace: str = "ycbcr"):
    """Classify images ``start_image..end_image`` (inclusive).  Returns
    ``(list[(image_name, category, prob)], elapsed_seconds)`` like the reference.
    ``topk`` > 1 (at most 16) returns ``(image_name, (cat_1..cat_k),
    (p_1..p_k))`` per image instead: the k most probable categories, most
    probable first, equal probabilities in class order.  ``weights`` is a
    checkpoint file for ``modelname`` (``.safetensors``, or a ``torch.save``d
    state dict read weights-only; torchvision's parameter names, 1000 classes);
    a file replaced on disk is loaded again.  ``classes`` is a file of category
    names, one per line (default: ``$IDUNNO_CLASSES``, else ``class_<i>``).
    Without ``weights`` the parameters are random-init from ``seed``.
    ``decoder="gpu"`` decodes the JPEG files with the native entropy decoder and
    the HIP kernels (``GpuJpegSource``: decoded images stay in HBM across calls
    by index -- ``drop_gpu_sources()`` after replacing files; without a GPU it
    decodes with Pillow like ``"pil"``).  ``entropy_on="gpu"`` (with
    ``decoder="gpu"``) also decodes the Huffman streams on the device instead of
    on host threads, one lane per image, and ``"gpu_parallel"`` does so with one
    workgroup per image; the default is ``"host"``.  ``progressive="native"``
    (with ``decoder="gpu"``) decodes progressive JPEG files natively in that
    form instead of handing them to Pillow; the default is ``"fallback"``.
    ``restart="intervals"`` (with ``decoder="gpu"`` and a device
    ``entropy_on``) decodes baseline files with a restart interval one interval
    per lane instead of on one lane; the default is ``"lane"``.
    ``sampling="native"`` (with ``decoder="gpu"``) decodes 4:4:0 and 4:1:1
    JPEG files natively instead of handing them to Pillow; the default is
    ``"fallback"``.
    ``colorspace="auto"`` (with ``decoder="gpu"``) reads the colour model of a
    JPEG file from its JFIF / Adobe markers and component ids as libjpeg does
    and decodes RGB-coded, CMYK and YCCK files natively.  Under the default
    ``"ycbcr"`` CMYK / YCCK files go to Pillow and an RGB-coded
    three-component file is decoded as YCbCr, which gives wrong colours."""
    if decoder not in ("pil", "gpu"):
        raise ValueError(f"decoder must be 'pil' or 'gpu', not {decoder!r}")
    if entropy_on not in ("host", "gpu", "gpu_parallel"):
        raise ValueError(f"entropy_on must be 'host', 'gpu' or 'gpu_parallel', not {entropy_on!r}")
    if progressive not in ("fallback", "native"):
        raise ValueError(f"progressive must be 'fallback' or 'native', not {progressive!r}")
    if restart not in ("lane", "intervals"):
        raise ValueError(f"restart must be 'lane' or 'intervals', not {restart!r}")
    if sampling not in ("fallback", "native"):
        raise ValueError(f"sampling must be 'fallback' or 'native', not {sampling!r}")
    if colorspace not in ("ycbcr", "auto"):
        raise ValueError(f"colorspace must be 'ycbcr' or 'auto', not {colorspace!r}")
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= 16:
        raise ValueError(f"topk must be an integer in [1, 16], not {topk!r}")
    t0 = time.time()
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    device = torch.device(device)
    model = canonical(modelname)
    ex = _executor(device, seed, model, weights)
    d = os.path.join(root, filename)
    if not os.path.isdir(d):
        src = SyntheticSource(data_seed, device)
    elif decoder == "gpu":
        with _LOCK:
            key = (str(device), os.path.abspath(d), entropy_on, progressive, restart, colorspace, sampling)
            src = _GPU_SOURCES.get(key)
            if src is None:
                src = _GPU_SOURCES[key] = GpuJpegSource(device, root=d, entropy_on=entropy_on, progressive=progressive,
                                                              restart=restart, sampling=sampling, colorspace=colorspace)
    else:
        src = JpegSource(device, root=d)
    names = class_names(path=classes)
    n = end_image - start_image + 1
    batch = n if not batch or batch <= 0 else batch
    out = []
    for s in range(start_image, end_image + 1, batch):
        e = min(s + batch - 1, end_image)
        if topk > 1:
            cls, prob = ex.run(model, src.get(s, e), s, e, topk=topk)
            out += [(f"test_{s + i}.JPEG", tuple(names[int(c)] for c in cs), tuple(float(p) for p in ps))
                    for i, (cs, ps) in enumerate(zip(cls, prob))]
            continue
        cls, prob = ex.run(model, src.get(s, e), s, e)
        out += [(f"test_{s + i}.JPEG", names[int(c)], float(p)) for i, (c, p) in enumerate(zip(cls, prob))]
    return out, time.time() - t0


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="one-process inference over test_<i>.JPEG (or synthetic) images")
    ap.add_argument("model", help="alexnet | resnet18 | resnet | resnet34 | resnet50 | resnet101 | resnet152 | resnext50_32x4d | "
                                  "resnext101_32x8d | wide_resnet50_2 | wide_resnet101_2")
    ap.add_argument("start", type=int)
    ap.add_argument("end", type=int)
    ap.add_argument("--dir", default=None, help="image directory (default: ./<model>, else synthetic)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--batch", type=int, default=0, help="images per forward (1 = reference behaviour)")
    ap.add_argument("--decoder", default="pil", choices=["pil", "gpu"],
                    help="JPEG decode: Pillow on host threads, or native entropy decode + HIP kernels")
    ap.add_argument("--entropy", default="host", choices=["host", "gpu", "gpu_parallel"],
                    help="with --decoder gpu: Huffman decode on host threads, on the device (one lane per image), "
                         "or on the device with one workgroup per image")
    ap.add_argument("--progressive", default="fallback", choices=["fallback", "native"],
                    help="with --decoder gpu: progressive JPEG files through Pillow, or decoded natively")
    ap.add_argument("--restart", default="lane", choices=["lane", "intervals"],
                    help="with --decoder gpu and a device --entropy: a file with restart markers on one lane, or one "
                         "restart interval per lane")
    ap.add_argument("--sampling", default="fallback", choices=["fallback", "native"],
                    help="with --decoder gpu: 4:4:0 and 4:1:1 JPEG files through Pillow, or decoded natively")
    ap.add_argument("--colorspace", default="ycbcr", choices=["ycbcr", "auto"],
                    help="with --decoder gpu: every three-component JPEG file taken for YCbCr and CMYK / YCCK files "
                         "through Pillow, or the colour model read from the file and RGB / CMYK / YCCK decoded natively")
    ap.add_argument("--topk", type=int, default=1, help="categories per image, most probable first (1..16)")
    ap.add_argument("--weights", default=None,
                    help="checkpoint file for the model (.safetensors or a torch.save'd state dict); default random-init")
    ap.add_argument("--classes", default=None, help="file of category names, one per line")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    res, dt = deeplearning(a.dir or a.model, a.model, a.start, a.end, device=a.device, batch=a.batch,
                           decoder=a.decoder, entropy_on=a.entropy, progressive=a.progressive, restart=a.restart,
                           topk=a.topk, weights=a.weights, classes=a.classes, sampling=a.sampling,
                           colorspace=a.colorspace)
    for r in res:
        print(json.dumps(r))
    print(f"{len(res)} images in {dt:.3f} s ({len(res) / max(dt, 1e-9):.1f} img/s)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
