"""Process launcher: one node process per GPU on one MI355X host.

  python -m idunno.launch node --index I [--shell] [--executor hip|torch|fake]
        run node I (TCP control plane on base_port + I, GPU I % ngpu)
  python -m idunno.launch cluster --nodes N [--shell-node K]
        spawn N node processes as children; node K (default N-1) runs in the
        foreground with the interactive shell (reference: every VM runs
        ``python3 mp4_machinelearning.py`` and gets the REPL, README.md:26)

Config comes from ``--config file.{json,yaml}``, IDUNNO_* env vars and flags
(see ``idunno.config``).  Children are started with ``subprocess`` — never
``exec`` — so no GPU context is ever replaced in place.
"""
from __future__ import annotations

import argparse
import os
import signal
import subprocess
import sys
import threading
import time


def _cfg(a):
    from .config import ClusterConfig

    over = {"num_nodes": a.nodes, "base_port": a.base_port, "store_root": a.store_root,
            "log_dir": a.log_dir, "coordinator": a.coordinator, "standby": a.standby}
    cfg = ClusterConfig.load(a.config, **{k: v for k, v in over.items() if v is not None})
    if getattr(a, "weights", None):
        cfg.weights = {**cfg.weights, **parse_weights(a.weights)}
    return cfg


def parse_weights(items) -> dict:
    """``["resnet18=/path/r18.pth", ...]`` -> {canonical model name: absolute path}."""
    from .models.reference import canonical

    out = {}
    for it in items or []:
        model, sep, path = it.partition("=")
        if not sep or not model or not path:
            raise ValueError(f"--weights takes MODEL=PATH, got {it!r}")
        out[canonical(model)] = os.path.abspath(path)
    return out


def run_node(a) -> int:
    import logging

    import torch

    from .runtime.client import Client
    from .runtime.data import GpuJpegSource, SdfsSource, SyntheticSource
    from .runtime.executor import make_executor
    from .runtime.node import Node
    from .runtime.shell import Shell
    from .runtime.transport import TcpTransport

    logging.basicConfig(level=logging.WARNING, format="%(asctime)s %(name)s %(message)s")
    cfg = _cfg(a)
    name = cfg.node_name(a.index)
    if torch.cuda.is_available() and a.executor in ("auto", "hip"):
        dev = torch.device("cuda", a.index % torch.cuda.device_count())
        torch.cuda.set_device(dev)
    else:
        dev = torch.device("cpu")
    ex = make_executor(a.executor, dev if dev.type == "cuda" else None, seed=cfg.model_seed, dtype=cfg.dtype,
                       fp32_impl=cfg.fp32_impl, weights=cfg.weights)
    if cfg.collective_rounds is None:
        # one node per process and per GPU: queries run as RCCL rounds by default
        # (RCCL needs a distinct GPU per rank; nodes sharing a GPU use the TCP path)
        cfg.collective_rounds = dev.type == "cuda" and a.executor in ("auto", "hip") and \
            torch.cuda.device_count() >= cfg.num_nodes      # (a single node: one-member rounds)
    tr = TcpTransport(name, cfg.address, cfg.address(name))
    node = Node(cfg, name, tr, ex)
    if a.source == "jpeg":
        # real files: `put` test_<i>.JPEG into SDFS, then `inference <start> <end> <model>`
        node.source = GpuJpegSource(sdfs=node.sdfs, device=dev, entropy_on=a.jpeg_entropy,
                                    progressive=a.jpeg_progressive, restart=a.jpeg_restart,
                                    sampling=a.jpeg_sampling, colorspace=a.jpeg_colorspace)
    else:
        node.source = (SdfsSource(node.sdfs, dev, peer_copy=cfg.sdfs_peer_copy) if a.source == "sdfs"
                       else SyntheticSource(cfg.data_seed, dev))
    if a.index != cfg.coordinator:
        time.sleep(a.join_delay)
    node.start(join=True)
    if a.shell:
        Shell(node, Client(node)).repl()
        node.stop()
        return 0
    stop = threading.Event()
    signal.signal(signal.SIGTERM, lambda *_: stop.set())
    signal.signal(signal.SIGINT, lambda *_: stop.set())
    while not stop.wait(0.5) and node.alive_flag:
        pass
    node.stop()
    return 0


def run_cluster(a) -> int:
    cfg = _cfg(a)
    shell_node = cfg.num_nodes - 1 if a.shell_node is None else a.shell_node
    procs = []
    base = [sys.executable, "-m", "idunno.launch", "node", "--executor", a.executor, "--source", a.source,
            "--jpeg-entropy", a.jpeg_entropy, "--jpeg-progressive", a.jpeg_progressive,
            "--jpeg-restart", a.jpeg_restart, "--jpeg-sampling", a.jpeg_sampling,
            "--jpeg-colorspace", a.jpeg_colorspace]
    for flag, v in (("--config", a.config), ("--nodes", cfg.num_nodes), ("--base-port", cfg.base_port),
                    ("--store-root", cfg.store_root), ("--log-dir", a.log_dir)):
        if v is not None:
            base += [flag, str(v)]
    for w in a.weights or []:
        base += ["--weights", w]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for i in range(cfg.num_nodes):
        if i == shell_node and not a.no_shell:
            continue
        procs.append(subprocess.Popen(base + ["--index", str(i)], env=env, stdin=subprocess.DEVNULL))
    rc = 0
    try:
        if not a.no_shell:
            a2 = argparse.Namespace(**vars(a))
            a2.index, a2.shell = shell_node, True
            rc = run_node(a2)
        else:
            for p in procs:
                p.wait()
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()
    return rc


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["node", "cluster"])
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--base-port", type=int, default=None)
    ap.add_argument("--store-root", default=None)
    ap.add_argument("--log-dir", default=None)
    ap.add_argument("--coordinator", type=int, default=None)
    ap.add_argument("--standby", type=int, default=None)
    ap.add_argument("--executor", default="auto", choices=["auto", "hip", "torch", "fake"])
    ap.add_argument("--source", default="synthetic", choices=["synthetic", "sdfs", "jpeg"])
    ap.add_argument("--jpeg-entropy", default="host", choices=["host", "gpu", "gpu_parallel"],
                    help="--source jpeg: Huffman decode on host threads, or on the device (no decode threads): "
                         "gpu = one lane per image, gpu_parallel = one workgroup per image")
    ap.add_argument("--jpeg-progressive", default="fallback", choices=["fallback", "native"],
                    help="--source jpeg: progressive files through Pillow, or decoded natively")
    ap.add_argument("--jpeg-restart", default="lane", choices=["lane", "intervals"],
                    help="--source jpeg with a device --jpeg-entropy: a file with restart markers on one lane, or one "
                         "restart interval per lane")
    ap.add_argument("--jpeg-sampling", default="fallback", choices=["fallback", "native"],
                    help="--source jpeg: 4:4:0 and 4:1:1 files through Pillow, or decoded natively")
    ap.add_argument("--jpeg-colorspace", default="ycbcr", choices=["ycbcr", "auto"],
                    help="--source jpeg: every three-component file taken for YCbCr and CMYK / YCCK through Pillow, or "
                         "the colour model read from the file and RGB / CMYK / YCCK decoded natively")
    ap.add_argument("--weights", action="append", default=None, metavar="MODEL=PATH",
                    help="checkpoint file for a model (repeatable); every node reads the same file")
    ap.add_argument("--shell", action="store_true")
    ap.add_argument("--shell-node", type=int, default=None)
    ap.add_argument("--no-shell", action="store_true")
    ap.add_argument("--join-delay", type=float, default=0.5)
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    return run_node(a) if a.mode == "node" else run_cluster(a)


if __name__ == "__main__":
    sys.exit(main())
