"""Trained checkpoints for the reference architectures.

The module trees of ``models.reference`` use torchvision's parameter names, so
a ``state_dict`` saved from torchvision's ``alexnet`` or any member of its
v0.10 ResNet family (``resnet18/34/50/101/152``, ``resnext50_32x4d``,
``resnext101_32x8d``, ``wide_resnet50_2``, ``wide_resnet101_2``; a grouped
``conv2.weight`` is ``[width, width // groups, 3, 3]``), or from
``reference.build``, loads strictly:

    state = load_state("resnet18.pth")            # or .safetensors
    m = model_from_state("resnet18", state)       # nn.Module, eval mode
    prog = build_program("resnet18", dtype="fp32", weights="resnet18.pth")

Files are read with ``torch.load(weights_only=True)`` (never a full unpickle)
or ``safetensors``.  Only 1000-class heads are accepted: no FC shape that the
kernels have not been tested on.  Nothing here downloads anything.
"""
from __future__ import annotations

import hashlib
import os

import torch
from torch import nn

from . import reference as ref

NUM_CLASSES = 1000
_WRAPPERS = ("state_dict", "model")
_CAST = (torch.float16, torch.bfloat16, torch.float64)
_SHOWN = 5       # offending keys named in an error


def _is_state(d) -> bool:
    return isinstance(d, dict) and len(d) > 0 and all(
        isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in d.items())


def normalise_state(state: dict) -> dict:
    """A bare state dict from ``state`` (itself, or the one under
    ``"state_dict"`` / ``"model"``): a uniform ``module.`` prefix stripped,
    ``num_batches_tracked`` dropped, fp16 / bf16 / fp64 tensors cast to fp32."""
    if not isinstance(state, dict):
        raise ValueError(f"checkpoint holds a {type(state).__name__}, not a state dict")
    if not _is_state(state):
        for w in _WRAPPERS:
            if _is_state(state.get(w)):
                state = state[w]
                break
        else:
            raise ValueError("checkpoint is not a state dict (name -> tensor), nor holds one under "
                             f"{' / '.join(map(repr, _WRAPPERS))}")
    if all(k.startswith("module.") for k in state):
        state = {k[len("module."):]: v for k, v in state.items()}
    out = {}
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            continue
        v = v.detach()
        out[k] = v.float() if v.dtype in _CAST else v
    return out


def load_state(path) -> dict:
    """The state dict stored in ``path``, on the CPU (see ``normalise_state``).
    ``.safetensors`` files are read with ``safetensors``; anything else with
    ``torch.load(weights_only=True)``, which refuses pickled objects other than
    tensors and plain containers."""
    path = os.fspath(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        raw = load_file(path, device="cpu")
    else:
        try:
            raw = torch.load(path, map_location="cpu", weights_only=True)
        except ValueError:
            raise
        except Exception as e:       # pickle.UnpicklingError, RuntimeError, EOFError ...
            raise ValueError(f"{path}: not a weights-only checkpoint ({type(e).__name__}: {e})") from e
    try:
        return normalise_state(raw)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from e


def _few(keys) -> str:
    keys = list(keys)
    more = f" (+{len(keys) - _SHOWN} more)" if len(keys) > _SHOWN else ""
    return ", ".join(keys[:_SHOWN]) + more


def model_from_state(name: str, state: dict) -> nn.Module:
    """A fresh ``reference.BUILDERS[name]()`` with ``state`` loaded strictly,
    in eval mode.  ``ValueError`` (naming the model and the first offending
    keys) for missing or unexpected keys, shape mismatches, non-finite values
    and a head that is not 1000 classes."""
    name = ref.canonical(name)
    state = normalise_state(state)
    m = ref.BUILDERS[name]()
    want = m.state_dict()
    want = {k: v for k, v in want.items() if not k.endswith("num_batches_tracked")}
    head = "fc" if isinstance(m, ref.ResNet) else "classifier.6"
    hw = state.get(head + ".weight")
    if hw is not None and hw.dim() == 2 and hw.shape[0] != NUM_CLASSES:
        raise ValueError(f"{name}: the head {head} has {hw.shape[0]} classes; only {NUM_CLASSES}-class "
                         "checkpoints are supported")
    missing = [k for k in want if k not in state]
    extra = [k for k in state if k not in want]
    if missing or extra:
        parts = []
        if missing:
            parts.append(f"missing keys: {_few(missing)}")
        if extra:
            parts.append(f"unexpected keys: {_few(extra)}")
        raise ValueError(f"{name}: checkpoint does not match the architecture; " + "; ".join(parts))
    # conv / linear weights first: the per-channel vectors that differ with them (BN, bias) say nothing more,
    # and a ResNeXt checkpoint offered as a ResNet should name the grouped conv2 among the first few
    shape = [f"{k} {tuple(state[k].shape)} != {tuple(v.shape)}"
             for first in (True, False) for k, v in want.items()
             if state[k].shape != v.shape and (v.dim() >= 2) == first]
    if shape:
        raise ValueError(f"{name}: shape mismatch: {_few(shape)}")
    bad = [k for k in want if not state[k].is_floating_point()]
    if bad:
        raise ValueError(f"{name}: non-floating-point tensors: {_few(bad)}")
    bad = [k for k in want if not bool(torch.isfinite(state[k]).all())]
    if bad:
        raise ValueError(f"{name}: non-finite values in: {_few(bad)}")
    try:
        m.load_state_dict(state, strict=True)
    except RuntimeError as e:
        raise ValueError(f"{name}: {e}") from e
    return m.eval()


def load_model(name: str, weights) -> nn.Module:
    """``model_from_state`` of a path or a state dict."""
    state = weights if isinstance(weights, dict) else load_state(weights)
    return model_from_state(name, state)


def state_digest(m_or_state) -> str:
    """SHA-256 over (name, dtype, shape, bytes) of every tensor in key order:
    two nodes that print the same digest serve the same parameters."""
    state = m_or_state.state_dict() if isinstance(m_or_state, nn.Module) else m_or_state
    h = hashlib.sha256()
    for k in sorted(state):
        if k.endswith("num_batches_tracked"):
            continue
        v = state[k].detach().cpu().contiguous()
        h.update(f"{k}|{v.dtype}|{tuple(v.shape)}|".encode())
        h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def file_key(path) -> tuple:
    """(abspath, size, mtime_ns): changes when the file is replaced."""
    p = os.path.abspath(os.fspath(path))
    st = os.stat(p)
    return (p, st.st_size, st.st_mtime_ns)
