"""Model families of the reference (AlexNet, ResNet18) plus the rest of
torchvision v0.10's ResNet family (ResNet34-152, ResNeXt, Wide ResNet).

``reference``  plain-PyTorch fp32 oracle modules (torchvision-compatible keys)
``packed``     BN-folded, MFMA-packed inference programs + their fp32 CPU emulator
``runner``     ``HipRunner``: a packed program on the HIP kernels, hipGraph capture
"""
from . import reference
from .packed import Program, build_program, compile_model, emulate, program_flops
from .reference import canonical
from .runner import HipRunner

__all__ = ["reference", "HipRunner", "Program", "build_program", "compile_model", "emulate",
           "program_flops", "canonical"]
