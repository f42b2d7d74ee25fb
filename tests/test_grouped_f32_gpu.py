"""conv3x3_grouped_f32.hip and the runner switch ``grouped_f32`` against fp64 on the CPU.  Bound: 2e-5 of the max
magnitude, as tests/test_kernels_f32_gpu.py::_check; torch's fp32 conv is within 6e-7 on these inputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

from idunno import ops
from idunno.models import HipRunner
from idunno.models import packed as P
from idunno.models import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [                        # (B, H, W, C, groups, stride): the smallest shapes that reach each code path
    (1, 9, 13, 64, 16, 1),       # Cg 4, ragged
    (3, 15, 15, 64, 8, 2),       # Cg 8, odd H at stride 2
    (1, 6, 6, 128, 8, 2),        # Cg 16
    (1, 7, 7, 256, 8, 1),        # Cg 32
    (1, 7, 7, 128, 2, 1),        # Cg 64
    (1, 1, 1, 64, 16, 1),        # only the centre tap is not padding
    (1, 2, 5, 128, 32, 2),       # tiny, strided
    (1, 5, 6, 96, 24, 1),        # half slab
    (2, 9, 17, 160, 5, 2),       # Cg 32, stride 2, half slab
    (1, 10, 33, 64, 4, 1),       # two tile rows, three tile columns
]


@functools.lru_cache(maxsize=None)
def _case(case):
    # tests/test_grouped_gpu.py::_case: one group's input channels are 64 x the others' (a leaked tap shows)
    B, H, W, C, groups, stride = case
    cg = C // groups
    g = torch.Generator().manual_seed(sum(case) + 1000 * groups)
    x = torch.randn(B, H, W, C, generator=g)
    x[..., cg:2 * cg] *= 64.0                                  # group 1 (groups >= 2)
    w = torch.randn(C, cg, 3, 3, generator=g) / (9 * cg) ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride, 1, groups=groups)
    return x, w, b, y.permute(0, 2, 3, 1).contiguous()


def _check(got, want, what):
    err = (got.double().cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
    print(f"{what}: rel err {err:.2e}")
    assert err <= 2e-5, f"{what}: rel err {err:.2e}"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_grouped_f32_kernel_vs_fp64(case, relu):
    groups, stride = case[4:]
    x, w, b, want = _case(case)
    y = ops.conv3x3_grouped_f32(x.to(DEV), P.pack_grouped_f32_weight(w, groups).to(DEV), b.to(DEV), groups, stride, relu)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape)
    _check(y, F.relu(want) if relu else want, f"grouped f32 {case} relu={relu}")


def test_grouped_f32_binding_checks_name_the_operand():
    def mk(c=64, groups=16, cb=16, b=1):
        return dict(x=torch.zeros(b, 4, 4, c, device=DEV), w=torch.zeros(c, 9 * cb, device=DEV),
                    bias=torch.zeros(c, device=DEV), groups=groups, stride=1, relu=True)

    fn = ops.conv3x3_grouped_f32
    assert tuple(fn(**mk()).shape) == (1, 4, 4, 64)                            # the valid call is accepted
    assert tuple(fn(**dict(mk(b=0), stride=2)).shape) == (0, 2, 2, 64)         # an empty batch returns at once
    bad = [
        (r"\bx has wrong dtype", dict(mk(), x=mk()["x"].half())),
        (r"\bw has wrong dtype", dict(mk(), w=mk()["w"].half())),
        (r"\bbias has wrong dtype", dict(mk(), bias=mk()["bias"].half())),
        (r"\bx must be a GPU tensor", dict(mk(), x=mk()["x"].cpu())),
        (r"\bx must have rank 4", dict(mk(), x=mk()["x"][0])),
        (r"groups: 24 .* divide x's C = 64", dict(mk(), groups=24)),
        (r"groups: C / groups = 12 ", dict(mk(96, 8, 16))),
        (r"stride must be 1 or 2, got 3", dict(mk(), stride=3)),
        (r"\bw: must be \[", dict(mk(), w=torch.zeros(64, 9 * 64, device=DEV))),
    ]
    for pattern, kw in bad:
        with pytest.raises(RuntimeError, match=pattern):
            fn(**kw)


def _resnext(seed, stem_gain, img_seed):
    from idunno.runtime.data import synth_images_cpu

    m = ref.build("resnext50_32x4d", seed=seed)
    m.conv1.weight.data *= stem_gain
    r = HipRunner(P.compile_model(m, "resnext50_32x4d", "fp32"))
    r.grouped_f32 = True
    img = torch.from_numpy(synth_images_cpu(img_seed, 0, 2))
    with torch.no_grad():
        want = m.double()(ref.preprocess_u8(img).double())
    return r, img.to(DEV), want


def test_f32_mfma_path_runs_resnext_on_the_grouped_kernel():
    r, img, want = _resnext(0, 1.0, 0)
    r.split = False
    _check(r.logits(img), want, "resnext50_32x4d, split off, grouped f32 kernel")
    assert not r._gdense
    r.grouped_dense = True                                                     # the dense arm still runs
    _check(r.logits(img), want, "resnext50_32x4d, split off, dense arm")
    assert len(r._gdense) == 16


def test_range_guard_rerun_takes_the_grouped_f32_kernel():
    r, img, want = _resnext(3, 1e5, 4)                         # test_resnext_range_guard_rerun_matches_fp64's setup
    assert r.split and r._split_ok()
    got = r.logits(img)
    assert r.overflow_reruns == 1 and not r._gdense                            # the guard tripped; no expansion
    _check(got, want, "guard rerun on the grouped f32 kernel")
