"""The fused layer-1 basic-block kernel (conv3x3_split_block.hip) on the GPU.

ops.conv3x3_split_block computes relu(conv_b(relu(conv_a(x))) + x) in one launch; every
accumulator receives the MFMAs of the one-conv kernel (tile 50) in the same order and the
intermediate is rounded by the same split, so the result must be ``torch.equal`` to
``ops.conv2d_split(..., tile=50)`` applied twice with the residual, whatever the band
split.  ``grid`` caps the persistent grid so that small tensors run several bands per
workgroup (bands that span images, odd-length bands, one-row bands).
"""
import pytest
import torch
import torch.nn.functional as F

import c64_block_cases as BC
import exact_ref as X
from idunno.models import HipRunner, build_program
from idunno.models import packed as P

DEV = "cuda"
pytestmark = pytest.mark.gpu

# (B, H, W, grids): 0 = one workgroup per CU (capped at one per row)
CASES = [
    (2, 56, 56, (0, 5)),
    (3, 13, 49, (0, 4)),
    (1, 9, 52, (0, 2)),
    (40, 56, 56, (0,)),
    (150, 13, 52, (0, 37)),      # 0: 7-8-row bands that span images; 37: 52-53-row bands over 4-5 images
    (5, 1, 56, (0, 2)),          # images shorter than the halo
    (4, 2, 50, (0, 3)),
]


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _weights(seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(2):
        w = torch.randn(64, 64, 3, 3, generator=g) / 24 * (gain if k == 0 else 1.0)
        b = torch.randn(64, generator=g) * 0.1
        sw, scale = P.pack_split_weight(w)
        out.append((w, b, sw.to(DEV), b.to(DEV), scale))
    return out


def _two_launches(ops, xs, wa, wb):
    y = ops.conv2d_split(xs, wa[2], wa[3], wa[4], 3, 3, 1, 1, True, tile=50)
    return ops.conv2d_split(y, wb[2], wb[3], wb[4], 3, 3, 1, 1, True, residual=xs, tile=50)


@pytest.mark.parametrize("B,H,W,grids", CASES)
def test_block_bit_identical_to_two_launches(ops, B, H, W, grids):
    torch.manual_seed(B * H + W)
    x = torch.randn(B, H, W, 64, device=DEV)
    xs = ops.split_from_f32(x)
    wa, wb = _weights(B + H + W)
    want = _two_launches(ops, xs, wa, wb)
    for grid in grids:
        got = ops.conv3x3_split_block(xs, wa[2], wa[3], wa[4], wb[2], wb[3], wb[4], grid=grid)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"grid {grid}: {(got != want).sum().item()} halfs differ"


@pytest.mark.parametrize("B,H,W,grids", CASES)
def test_block_tolerance_fp64(ops, B, H, W, grids):
    """The fused output itself against the fp64 reference (computed on the GPU) at the
    project's fp32 tolerance, 2e-5 of the output scale, on randn data."""
    torch.manual_seed(B * H + W + 1)
    x = torch.randn(B, H, W, 64, device=DEV)
    wa, wb = _weights(B + H + W + 1)
    got = ops.conv3x3_split_block(ops.split_from_f32(x), wa[2], wa[3], wa[4], wb[2], wb[3], wb[4], grid=grids[-1])
    xn = x.double().permute(0, 3, 1, 2)
    y = F.relu(F.conv2d(xn, wa[0].double().to(DEV), wa[1].double().to(DEV), 1, 1))
    ref = F.relu(F.conv2d(y, wb[0].double().to(DEV), wb[1].double().to(DEV), 1, 1) + xn).permute(0, 2, 3, 1)
    err = (P.from_split(got).double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-5 * scale, f"max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("B,H,W", BC.SHAPES)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_block_exact_oracle(ops, kind, B, H, W):
    """Against the arithmetic-contract oracle of exact_ref.py, composed conv a then conv b
    (c64_block_cases.py): non-canonical x planes, which are also the residual; wide
    weights (w_lo != 0) in conv a or in conv b; both planes ``torch.equal``.  The two
    launches are held to the same expectation.  No case may raise the range guard."""
    case_a, case_b, xs, expect, ref = BC.block_case(kind, B, H, W)
    xs = xs.to(DEV)
    wa, wb = case_a.sw.to(DEV), case_b.sw.to(DEV)
    ba, bb = case_a.bias.float().to(DEV), case_b.bias.float().to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.set_split_guard(flag)
    try:
        outs = {f"fused grid {g}": ops.conv3x3_split_block(xs, wa, ba, case_a.scale, wb, bb, case_b.scale, grid=g)
                for g in (0, 3)}
        y = ops.conv2d_split(xs, wa, ba, case_a.scale, 3, 3, 1, 1, True, tile=50)
        outs["two launches"] = ops.conv2d_split(y, wb, bb, case_b.scale, 3, 3, 1, 1, True, residual=xs, tile=50)
    finally:
        ops.set_split_guard(None)
    torch.cuda.synchronize()
    fails = []
    for label, got in outs.items():
        try:
            X.assert_bits(got, expect, ref, split=True)
        except AssertionError as e:
            fails.append(f"{label}: {e}")
    assert not fails, "\n".join(fails)
    assert int(flag.item()) == 0


def test_block_range_guard(ops):
    """conv a's output past 65504 has no finite hi half: the guard flag is set, as it is
    by the unfused conv a."""
    torch.manual_seed(9)
    xs = ops.split_from_f32(torch.randn(2, 9, 52, 64, device=DEV))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(fn):
        flag.zero_()
        ops.set_split_guard(flag)
        try:
            fn()
        finally:
            ops.set_split_guard(None)
        torch.cuda.synchronize()
        return int(flag.item())

    for gain, want in ((1.0, 0), (1e5, 1)):
        wa, wb = _weights(4, gain)
        assert run(lambda: ops.conv2d_split(xs, wa[2], wa[3], wa[4], 3, 3, 1, 1, True, tile=50)) == want
        assert run(lambda: ops.conv3x3_split_block(xs, wa[2], wa[3], wa[4], wb[2], wb[3], wb[4], grid=3)) == want


def test_block_ok_threshold(ops):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b_min = -(-16 * cus // 56)
    assert ops.conv3x3_split_block_ok(b_min, 56, 56, 64, 64)
    assert not ops.conv3x3_split_block_ok(b_min - 1, 56, 56, 64, 64)
    assert not ops.conv3x3_split_block_ok(400, 56, 57, 64, 64)
    assert not ops.conv3x3_split_block_ok(400, 56, 48, 64, 64)
    assert not ops.conv3x3_split_block_ok(400, 56, 56, 128, 128)


def test_whole_model_fused_equals_unfused(ops):
    """ResNet18 logits with fuse_block_c64 0 and 1; the switch routes at any batch the
    library fuses by default, so the small batch here goes through a runner whose rule
    is widened to every supported shape."""
    prog = build_program("resnet18", dtype="fp32")
    img = ops.synth_images(7, 0, 8, torch.device(DEV))
    outs = {}
    for flag in (0, 1):
        r = HipRunner(prog, DEV)
        r.fuse_block_c64 = flag
        if flag:
            ok = r._block_c64_ok
            fused = []
            r.ops = _AlwaysOk(ops, fused)
            assert ok(prog.blocks[0], torch.empty(8, 56, 56, 128, device=DEV))
        eager = r.logits(img).clone()
        _s, run = r.capture_window(img, 8)
        replays = [tuple(t.clone() for t in run()) for _ in range(2)]
        torch.cuda.synchronize()
        outs[flag] = (eager, replays)
        if flag:
            assert len(fused) >= 2, "the fused kernel did not run"
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip(outs[1][1][0], outs[1][1][1]))


class _AlwaysOk:
    """ops with the fused block's batch rule dropped (supported shapes only) and its calls counted."""

    def __init__(self, ops, calls):
        self._ops, self._calls = ops, calls

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def conv3x3_split_block_ok(self, b, h, w, c, cout):
        return c == 64 and cout == 64 and 49 <= w <= 56

    def conv3x3_split_block(self, *a, **k):
        self._calls.append(1)
        return self._ops.conv3x3_split_block(*a, **k)
