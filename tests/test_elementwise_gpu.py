"""The memory-bound HIP kernels (resize_crop, max pools, global average pool,
softmax_top1, split conversions) against the float64 references of
tests/elementwise_ref.py, at the small shapes where such kernels go wrong: odd
sizes, W != H, one and several blocks, every thread-map regime of the average
pool, rows around softmax_top1's four-rows-per-block boundary.  Inputs are
seeded noise, so a one-pixel shift or a swapped tap shows at full amplitude."""
import pytest
import torch
from elementwise_ref import (GREY, RESIZE_CASES, RESIZE_MARGIN, avgpool_ref, center_crop_geometry, half_ulp_f16,
                             maxpool_ref, resize_case_image, resize_crop_ref, softmax_top1_ref)

from idunno.models import packed as P

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _check_rel(y, ref, rel):
    """tests/test_split.py's _check: max error relative to the reference's largest magnitude."""
    y, ref = y.double().cpu(), ref.double().cpu()
    scale = ref.abs().max().item() + 1e-12
    err = (y - ref).abs().max().item()
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


# ---- resize_crop ----------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(RESIZE_CASES)), ids=[f"{c[1]}x{c[2]}-{c[3]}-{c[4]}" for c in RESIZE_CASES])
def test_resize_crop_vs_fp64(ops, i):
    """resize_crop against resize_crop_ref (float64: shorter side -> resize,
    round-half-even centre crop, bilinear with half-pixel centres, normalise).

    Tolerance per element: half an fp16 ulp at the reference value (the output's
    rounding) + RESIZE_MARGIN (4) x the distance of a CPU fp32 emulation from the
    float64 reference, measured as 1.46e-5 over the five small cases and 9.6e-5
    for 375x500 (recorded as 1.5e-5 / 1.0e-4 in RESIZE_CASES and asserted by
    test_elementwise_cpu.py): at most 9.8e-4 + 4.0e-4 = 1.4e-3, below a tenth
    of a grey level (1.7e-3), so an off-by-one-level or off-by-one-pixel result
    cannot pass.  The cases with an odd n - crop whose half is even ((30, 40),
    (40, 30), (375, 500)) fail with a crop offset rounded half up."""
    B, Hi, Wi, resize, crop, err32 = RESIZE_CASES[i]
    img = resize_case_image(i)
    ref = torch.from_numpy(resize_crop_ref(img, resize, crop))
    tol = half_ulp_f16(ref) + RESIZE_MARGIN * err32
    assert tol.max().item() < 0.1 * GREY
    assert ops.resize_crop_geometry(Hi, Wi, resize, crop) == center_crop_geometry(Hi, Wi, resize, crop)
    z = ops.resize_crop(torch.from_numpy(img).to(DEV), resize, crop)
    assert z.shape == (B, crop, crop, 4) and z.dtype == torch.float16 and z.is_contiguous()
    z = z.cpu()
    assert torch.count_nonzero(z[..., 3]).item() == 0
    err = (z[..., :3].double() - ref).abs()
    print(f"resize_crop {RESIZE_CASES[i][:5]}: max err {err.max().item():.3e}, max err / tol "
          f"{(err / tol).max().item():.3f}, max err beyond the fp16 rounding "
          f"{(err - half_ulp_f16(ref)).max().item():.3e} (slack {RESIZE_MARGIN * err32:.1e})")
    assert bool((err <= tol).all())


# ---- max pools ------------------------------------------------------------------------

POOL_CASES = [
    # (B, H, W, C, k, s, pad)
    (2, 7, 9, 8, 3, 2, 1),
    (1, 8, 5, 24, 3, 2, 1),
    (2, 6, 6, 64, 2, 2, 0),
    (1, 5, 7, 32, 3, 1, 1),
    (3, 13, 13, 96, 3, 2, 0),
    (1, 1, 1, 8, 1, 1, 0),
]
SPLIT_POOL_CASES = [c for c in POOL_CASES if c[3] % 32 == 0] + [(2, 7, 9, 32, 3, 2, 1)]


def _pool_input(case, offset=0.0):
    B, H, W, C = case[:4]
    g = torch.Generator().manual_seed(sum(case) + 31 * C)
    return torch.randn(B, H, W, C, generator=g) * 3 + offset


def _inf_border(x, k, pad):
    """The first k - pad rows and columns at -inf: the windows of the first output
    row and column hold nothing else, every other window also has finite values."""
    x = x.clone()
    x[:, :k - pad] = float("-inf")
    x[:, :, :k - pad] = float("-inf")
    return x


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "f32"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_maxpool_vs_fp64(ops, case, dtype):
    B, H, W, C, k, s, pad = case
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    # noise; all negative (a padding that counted as 0 would win); -inf borders
    inputs = [_pool_input(case), _pool_input(case, -20.0).clamp_max(-0.5)]
    if H > k - pad and W > k - pad:
        inputs.append(_inf_border(_pool_input(case), k, pad))
    for n, x in enumerate(inputs):
        x = x.to(dtype)
        ref = maxpool_ref(x, k, s, pad)
        y = ops.maxpool2d(x.to(DEV), k, s, pad)
        assert y.shape == (B, Ho, Wo, C) and y.dtype == dtype and y.is_contiguous()
        assert torch.equal(y.double().cpu(), ref), f"input {n}"
        if n == 1:
            assert ref.max().item() < 0
        if n == 2:
            assert torch.isinf(ref[:, 0]).all() and torch.isinf(ref[:, :, 0]).all() and torch.isfinite(ref[:, 1:, 1:]).all()
    # out= a batch slice of a larger tensor: rows outside the slice stay as they were
    x = inputs[0].to(dtype)
    big = torch.full((B + 2, Ho, Wo, C), 77.0, dtype=dtype, device=DEV)
    got = ops.maxpool2d(x.to(DEV), k, s, pad, out=big[1:B + 1])
    assert got.data_ptr() == big[1:].data_ptr()
    assert torch.equal(big[1:B + 1].double().cpu(), maxpool_ref(x, k, s, pad))
    assert bool((big[0] == 77.0).all()) and bool((big[B + 1] == 77.0).all())


@pytest.mark.parametrize("in_split", [False, True], ids=["f32-in", "split-in"])
@pytest.mark.parametrize("case", SPLIT_POOL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_maxpool_split_vs_fp64(ops, case, in_split):
    B, H, W, C, k, s, pad = case
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    for n, x in enumerate([_pool_input(case), _pool_input(case, -20.0).clamp_max(-0.5)]):
        xs = P.to_split(x)
        inp, vals = (xs, P.from_split(xs)) if in_split else (x, x)
        ref = maxpool_ref(vals, k, s, pad)
        y = ops.maxpool2d_split(inp.to(DEV), k, s, pad)
        assert y.shape == (B, Ho, Wo, 2 * C) and y.dtype == torch.float16 and y.is_contiguous()
        _check_rel(P.from_split(y.cpu()), ref, rel=1e-6)
        if n == 1:
            assert ref.max().item() < 0 and P.from_split(y.cpu()).max().item() < 0
    x = _pool_input(case)
    inp = P.to_split(x) if in_split else x
    big = torch.full((B + 2, Ho, Wo, 2 * C), 77.0, dtype=torch.float16, device=DEV)
    ops.maxpool2d_split(inp.to(DEV), k, s, pad, out=big[1:B + 1])
    assert torch.equal(big[1:B + 1], ops.maxpool2d_split(inp.to(DEV), k, s, pad))
    assert bool((big[0] == 77.0).all()) and bool((big[B + 1] == 77.0).all())


# ---- global average pool, fp16 --------------------------------------------------------

@pytest.mark.parametrize("B,H,W,C", [
    (4, 7, 7, 512),       # ResNet18: G = 4 pixel groups, LDS combine
    (2, 7, 7, 2048),      # ResNet50: one group, one chunk per thread
    (3, 5, 5, 8),         # one chunk, 256 groups for 25 pixels
    (2, 3, 3, 24),        # G = 85: 256 is no multiple of cv, idle threads
    (2, 7, 7, 1280),      # cv = 160 in (128, 256): one group, idle threads
    (1, 2, 2, 1536),      # cv = 192
    (2, 1, 1, 4096),      # cv = 512: two chunks per thread
    (50, 7, 7, 64),       # many images
])
def test_global_avgpool_fp16_vs_fp64(ops, B, H, W, C):
    """Against the float64 mean of the same fp16 values.  Tolerance: half an fp16
    ulp at the reference (the output's rounding) + HW * 2^-24 * max|x| (the fp32
    sum of HW terms).  The inputs' mean is 3, so a chunk that was never summed,
    or was overwritten by zeros, is off by ~3."""
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    x = (torch.randn(B, H, W, C, generator=g) + 3).half()
    ref = avgpool_ref(x)
    tol = half_ulp_f16(ref) + H * W * 2.0 ** -24 * x.abs().max().item()
    y = ops.global_avgpool(x.to(DEV))
    assert y.shape == (B, C) and y.dtype == torch.float16 and y.is_contiguous()
    err = (y.double().cpu() - ref).abs()
    print(f"avgpool {(B, H, W, C)}: max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), f"max err {err.max().item():.3e} at {err.argmax().item()}"


# ---- softmax_top1 ---------------------------------------------------------------------

ROWS = (1, 4, 5, 37)          # the launch puts 4 rows (waves) in a block


def _logits(rows, N, seed):
    """Multiples of 1/64 in about +-12: adding +-1e4 to them is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.randn(rows, N, generator=g) * 3 * 64) / 64


def _softmax_check(ops, logits_dev, ref_logits, **kw):
    cls, prob = ops.softmax_top1(logits_dev, **kw)
    rows = ref_logits.shape[0]
    assert cls.shape == (rows,) and cls.dtype == torch.int32 and prob.shape == (rows,) and prob.dtype == torch.float32
    i, v = softmax_top1_ref(ref_logits)
    assert torch.equal(cls.long().cpu(), i)
    assert torch.isfinite(prob).all()
    assert torch.allclose(prob.double().cpu(), v, rtol=1e-5, atol=1e-7)
    return cls, prob


@pytest.mark.parametrize("N", [1, 2, 65, 1000, 1024, 1025])
def test_softmax_top1_rows_widths_shifts(ops, N):
    for rows in ROWS:
        z = _logits(rows, N, 100 * N + rows)
        if N >= 65:                                    # ties: same lane (j, j + 64), different lanes
            z[0, 64] = z[0, 0] = 50.0
            z[rows - 1, N - 1] = z[rows - 1, 3] = 50.0
        cls, prob = _softmax_check(ops, z.to(DEV), z)
        if N >= 65:
            assert cls[0].item() == 0 and cls[rows - 1].item() == (0 if rows == 1 else 3)
        for shift in (1e4, -1e4):                      # no overflow, and the same probabilities
            zs = z + shift
            assert torch.equal((zs - shift), z)        # the shift is exact
            c2, p2 = _softmax_check(ops, zs.to(DEV), z)
            assert torch.equal(c2, cls) and torch.allclose(p2, prob, rtol=1e-5, atol=0)


@pytest.mark.parametrize("rows", ROWS)
def test_softmax_top1_strided_rows_and_neg_inf(ops, rows):
    z = _logits(rows, 1000, 7 + rows)
    buf = torch.full((rows, 1024), 1e9, device=DEV)    # a kernel that read past N would pick these
    buf[:, :1000] = z.to(DEV)
    view = buf[:, :1000]
    assert view.stride(0) == 1024 and (rows == 1 or not view.is_contiguous())
    _softmax_check(ops, view, z)
    for N in (65, 1000, 1025):
        z = _logits(rows, N, 11 * N + rows)
        z[:, ::3] = float("-inf")
        z[0] = float("-inf")
        z[0, N - 1] = 2.5                              # one finite entry: probability 1
        cls, prob = _softmax_check(ops, z.to(DEV), z)
        assert cls[0].item() == N - 1 and prob[0].item() == 1.0


@pytest.mark.parametrize("rows", ROWS)
def test_softmax_top1_packed_and_overflow_flag(ops, rows):
    z = _logits(rows, 1000, 50 + rows)
    sentinel = -123456
    packed = torch.full((rows + 3, 2), sentinel, dtype=torch.int32, device=DEV)
    cls, prob = _softmax_check(ops, z.to(DEV), z, packed=packed)
    assert torch.equal(packed[:rows, 0], cls) and torch.equal(packed[:rows, 1], prob.view(torch.int32))
    assert bool((packed[rows:] == sentinel).all())
    # flag 0: as without a flag; flag 1: every row marked, whatever the logits say
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    packed.fill_(sentinel)
    c0, p0 = _softmax_check(ops, z.to(DEV), z, packed=packed, ovf=flag)
    assert torch.equal(c0, cls) and torch.equal(p0, prob) and torch.equal(packed[:rows, 0], cls)
    flag.fill_(1)
    packed.fill_(sentinel)
    c1, p1 = ops.softmax_top1(z.to(DEV), packed=packed, ovf=flag)
    assert bool((c1 == ops.OVERFLOW_CLASS).all()) and ops.OVERFLOW_CLASS == -2 and bool((p1 == 0).all())
    assert bool((packed[:rows, 0] == -2).all()) and bool((packed[:rows, 1] == 0).all())
    assert bool((packed[rows:] == sentinel).all())
    assert flag.item() == 1


# ---- split conversions ----------------------------------------------------------------

@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("lead", [(1, 1), (3, 5, 7)], ids=["1x1", "3x5x7"])
def test_split_conversions_bit_equal(ops, lead, C):
    g = torch.Generator().manual_seed(C + len(lead))
    x = torch.randn(*lead, C, generator=g) * 5
    flat = x.view(-1)
    special = torch.tensor([0.0, -0.0, 1e-6, -1e-6, 3e-8, 6.1e-5, 65503.0, -65503.5, 65000.123, 1.0, -2.0 ** -14])
    idx = torch.randperm(flat.numel(), generator=g)[:special.numel()]
    flat[idx] = special
    want = P.to_split(x)
    assert torch.isfinite(want.float()).all()
    xs = ops.split_from_f32(x.to(DEV))
    assert xs.shape == (*lead, 2 * C) and xs.dtype == torch.float16 and xs.is_contiguous()
    assert torch.equal(xs.cpu().view(torch.int16), want.view(torch.int16))          # bits: -0.0 is not 0.0
    back = ops.f32_from_split(xs)
    assert back.shape == (*lead, C) and back.dtype == torch.float32
    assert torch.equal(back.cpu().view(torch.int32), P.from_split(want).view(torch.int32))
    # the round trip keeps 22 bits where the lo half is a normal fp16
    big = x.abs() >= 0.25
    assert ((back.cpu() - x).abs()[big] <= x.abs()[big] * 2.0 ** -21).all()
