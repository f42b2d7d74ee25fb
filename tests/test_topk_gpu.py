"""ops.softmax_topk against a stable descending sort and the fp64 softmax, at the
shapes of tests/test_elementwise_gpu.py's softmax_top1 cases: rows around the
four-rows-per-block boundary, widths around the 64-lane and 1024-column
(register path / memory path) boundaries.  torch.topk is not the oracle: it
does not promise the stable tie order the kernel promises."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 4, 5, 37)          # the launch puts 4 rows (waves) in a block
WIDTHS = (1, 2, 65, 1000, 1024, 1025)
NEG = float("-inf")


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _logits(rows, N, seed):
    """Multiples of 1/64 in about +-12: adding +-1e4 to them is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.randn(rows, N, generator=g) * 3 * 64) / 64


def _ks(N):
    return sorted({k for k in (1, 2, 5, min(N, 16)) if k <= N})


def topk_ref(z, k):
    """(indices int64 [rows, k], fp64 probabilities) of a stable descending sort (CPU)."""
    z = z.double().cpu()
    idx = torch.sort(z, dim=1, descending=True, stable=True).indices[:, :k]
    return idx, torch.softmax(z, 1).gather(1, idx)


def _check(ops, z_dev, z_ref, k, **kw):
    cls, prob = ops.softmax_topk(z_dev, k, **kw)
    rows = z_ref.shape[0]
    assert cls.shape == (rows, k) and cls.dtype == torch.int32 and cls.is_contiguous()
    assert prob.shape == (rows, k) and prob.dtype == torch.float32 and prob.is_contiguous()
    i, v = topk_ref(z_ref, k)
    assert torch.equal(cls.long().cpu(), i), (k, cls.cpu(), i)
    assert torch.isfinite(prob).all()
    assert torch.allclose(prob.double().cpu(), v, rtol=1e-5, atol=1e-7), (prob.double().cpu() - v).abs().max()
    # column 0 is softmax_top1: class and probability bits
    c1, p1 = ops.softmax_top1(z_dev, **kw)
    assert torch.equal(cls[:, 0], c1) and torch.equal(prob[:, 0].view(torch.int32), p1.view(torch.int32))
    return cls, prob


def test_stable_sort_reference_on_the_known_tie_case():
    z = torch.tensor([[1.0, 5.0, 5.0, 2.0, 5.0, NEG, 2.0]])
    assert topk_ref(z, 5)[0].tolist() == [[1, 2, 4, 3, 6]]
    assert topk_ref(z, 7)[0].tolist() == [[1, 2, 4, 3, 6, 0, 5]]


@pytest.mark.parametrize("N", WIDTHS)
def test_topk_rows_widths_k_shifts(ops, N):
    for rows in ROWS:
        z = _logits(rows, N, 100 * N + rows)
        if N >= 65:                                    # ties: same lane (j, j + 64), different lanes
            z[0, 64] = z[0, 0] = 50.0
            z[rows - 1, N - 1] = z[rows - 1, 3] = 50.0
        zd = z.to(DEV)
        for k in _ks(N):
            cls, prob = _check(ops, zd, z, k)
            if N >= 65 and k >= 2 and rows > 1:
                assert cls[0, :2].tolist() == [0, 64] and cls[rows - 1, :2].tolist() == [3, N - 1]
            for shift in (1e4, -1e4):                  # no overflow, the same classes and probabilities
                zs = z + shift
                assert torch.equal((zs - shift), z)    # the shift is exact
                c2, p2 = _check(ops, zs.to(DEV), z, k)
                assert torch.equal(c2, cls) and torch.allclose(p2, prob, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("N", (7, 130, 1000, 1025))
def test_topk_ties_in_lane_across_lanes_and_at_the_k_boundary(ops, N):
    rows = 5
    z = _logits(rows, N, 31 * N)
    z[0] = torch.tensor([1.0, 5.0, 5.0, 2.0, 5.0, NEG, 2.0]).repeat(N // 7 + 1)[:N] if N > 7 else \
        torch.tensor([1.0, 5.0, 5.0, 2.0, 5.0, NEG, 2.0])
    z[1] = 0.25                                        # every entry equal: classes 0 .. k-1, probability 1/N
    if N >= 65:
        z[2, 3] = z[2, 3 + 64] = z[2, 40] = 50.0       # same lane (3, 67) and another lane (40)
        z[3, N - 1] = z[3, N - 2] = z[3, 0] = 50.0
        z[4, 1::2] = 50.0                              # half the row ties: the boundary falls inside the tie
    zd = z.to(DEV)
    for k in sorted({1, 2, 3, 5, min(N, 16)}):
        cls, prob = _check(ops, zd, z, k)
        assert cls[1].tolist() == list(range(k))
        if N == 7:
            assert cls[0].tolist() == [1, 2, 4, 3, 6, 0, 5][:k]
        if N >= 65:
            assert cls[2, :3].tolist() == [3, 40, 67][:k] and cls[3, :3].tolist() == [0, N - 2, N - 1][:k]
            assert cls[4].tolist() == list(range(1, 2 * k, 2))


@pytest.mark.parametrize("N", (7, 65, 1000, 1025))
def test_topk_fewer_finite_entries_than_k(ops, N):
    rows = 6
    z = _logits(rows, N, 17 * N)
    z[:, ::3] = NEG
    z[0] = NEG
    z[0, N - 1] = 2.5                                  # one finite entry: probability 1, then -inf in index order
    z[1] = NEG
    z[1, 5], z[1, 2] = 1.0, 3.0
    z[2] = NEG
    z[2, 0] = -4.0
    zd = z.to(DEV)
    for k in sorted({1, 2, 5, min(N, 16)}):
        cls, prob = _check(ops, zd, z, k)
        assert cls[0].tolist() == ([N - 1] + list(range(N - 1)))[:k] and prob[0, 0].item() == 1.0
        assert bool((prob[0, 1:] == 0).all())
        assert cls[1].tolist() == ([2, 5] + [i for i in range(N) if i not in (2, 5)])[:k]
        assert bool((prob[1, 2:] == 0).all())
        assert cls[2].tolist() == list(range(k))
        for r in range(rows):                          # distinct classes in every row
            assert len(set(cls[r].tolist())) == k


@pytest.mark.parametrize("rows", ROWS)
def test_topk_strided_rows_read_nothing_past_n(ops, rows):
    for N, ld in ((1000, 1024), (65, 128), (1025, 1100)):
        z = _logits(rows, N, 7 * N + rows)
        buf = torch.full((rows, ld), 1e9, device=DEV)  # a kernel that read past N would pick these
        buf[:, :N] = z.to(DEV)
        view = buf[:, :N]
        assert view.stride(0) == ld and (rows == 1 or not view.is_contiguous())
        for k in (1, 5, 16):
            _check(ops, view, z, k)


@pytest.mark.parametrize("rows", ROWS)
def test_topk_overflow_flag(ops, rows):
    z = _logits(rows, 1000, 50 + rows)
    zd = z.to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in (1, 5, 16):
        cls, prob = _check(ops, zd, z, k)
        flag.zero_()
        c0, p0 = _check(ops, zd, z, k, ovf=flag)       # flag 0: as without a flag
        assert torch.equal(c0, cls) and torch.equal(p0, prob)
        flag.fill_(1)                                  # flag 1: every entry marked, whatever the logits say
        c1, p1 = ops.softmax_topk(zd, k, ovf=flag)
        assert c1.shape == (rows, k) and bool((c1 == ops.OVERFLOW_CLASS).all()) and bool((p1 == 0).all())
        assert flag.item() == 1


def test_topk_refusals(ops):
    z = _logits(4, 40, 1).to(DEV)
    for k in (0, -1, 17, 41):
        with pytest.raises(RuntimeError, match="k must be"):
            ops.softmax_topk(z, k)
    with pytest.raises(RuntimeError, match="k must be"):
        ops.softmax_topk(z[:, :3], 5)                  # k > N
    with pytest.raises(RuntimeError, match="dtype"):
        ops.softmax_topk(z.half(), 5)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.softmax_topk(z.double(), 5)
    with pytest.raises(RuntimeError, match="unit column stride"):
        ops.softmax_topk(z.t(), 2)
    with pytest.raises(RuntimeError, match="unit column stride"):
        ops.softmax_topk(z[:, ::2], 2)
    with pytest.raises(RuntimeError, match="rank"):
        ops.softmax_topk(z[0], 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.softmax_topk(z.cpu(), 5)
    with pytest.raises(RuntimeError, match="ovf"):
        ops.softmax_topk(z, 5, ovf=torch.zeros(1, dtype=torch.int32))
    cls, prob = ops.softmax_topk(z[:0], 5)             # no rows: empty results, no launch
    assert cls.shape == (0, 5) and prob.shape == (0, 5)
    torch.cuda.synchronize()
