"""Host-side model of the fused layer-1 block kernel's schedule and addressing
(csrc/kernels/conv3x3_split_block.hip): which ring rows each step reads and writes,
the producer's swizzled y-ring store against the consumer's fragment read, and the
halo rows a band computes.  The model restates the kernel's rules; the GPU tests
(test_c64_block_gpu.py) check the kernel itself.
"""
import pytest

import c64_block_cases as BC
import exact_ref as X

RING = 5
RC = 60


def slot(chunk, col):
    return chunk ^ ((2 * col) & 15)


def steps(y0, y1, H):
    """Per step s of the band [y0, y1): (x rows read, x row whose DMA is issued or None,
    y rows read, y rows written) as the kernel schedules them."""
    ylast = min(H - 1, y1)
    out = []
    for s in range(y0 - 1, y1 + 2):
        x_read, y_read, y_write = set(), set(), set()
        dma = s + 3 if s + 3 <= ylast + 1 else None
        if s <= y1:                                     # producer
            if 0 <= s < H:
                first = s >= y0 and (s - y0) % 2 == 0
                pair = first and s + 1 <= ylast
                x_read |= {s - 1, s, s + 1}
                y_write.add(s)
                if pair:
                    x_read.add(s + 2)
                    y_write.add(s + 1)
            else:
                y_write.add(s)                          # a zero row
        c = s - 2                                       # consumer
        if c >= y0:
            assert c < y1
            y_read |= {c - 1, c, c + 1}
            if (c - y0) % 2 == 1:
                y_read.add(c - 2)
        out.append((s, x_read, dma, y_read, y_write))
    return out


BANDS = [(0, 56, 56), (0, 1, 1), (0, 2, 2), (3, 10, 13), (5, 13, 13), (0, 7, 13), (12, 13, 13), (1, 2, 9), (0, 55, 56),
         (31, 56, 56), (0, 4, 56), (7, 8, 9)]


@pytest.mark.parametrize("y0,y1,H", BANDS)
def test_rings_over_a_band(y0, y1, H):
    """Every row a step reads is resident (DMA'd at least one step earlier, or produced
    by an earlier step) and no slot a step reads is written in that step."""
    landed = {y0 - 2, y0 - 1, y0, y0 + 1}               # the band's prologue
    in_flight = None
    produced = {}                                       # y row -> step that completed it
    xslot, yslot = {}, {}
    for r in landed:
        xslot[r % RING] = r
    for s, x_read, dma, y_read, y_write in steps(y0, y1, H):
        if in_flight is not None:                       # the barrier publishes last step's DMA
            landed.add(in_flight)
            xslot[in_flight % RING] = in_flight
        for r in x_read:
            assert r in landed and xslot[r % RING] == r, (s, r)
        if dma is not None:
            assert all(dma % RING != r % RING for r in x_read), (s, dma, x_read)
        in_flight = dma
        for r in y_read:
            assert yslot.get(r % RING) == r and produced[r] < s, (s, r)
        for r in y_write:
            assert all(r % RING != q % RING for q in y_read), (s, r, y_read)
            yslot[r % RING] = r
        if s <= y1:
            produced[s] = s                             # row s is complete when step s ends
    assert sorted(r for r in produced) == list(range(y0 - 1, y1 + 1))


@pytest.mark.parametrize("y0,y1,H", BANDS)
def test_halo_rows(y0, y1, H):
    """The producer computes y rows max(0, y0-1) .. min(H-1, y1), writes zeros for row -1
    or H, and every y row's tail columns are written exactly once, no later than the row."""
    computed, zero, tail_at = [], [], {}
    ylast = min(H - 1, y1)
    for s in range(y0 - 1, y1 + 1):
        if not 0 <= s < H:
            zero.append(s)
            continue
        computed.append(s)
        first = s >= y0 and (s - y0) % 2 == 0
        if first or s < y0:
            for r in ([s, s + 1] if first and s + 1 <= ylast else [s]):
                assert r not in tail_at
                tail_at[r] = s
    assert computed == list(range(max(0, y0 - 1), min(H - 1, y1) + 1))
    assert zero == [r for r in (y0 - 1, y1) if not 0 <= r < H]
    assert sorted(tail_at) == computed and all(at <= r for r, at in tail_at.items())


def test_store_address_matches_fragment_read():
    """The producer lane (wave cw, lane group q) holds global chunk
    split_off_q(16 cw, q) / 8 of its pixel and stores it at col * 256 + slot(chunk, col) * 16;
    the consumer reads chunk 4 (2 cb + p) + q' of LDS column col at
    col_off(col) ^ ((2 cb + p) << 6).  Exhaustive over (col, chunk)."""
    def split_off(c):
        return ((c >> 5) << 6) + (c & 31)

    def split_off_q(nb, q):
        return split_off(nb + 8 * (q >> 1)) + 32 * (q & 1)

    def col_off(col, q):
        x = (2 * col) & 15
        return col * 256 + (((x >> 2) & 3) << 6) + (((q ^ x) & 3) << 4)

    stored = {}
    for col in range(1, 57):
        for cw in range(4):
            for q in range(4):
                chunk = split_off_q(16 * cw, q) >> 3
                # the chunk's place in the global pixel: block, hi/lo plane, 8-channel group
                assert chunk == 8 * (cw >> 1) + 4 * (q & 1) + 2 * (cw & 1) + (q >> 1)
                stored[(col, chunk)] = col * 256 + (slot(chunk, col) << 4)
        assert sorted(c for (cc, c) in stored if cc == col) == list(range(16))
    for col in range(1, 57):
        for cb in range(2):
            for p in range(2):
                for q in range(4):
                    read = col_off(col, q) ^ ((2 * cb + p) << 6)
                    assert read == stored[(col, 4 * (2 * cb + p) + q)], (col, cb, p, q)
    assert max(stored.values()) + 16 <= RC * 256


@pytest.mark.parametrize("B,H,W", BC.SHAPES)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_exact_cases_qualify(kind, B, H, W):
    """The composed exact cases of test_c64_block_gpu.py pass exact_ref's headroom and
    integrality assertions for both convs (any f32 accumulation order is exact), the planes
    that must be live are, and the expected output exercises the lo plane."""
    case_a, case_b, xs, expect, ref = BC.block_case(kind, B, H, W)
    _, _, ha = X.exact_split_conv(case_a, True, False)
    _, _, hb = X.exact_split_conv(case_b, True, True)
    assert ha < 1 and hb < 1
    xh, xl = X.split_planes(xs)
    assert bool(((xl.double().abs() > xh.double().abs() / 1024) & (xh != 0)).any()), "x is a canonical pair"
    assert (X.split_planes(expect)[1] != 0).double().mean().item() > 0.2
    assert (ref > 0).double().mean().item() > 0.2
