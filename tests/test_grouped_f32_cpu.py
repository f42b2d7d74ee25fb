"""pack_grouped_f32_weight: pack_grouped_weight's block-local rows, kept in fp32."""
import pytest
import torch

from idunno.models import packed as P


@pytest.mark.parametrize("c,groups", [(64, 16), (64, 8), (64, 4), (128, 4), (128, 2)])     # Cg 4, 8, 16, 32, 64
def test_f32_rows_are_the_f16_rows_unrounded(c, groups):
    cg = c // groups
    torch.manual_seed(c + groups)
    w = (torch.randn(c, cg, 3, 3) / (9 * cg) ** 0.5).half().float()                        # half-representable
    rows = P.pack_grouped_f32_weight(w, groups)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (c, 9 * max(16, cg)) and rows.is_contiguous()
    assert torch.equal(rows.half(), P.pack_grouped_weight(w, groups))
    assert torch.equal(rows, P.pack_grouped_weight(w, groups).float())                      # nothing lost either way


@pytest.mark.parametrize("shape,groups,msg", [((48, 12, 3, 3), 4, r"\b12\b.*channels per group"),
                                              ((64, 4, 1, 1), 16, r"must be \[Cout, Cin/groups, 3, 3\]"),
                                              ((64, 4, 3, 3), 8, r"do not describe a conv with Cin = Cout")])
def test_f32_packing_refuses_what_the_f16_packing_refuses(shape, groups, msg):
    for pack in (P.pack_grouped_f32_weight, P.pack_grouped_weight):
        with pytest.raises(ValueError, match=msg):
            pack(torch.zeros(shape), groups)
