"""Semantics of the int8 row quantiser's oracle (ops.reference.quant_i8_rows), which the HIP
quantiser (knn8.hip) is held to bit for bit in test_knn8_gpu.py."""
import pytest
import torch

from copilot_for_consensus_amd.ops import reference as R


def _int_rows(n=32, dim=128):
    x = torch.randint(-127, 128, (n, dim), generator=torch.Generator().manual_seed(0))
    x[:, 0] = 127                                     # amax 127: 127 / amax == 1
    return x


@pytest.mark.parametrize("shrink", [1.0, 2.0 ** -9])
def test_integer_rows_come_back_as_themselves(shrink):
    x = _int_rows()
    codes, scale, norm2 = R.quant_i8_rows((x.float() * shrink).bfloat16())     # <= 127: exact in bf16
    assert torch.equal(codes, x.to(torch.int8))
    assert torch.equal(scale, torch.full((32,), shrink))
    assert torch.equal(norm2, x.pow(2).sum(1).float() * shrink * shrink)


def test_ties_go_to_even_and_a_zero_row_has_scale_zero():
    x = torch.zeros(2, 128)
    x[0, :4] = torch.tensor([127.0, 0.5, 1.5, 2.5])
    codes, scale, norm2 = R.quant_i8_rows(x.bfloat16())
    assert codes[0, :4].tolist() == [127, 0, 2, 2]
    assert not codes[1].any() and scale[1] == 0 and norm2[1] == 0


def test_decode_bound_and_unit_norm():
    x = torch.randn(64, 384, generator=torch.Generator().manual_seed(1)).bfloat16()
    amax = x.float().abs().amax(1, keepdim=True)
    codes, scale, _ = R.quant_i8_rows(x)
    err = (codes.float() * scale[:, None] - x.float()).abs()
    # half a step plus four fp32 roundings
    assert bool((err <= 0.5 * scale[:, None] + 4 * 2.0 ** -24 * amax).all())
    cn, sn, n2 = R.quant_i8_rows(x, normalize=True)
    assert torch.equal(cn, codes) and torch.equal(n2, torch.ones(64))
    assert torch.allclose((cn.double() * sn.double()[:, None]).norm(dim=1), torch.ones(64, dtype=torch.double), atol=1e-6)
