"""The W4A8 MXFP4 prefill GEMM (csrc/kernels/mx4pgemm.hip), linear_mxfp4(tiled=True) and the decoder's
CFC_PREFILL_MX4_GEMM switch on an MI355X, against float64 products of the same quantised operands."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _exact_operands(M, N, Kd, g, device="cuda"):
    """test_mx4dgemm_gpu.py's: all 16 e2m1 codes, an independent scale 2^s, s in [-3, 3], per (row,
    32-block); X from {0, +-0.5, +-1, +-2}, sx a power of two.  Every product is a multiple of 2^-5
    and |sum| <= 2432 * 96 < 2^18: every fp32 partial and the total's bf16 rounding are exact."""
    codes = torch.randint(0, 256, (N, Kd // 2), generator=g, dtype=torch.uint8).to(device)
    scales = torch.randint(124, 131, (N, Kd // 32), generator=g, dtype=torch.uint8).to(device)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    x8 = vals[torch.randint(0, 7, (M, Kd), generator=g)].to(F8).to(device)
    sx = (2.0 ** torch.randint(-3, 3, (M, 1), generator=g)).to(device)
    want = (x8.float().double() @ K.dequant_mxfp4(codes, scales).double().t()) * sx.double()
    return codes, scales, x8, sx, want


# M: clamped rows, and one, two and three M-tiles with their edges; N: less than a wave column, a tile
# plus a 64-column edge, four tiles, bn 96 / 112 so that a 256-column tile straddles packed groups;
# K: one block (a scale on the wrong lane or a mispaired k fails it alone), three (tail only), one
# quad, a quad plus one, 19 blocks (four quads and a tail of three, longer than the X ring)
@gpu
@pytest.mark.parametrize("M,N,Kd,bn", [
    (1, 64, 128, 64), (129, 192, 384, 96), (255, 320, 512, 112), (256, 1024, 640, 128), (257, 320, 2432, 96),
    (300, 1024, 2432, 112), (513, 192, 128, 64), (513, 1024, 640, 96), (300, 64, 2432, 128), (129, 1024, 384, 112),
    (256, 320, 128, 112), (513, 320, 512, 64)])
def test_exact_arithmetic(M, N, Kd, bn):
    codes, scales, x8, sx, want = _exact_operands(M, N, Kd, torch.Generator().manual_seed(M * 7 + N + Kd + bn))
    out = torch.full((M, N + 8), -7.0, device="cuda", dtype=torch.bfloat16)
    K.mx4pgemm(x8, sx, K.pack_mx4dgemm_weight(codes, scales, bn=bn), out=out[:, 4:4 + N])
    assert torch.equal(out[:, 4:4 + N], want.to(torch.bfloat16))
    assert bool((out[:, :4] == -7.0).all()) and bool((out[:, 4 + N:] == -7.0).all())


@gpu
@pytest.mark.parametrize("M,N,Kd", [(300, 320, 512), (513, 1024, 1024)])
def test_random_data_within_summation_bound(M, N, Kd):
    """|y - ref| <= (2 K + 8) 2^-24 (|x8| @ |w|^T) sx + 2^-8 |ref|: test_mx4dgemm_gpu.py's bound."""
    g = torch.Generator(device="cuda").manual_seed(M)
    x8, sx = K.quant_fp8_rows(torch.randn(M, Kd, device="cuda", generator=g).bfloat16())
    pw = K.pack_mx4dgemm_weight(*K.quant_mxfp4_weight((0.02 * torch.randn(N, Kd, device="cuda", generator=g)).bfloat16()))
    xd, wd = x8.float().double(), K.dequant_mxfp4(*pw.rowmajor()).double()
    want, bound = (xd @ wd.t()) * sx.double(), (2 * Kd + 8) * 2.0 ** -24 * (xd.abs() @ wd.abs().t()) * sx.double()
    assert bool(((K.mx4pgemm(x8, sx, pw).double() - want).abs() <= bound + 2.0 ** -8 * want.abs()).all())


@pytest.mark.parametrize("M,device", [pytest.param(128, "cuda", marks=gpu), pytest.param(129, "cuda", marks=gpu),
                                      pytest.param(300, "cuda", marks=gpu), (129, "cpu")])
def test_linear_mxfp4_tiled(M, device):
    """Exact operands make the prefill kernel and the slice loop bit-equal; cpu: the float64 branch."""
    codes, scales, x8, sx, want = _exact_operands(M, 192, 384, torch.Generator().manual_seed(M), device)
    pw = K.pack_mx4dgemm_weight(codes, scales)
    y = K.linear_mxfp4((x8, sx), pw, tiled=True)
    assert torch.equal(y, want.to(torch.bfloat16))
    assert torch.equal(y, K.linear_mxfp4((x8, sx), pw, tiled=False))


@gpu
@pytest.mark.parametrize("B,T", [(3, 100), (2, 70)])
def test_decoder_prefill_sits_inside_the_quantisation_noise(B, T, monkeypatch):
    """Prefill of B x T tokens, all rows, on the same to_mxfp4() weights: the prefill kernel shares
    every rounding point with the slice loop and differs in fp32 summation order only:
    rel(tiled, slices) <= rel(slices, dequantised-bf16 model) / 4.  Measured on one MI355X, 3 x 100 /
    2 x 70: rel(tiled, slices) = 3.2e-7 / 4.6e-7, rel(slices, dequantised bf16) = 2.9e-3 / 3.0e-3."""
    def rel(a, b):
        return float((a.float() - b.float()).norm() / b.float().norm())

    cfg, i32 = get_config("tiny"), dict(dtype=torch.int32, device="cuda")
    monkeypatch.delenv("CFC_PREFILL_MX4_GEMM", raising=False)
    ms = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_mxfp4())
    wd = DecoderWeights.random(cfg, "cuda", seed=3)
    for layer, packed in zip(wd.layers, ms.w.mx4_packed):
        for k, p in packed.items():
            layer[k] = K.dequant_mxfp4(*p.rowmajor())
    md = DecoderModel(wd)
    monkeypatch.setenv("CFC_PREFILL_MX4_GEMM", "1")
    mt = DecoderModel(ms.w)
    assert mt.prefill_mx4gemm and not ms.prefill_mx4gemm and not md.prefill_mx4gemm
    # sequence b: T prompt tokens in cache blocks 4 b .. 4 b + 3
    seq, tok = torch.arange(B, **i32)[:, None], torch.arange(T, **i32)[None]
    ids, bt = ((seq * 31 + tok * 7) % 500 + 3).reshape(-1), (4 * seq + torch.arange(4, **i32)[None]).contiguous()
    hidden = []
    for m in (md, ms, mt):
        kv = PagedKVCache(cfg.layers, 64, m.w.kv_heads, cfg.head_dim, "cuda")
        hidden.append(m.forward_prefill(ids, tok.repeat(B, 1).reshape(-1), (128 * seq + tok).reshape(-1),
                                        torch.arange(B + 1, **i32) * T, torch.full((B,), T, **i32), bt, kv))
    assert hidden[2].shape[0] == B * T
    d_q, d_new = rel(hidden[1], hidden[0]), rel(hidden[2], hidden[1])
    print(f"B={B} T={T}: rel(tiled, slices)={d_new:.3e} rel(slices, dequantised bf16)={d_q:.3e}")
    assert d_new <= d_q / 4
    monkeypatch.setenv("CFC_PREFILL_MX4_GEMM", "2")
    with pytest.raises(ValueError):
        DecoderModel(ms.w)


@gpu
def test_engine_generates_with_the_prefill_kernel(monkeypatch):
    monkeypatch.setenv("CFC_PREFILL_MX4_GEMM", "1")
    cfg = get_config("tiny")
    model = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_mxfp4())
    eng = LLMEngine(model, PagedKVCache(cfg.layers, 64, model.w.kv_heads, cfg.head_dim, "cuda"), prefix_cache=False)
    prompt = [1] + [(11 * i) % 500 + 3 for i in range(299)]
    res = eng.generate([prompt, prompt[:70]], 8, temperature=0.0, ignore_eos=True)
    assert model.prefill_mx4gemm and model.decode_path(2) == "mx4gemm" and eng.last_used_graph
    assert [len(t) for t in res.tokens] == [8, 8]
