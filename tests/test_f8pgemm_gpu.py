"""The W8A8 FP8 prefill GEMM (csrc/kernels/f8pgemm.hip), K.linear_fp8_packed and the decoder on one
packed FP8 weight copy (CFC_DECODE_FP8_GEMM=1 + CFC_PREFILL_FP8_GEMM=1) on an MI355X, against
float64 products of the same quantised operands."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _ref(x8, sx, w8, sw):
    """float64 (x8 @ w8^T) * sx * sw and (|x8| @ |w8|^T) * sx * sw of the quantised operands."""
    xd, wd, s = x8.float().double(), w8.float().double(), sx.double() * sw.double()
    return (xd @ wd.t()) * s, (xd.abs() @ wd.abs().t()) * s


def _random(M, N, Kd):
    g = torch.Generator(device="cuda").manual_seed(M)
    xb = torch.randn(M, Kd, device="cuda", generator=g).bfloat16()
    w8, sw = K.quant_fp8_weight((0.02 * torch.randn(N, Kd, device="cuda", generator=g)).bfloat16())
    return xb, K.quant_fp8_rows(xb), w8, sw


def _within_bound(y, x8, sx, w8, sw):
    """test_f8dgemm_gpu's bound: (2 K + 8) 2^-24 (|x8| @ |w8|^T) sx sw for the fp32 sums of this
    instruction and the two scale multiplies, + 2^-8 |ref| for the bf16 rounding."""
    want, mag = _ref(x8, sx, w8, sw)
    return bool(((y.double() - want).abs() <= (2 * x8.shape[1] + 8) * 2.0 ** -24 * mag + 2.0 ** -8 * want.abs()).all())


# M: clamped rows, exactly one tile, one row over, two and three M-tiles; N: less than a tile, a tile
# + a 64-column edge, several tiles; bn 96 / 112 at N = 320 and 1024: a 256-row tile straddles the
# packed bn-row groups; K: one, two, three K-tiles (the pipeline's prologue is two) and 19, odd
@pytest.mark.parametrize("M,N,Kd,bn", [
    (1, 64, 128, 64), (129, 320, 256, 96), (255, 320, 384, 112), (256, 1024, 2432, 96),
    (257, 1024, 128, 112), (300, 192, 2432, 128), (513, 1024, 256, 64), (300, 320, 384, 128),
    (513, 320, 2432, 112), (129, 1024, 384, 128), (257, 192, 256, 64), (1, 1024, 2432, 96),
    (256, 64, 128, 112)])
def test_exact_arithmetic(M, N, Kd, bn):
    """Entries from {0, +-0.5, +-1, +-2}, power-of-two scales: every product is a multiple of 0.25,
    every sum stays under 2^14, so each fp32 partial and the total's bf16 rounding are exact."""
    g = torch.Generator().manual_seed(M * 7 + N + Kd + bn)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    x8 = vals[torch.randint(0, 7, (M, Kd), generator=g)].to(F8).cuda()
    w8 = vals[torch.randint(0, 7, (N, Kd), generator=g)].to(F8).cuda()
    sx = (2.0 ** torch.randint(-3, 3, (M, 1), generator=g)).cuda()
    sw = (2.0 ** torch.randint(-3, 3, (1, N), generator=g)).cuda()
    want, _ = _ref(x8, sx, w8, sw)
    out = torch.full((M, N + 8), -7.0, device="cuda", dtype=torch.bfloat16)
    K.f8pgemm(x8, sx, K.pack_f8dgemm_weight(w8, sw, bn=bn), out=out[:, 4:4 + N])
    assert torch.equal(out[:, 4:4 + N], want.to(torch.bfloat16))
    assert bool((out[:, :4] == -7.0).all()) and bool((out[:, 4 + N:] == -7.0).all())


@pytest.mark.parametrize("M,N,Kd", [(300, 320, 512), (513, 1024, 1024)])
def test_random_data_within_summation_bound(M, N, Kd):
    _, (x8, sx), w8, sw = _random(M, N, Kd)
    assert _within_bound(K.f8pgemm(x8, sx, K.pack_f8dgemm_weight(w8, sw)), x8, sx, w8, sw)


@pytest.mark.parametrize("M", [128, 129])
def test_dispatcher_takes_both_kernels_and_both_inputs(M):
    """128 rows: the decode GEMM; 129: the prefill GEMM; bf16 x is quantised to the same (x8, scale)."""
    xb, (x8, sx), w8, sw = _random(M, 1024, 1024)
    pw = K.pack_f8dgemm_weight(w8, sw)
    for x in ((x8, sx), xb):
        y = K.linear_fp8_packed(x, pw)
        assert y.dtype == torch.bfloat16 and _within_bound(y, x8, sx, w8, sw)


@pytest.mark.parametrize("B,T", [(3, 100), (2, 70)])
def test_decoder_prefill_sits_inside_the_quantisation_noise(B, T, monkeypatch):
    """Prefill of B x T tokens, all rows: the packed path shares every rounding point with the
    library FP8 path and differs in fp32 summation order only: rel(new, lib) <= rel(lib, bf16) / 4.
    Measured on one MI355X, 3 x 100 / 2 x 70: rel(new, lib) = 4.5e-5 / 0, rel(lib, bf16) = 3.6e-3 /
    3.7e-3.  The model's weights hold one FP8 copy and refuse a model without both kernels."""
    def rel(a, b):
        return float((a.float() - b.float()).norm() / b.float().norm())

    cfg, i32 = get_config("tiny"), dict(dtype=torch.int32, device="cuda")
    for var in ("CFC_DECODE_FP8_GEMM", "CFC_PREFILL_FP8_GEMM"):
        monkeypatch.delenv(var, raising=False)
    mb = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3))
    ml = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    monkeypatch.setenv("CFC_DECODE_FP8_GEMM", "1")
    two_copies = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8()).w.nbytes()
    monkeypatch.setenv("CFC_PREFILL_FP8_GEMM", "1")
    mf = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    assert not any(mf.w.fp8_layers) and mf.w.nbytes() < two_copies
    # sequence b: T prompt tokens in cache blocks 4 b .. 4 b + 3
    seq, tok = torch.arange(B, **i32)[:, None], torch.arange(T, **i32)[None]
    ids, bt = ((seq * 31 + tok * 7) % 500 + 3).reshape(-1), (4 * seq + torch.arange(4, **i32)[None]).contiguous()
    hidden = []
    for m in (mb, ml, mf):
        kv = PagedKVCache(cfg.layers, 64, m.w.kv_heads, cfg.head_dim, "cuda")
        hidden.append(m.forward_prefill(ids, tok.repeat(B, 1).reshape(-1), (128 * seq + tok).reshape(-1),
                                        torch.arange(B + 1, **i32) * T, torch.full((B,), T, **i32), bt, kv))
    assert hidden[2].shape[0] == B * T
    d_lib, d_new = rel(hidden[1], hidden[0]), rel(hidden[2], hidden[1])
    print(f"B={B} T={T}: rel(new, lib)={d_new:.3e} rel(lib, bf16)={d_lib:.3e}")
    assert d_new <= d_lib / 4
    monkeypatch.delenv("CFC_DECODE_FP8_GEMM")
    monkeypatch.delenv("CFC_PREFILL_FP8_GEMM")
    with pytest.raises(ValueError):
        DecoderModel(mf.w)


def test_engine_generates_on_one_fp8_copy(monkeypatch):
    monkeypatch.setenv("CFC_DECODE_FP8_GEMM", "1")
    monkeypatch.setenv("CFC_PREFILL_FP8_GEMM", "1")
    cfg = get_config("tiny")
    model = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    eng = LLMEngine(model, PagedKVCache(cfg.layers, 64, model.w.kv_heads, cfg.head_dim, "cuda"), prefix_cache=False)
    prompt = [1] + [(11 * i) % 500 + 3 for i in range(299)]
    res = eng.generate([prompt, prompt[:70]], 8, temperature=0.0, ignore_eos=True)
    assert model.decode_path(2) == "f8gemm" and eng.last_used_graph and [len(t) for t in res.tokens] == [8, 8]
