"""The W4A8 MXFP4 decode GEMM (csrc/kernels/mx4dgemm.hip), its quantiser and packer, linear_mxfp4 and
the decoder's "mx4gemm" kernel family on an MI355X, against float64 products of the same quantised
operands; and the config knob that reaches the mode."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.config.loader import ConfigError, load_adapter_config
from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.ops import reference as ref
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _exact_operands(M, N, Kd, g):
    """Codes from all 16 e2m1 values, an independent scale 2^s, s in [-3, 3], per (row, 32-block); X
    from {0, +-0.5, +-1, +-2} in e4m3, sx a power of two.  Every product is a multiple of 2^-5 and
    |sum| <= 2432 * 96 < 2^18: every fp32 partial and the total's bf16 rounding are exact."""
    codes = torch.randint(0, 256, (N, Kd // 2), generator=g, dtype=torch.uint8).cuda()
    scales = torch.randint(124, 131, (N, Kd // 32), generator=g, dtype=torch.uint8).cuda()
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    x8 = vals[torch.randint(0, 7, (M, Kd), generator=g)].to(F8).cuda()
    sx = (2.0 ** torch.randint(-3, 3, (M, 1), generator=g)).cuda()
    want = (x8.float().double() @ K.dequant_mxfp4(codes, scales).double().t()) * sx.double()
    return codes, scales, x8, sx, want


# M: tile edges and clamped rows, every row-tile count the kernel is built for (16 / 32 / 64 / 128);
# N: less than one workgroup, no multiple of the widest bn, several workgroups; K: one block (one
# scale byte per lane: a scale on the wrong lane or a mispaired k fails it alone), three (split 2
# uneven, parts inside one quad), and 19 blocks: more than the ring's 16 and no multiple of it
@gpu
@pytest.mark.parametrize("M,N,Kd,split,bn", [
    (1, 64, 128, 1, 64), (5, 192, 384, 2, 128), (16, 192, 384, 3, 96), (17, 1024, 2432, 3, 112),
    (100, 1024, 2432, 2, 128), (128, 1024, 2432, 1, 64), (128, 64, 2432, 3, 128), (17, 192, 128, 1, 112),
    (40, 192, 2432, 3, 64), (64, 1024, 384, 2, 112), (128, 192, 2432, 2, 96), (1, 1024, 384, 3, 64),
    (5, 1024, 2432, 1, 128), (100, 64, 384, 1, 96)])
def test_exact_arithmetic(M, N, Kd, split, bn):
    codes, scales, x8, sx, want = _exact_operands(M, N, Kd, torch.Generator().manual_seed(M * 7 + N + Kd + split))
    pw = K.pack_mx4dgemm_weight(codes, scales, bn=bn)
    buf = torch.full((split, M, N + 8), -7.0, device="cuda")
    K.mx4dgemm(x8, sx, pw, "part", split, part=buf[:, :, 4:4 + N])
    assert torch.equal(buf[:, :, 4:4 + N].double().sum(0), want)
    assert bool((buf[:, :, :4] == -7.0).all()) and bool((buf[:, :, 4 + N:] == -7.0).all())
    out = torch.full((M, N + 8), -7.0, device="cuda", dtype=torch.bfloat16)
    K.mx4dgemm(x8, sx, pw, "bf16", out=out[:, 4:4 + N])
    assert torch.equal(out[:, 4:4 + N], want.to(torch.bfloat16))
    assert bool((out[:, :4] == -7.0).all()) and bool((out[:, 4 + N:] == -7.0).all())


@gpu
@pytest.mark.parametrize("M,N,Kd", [(128, 1024, 1024), (33, 256, 512)])
def test_random_data_within_summation_bound(M, N, Kd):
    """|y - ref| <= (2 K + 8) 2^-24 (|x8| @ |w|^T) sx: K 2^-24 bounds round-to-nearest summation in
    any order, doubled for the matrix unit's undocumented rounding of its 128-term sums, + 8 for the
    scale multiplies (test_f8dgemm_gpu.py's bound); the block scales are powers of two and add no
    rounding; the bf16 output adds its own, 2^-8 |ref|."""
    g = torch.Generator(device="cuda").manual_seed(M)
    x8, sx = K.quant_fp8_rows(torch.randn(M, Kd, device="cuda", generator=g).bfloat16())
    pw = K.pack_mx4dgemm_weight(*K.quant_mxfp4_weight((0.02 * torch.randn(N, Kd, device="cuda", generator=g)).bfloat16()))
    xd, wd = x8.float().double(), K.dequant_mxfp4(*pw.rowmajor()).double()
    want, bound = (xd @ wd.t()) * sx.double(), (2 * Kd + 8) * 2.0 ** -24 * (xd.abs() @ wd.abs().t()) * sx.double()
    part = K.mx4dgemm(x8, sx, pw, "part", K.mx4dgemm_config(M, N, Kd, pw.bn)[1])
    assert bool(((part.double().sum(0) - want).abs() <= bound).all())
    y = K.mx4dgemm(x8, sx, pw, "bf16")
    assert bool(((y.double() - want).abs() <= bound + 2.0 ** -8 * want.abs()).all())


@gpu
def test_quantiser_and_pack_round_trip():
    codes, scales, *_ = _exact_operands(1, 192, 384, torch.Generator().manual_seed(5))
    w = K.dequant_mxfp4(codes, scales)                          # on the MXFP4 grid
    assert torch.equal(K.dequant_mxfp4(*K.quant_mxfp4_weight(w)), w)
    c, s = K.quant_mxfp4_weight(torch.zeros(64, 128).bfloat16())
    assert int(c.max()) == 0 and s.unique().tolist() == [127]
    cpu = ref.pack_mx4dgemm_weight(codes.cpu(), scales.cpu(), 128)   # two workgroups, the second half padding;
    dev = K.pack_mx4dgemm_weight(codes, scales, bn=128)              # three blocks: a padded quad too
    assert torch.equal(dev.data.cpu(), cpu.reshape(-1))
    back = dev.rowmajor()
    assert torch.equal(back[0], codes) and torch.equal(back[1], scales)


@gpu
@pytest.mark.parametrize("M", [128, 129, 300])
def test_linear_mxfp4_across_the_slice_boundary(M):
    codes, scales, x8, sx, want = _exact_operands(M, 192, 384, torch.Generator().manual_seed(M))
    y = K.linear_mxfp4((x8, sx), K.pack_mx4dgemm_weight(codes, scales))
    assert torch.equal(y, want.to(torch.bfloat16))


@gpu
@pytest.mark.parametrize("B", [1, 5, 17])
def test_decoder_family_sits_inside_the_fp8_mode_s_noise(B, monkeypatch):
    """mx (to_mxfp4) against md, a bf16 model holding mx's dequantised weights, differs by the e4m3
    activation rounding only; ml (the to_fp8 library loop) against mb (bf16) carries that rounding
    plus the FP8 weight rounding: rel(mx, md) <= rel(ml, mb), both taken in this run.  B = 5 / 17
    prefill 200 / 680 rows, i.e. 128-row slices.  Measured on one MI355X, B = 1 / 5 / 17:
    rel(mx, md) = 2.27e-3 / 2.99e-3 / 2.88e-3, rel(ml, mb) = 3.11e-3 / 3.25e-3 / 3.30e-3."""
    def rel(a, b):
        return float((a.float() - b.float()).norm() / b.float().norm())

    cfg, T, i32 = get_config("tiny"), 40, dict(dtype=torch.int32, device="cuda")
    monkeypatch.delenv("CFC_DECODE_FP8_GEMM", raising=False)
    monkeypatch.delenv("CFC_PREFILL_FP8_GEMM", raising=False)
    mx = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_mxfp4())
    wd = DecoderWeights.random(cfg, "cuda", seed=3)
    for layer, packed in zip(wd.layers, mx.w.mx4_packed):
        for k, p in packed.items():
            layer[k] = K.dequant_mxfp4(*p.rowmajor())
    md, mb = DecoderModel(wd), DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3))
    ml = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    assert mx.decode_path(B) == "mx4gemm" and mx.decode_path(129) == "lib" and ml.decode_path(B) == "lib"
    # sequence b: T prompt tokens in cache blocks 2 b and 2 b + 1, then one decode step
    seq, tok = torch.arange(B, **i32)[:, None], torch.arange(T, **i32)[None]
    ids, bt = ((seq * 31 + tok * 7) % 500 + 3).reshape(-1), torch.cat([2 * seq, 2 * seq + 1], 1).contiguous()
    hidden = []
    for m in (mx, md, ml, mb):
        kv = PagedKVCache(cfg.layers, 64, m.w.kv_heads, cfg.head_dim, "cuda")
        m.forward_prefill(ids, tok.repeat(B, 1).reshape(-1), (64 * seq + tok).reshape(-1),
                          torch.arange(B + 1, **i32) * T, torch.full((B,), T, **i32), bt, kv)
        pos = torch.full((B,), T, **i32)
        hidden.append(m.forward_decode(ids[::T].contiguous(), pos, 64 * seq[:, 0] + T, pos + 1, bt, kv, part_blocks=4))
    d_mx, d_f8 = rel(hidden[0], hidden[1]), rel(hidden[2], hidden[3])
    print(f"B={B}: rel(mx4gemm, dequantised bf16)={d_mx:.3e} rel(fp8 lib, bf16)={d_f8:.3e}")
    assert d_mx <= d_f8


@gpu
def test_engine_generates_with_graph_capture():
    cfg = get_config("tiny")
    model = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_mxfp4())
    eng = LLMEngine(model, PagedKVCache(cfg.layers, 64, model.w.kv_heads, cfg.head_dim, "cuda"), prefix_cache=False)
    prompt = [1] + [(11 * i) % 500 + 3 for i in range(150)]
    res = eng.generate([prompt, prompt[:70]], 8, temperature=0.0, ignore_eos=True)
    assert model.decode_path(2) == "mx4gemm" and eng.last_used_graph and [len(t) for t in res.tokens] == [8, 8]


def test_config_schema_takes_mxfp4_and_still_refuses_unknown_values():
    env = {"LLM_BACKEND_TYPE": "hip", "LLM_WEIGHT_DTYPE": "mxfp4"}
    assert load_adapter_config("llm_backend", env=env).weight_dtype == "mxfp4"
    with pytest.raises(ConfigError, match="weight_dtype parameter is invalid"):
        load_adapter_config("llm_backend", env={**env, "LLM_WEIGHT_DTYPE": "int4"})
