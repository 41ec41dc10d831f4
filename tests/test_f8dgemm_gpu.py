"""The W8A8 FP8 decode GEMM (csrc/kernels/f8dgemm.hip), its fused split-K reduce and the decoder's
"f8gemm" kernel family on an MI355X, against float64 products of the same quantised operands."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.ops import reference as ref
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _ref(x8, sx, w8, sw):
    """float64 (x8 @ w8^T) * sx * sw and (|x8| @ |w8|^T) * sx * sw of the quantised operands."""
    xd, wd, s = x8.float().double(), w8.float().double(), sx.double() * sw.double()
    return (xd @ wd.t()) * s, (xd.abs() @ wd.abs().t()) * s


# M: tile edges and clamped rows, every row-tile count the kernel is built for (16 / 32 / 64 / 128);
# N: less than one workgroup, no multiple of the widest bn, several workgroups; K: one block, three
# (split 2 uneven), and 19 blocks: more than twice the ring's depth (8; 6 at bn 128) and no multiple
@pytest.mark.parametrize("M,N,Kd,split,bn", [
    (1, 64, 128, 1, 64), (5, 192, 384, 2, 128), (16, 192, 384, 3, 96), (17, 1024, 2432, 3, 112),
    (100, 1024, 2432, 2, 128), (128, 1024, 2432, 1, 64), (128, 64, 2432, 3, 128), (17, 192, 128, 1, 112),
    (40, 192, 2432, 3, 64), (64, 1024, 384, 2, 112), (128, 192, 2432, 2, 96), (1, 1024, 384, 3, 64),
    (5, 1024, 2432, 1, 128), (100, 64, 384, 1, 96)])
def test_exact_arithmetic(M, N, Kd, split, bn):
    """Entries from {0, +-0.5, +-1, +-2}, power-of-two scales: every product is a multiple of 0.25,
    every sum stays under 2^14, so each fp32 partial and the total's bf16 rounding are exact."""
    g = torch.Generator().manual_seed(M * 7 + N + Kd + split)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    x8 = vals[torch.randint(0, 7, (M, Kd), generator=g)].to(F8).cuda()
    w8 = vals[torch.randint(0, 7, (N, Kd), generator=g)].to(F8).cuda()
    sx = (2.0 ** torch.randint(-3, 3, (M, 1), generator=g)).cuda()
    sw = (2.0 ** torch.randint(-3, 3, (1, N), generator=g)).cuda()
    want, _ = _ref(x8, sx, w8, sw)
    pw = K.pack_f8dgemm_weight(w8, sw, bn=bn)
    buf = torch.full((split, M, N + 8), -7.0, device="cuda")
    K.f8dgemm(x8, sx, pw, "part", split, part=buf[:, :, 4:4 + N])
    assert torch.equal(buf[:, :, 4:4 + N].double().sum(0), want)
    assert bool((buf[:, :, :4] == -7.0).all()) and bool((buf[:, :, 4 + N:] == -7.0).all())
    out = torch.full((M, N + 8), -7.0, device="cuda", dtype=torch.bfloat16)
    K.f8dgemm(x8, sx, pw, "bf16", out=out[:, 4:4 + N])
    assert torch.equal(out[:, 4:4 + N], want.to(torch.bfloat16))
    assert bool((out[:, :4] == -7.0).all()) and bool((out[:, 4 + N:] == -7.0).all())


@pytest.mark.parametrize("M,N,Kd", [(128, 1024, 1024), (33, 256, 512)])
def test_random_data_within_summation_bound(M, N, Kd):
    """|y - ref| <= (2 K + 8) 2^-24 (|x8| @ |w8|^T) sx sw: K 2^-24 bounds round-to-nearest summation
    in any order, doubled for the matrix unit's undocumented rounding of its 128-term sums, + 8 for
    the two scale multiplies; the bf16 output adds its own rounding, 2^-8 |ref|."""
    g = torch.Generator(device="cuda").manual_seed(M)
    x8, sx = K.quant_fp8_rows(torch.randn(M, Kd, device="cuda", generator=g).bfloat16())
    w8, sw = K.quant_fp8_weight((0.02 * torch.randn(N, Kd, device="cuda", generator=g)).bfloat16())
    want, mag = _ref(x8, sx, w8, sw)
    bound = (2 * Kd + 8) * 2.0 ** -24 * mag
    pw = K.pack_f8dgemm_weight(w8, sw)
    part = K.f8dgemm(x8, sx, pw, "part", K.f8dgemm_config(M, N, Kd, pw.bn)[1])
    assert bool(((part.double().sum(0) - want).abs() <= bound).all())
    y = K.f8dgemm(x8, sx, pw, "bf16")
    assert bool(((y.double() - want).abs() <= bound + 2.0 ** -8 * want.abs()).all())


@pytest.mark.parametrize("rows", [1, 37, 128])
@pytest.mark.parametrize("dim", [256, 4096])
def test_fused_reduce_is_bit_identical_to_the_pair(rows, dim):
    g = torch.Generator(device="cuda").manual_seed(rows + dim)
    part = torch.randn(3, rows, dim, device="cuda", generator=g)
    w = (1 + 0.1 * torch.randn(dim, device="cuda", generator=g)).bfloat16()
    r1 = torch.randn(rows, dim, device="cuda", generator=g).bfloat16()
    r2 = r1.clone()
    x8, s = K.splitk_residual_rmsnorm_fp8(part, r1, w, 1e-5)
    e8, es = K.rmsnorm_fp8(K.splitk_reduce(part), w, 1e-5, residual=r2)
    assert torch.equal(r1, r2) and torch.equal(s, es) and torch.equal(x8.view(torch.uint8), e8.view(torch.uint8))


def test_pack_round_trip():
    w8 = torch.randn(192, 384, generator=torch.Generator().manual_seed(5)).to(F8)
    cpu = ref.pack_f8dgemm_weight(w8, 128)                      # two workgroups, the second half padding
    dev = K.pack_f8dgemm_weight(w8.cuda(), torch.ones(1, 192, device="cuda"), bn=128)
    assert torch.equal(dev.data.cpu(), cpu.reshape(-1))
    assert torch.equal(ref.unpack_f8dgemm_weight(cpu, 192).view(torch.uint8), w8.view(torch.uint8))


@pytest.mark.parametrize("B", [1, 5, 17])
def test_decoder_family_sits_inside_the_quantisation_noise(B, monkeypatch):
    """The f8gemm family shares every rounding point with the library FP8 loop and differs in fp32
    summation order only: rel(f8gemm, lib) <= rel(lib, bf16) / 4.  Measured on one MI355X,
    B = 1 / 5 / 17: rel(f8gemm, lib) = 0 / 0 / 0, rel(lib, bf16) = 3.1e-3 / 3.3e-3 / 3.3e-3."""
    def rel(a, b):
        return float((a.float() - b.float()).norm() / b.float().norm())

    cfg, T, i32 = get_config("tiny"), 40, dict(dtype=torch.int32, device="cuda")
    monkeypatch.delenv("CFC_DECODE_FP8_GEMM", raising=False)
    mb = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3))
    ml = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    monkeypatch.setenv("CFC_DECODE_FP8_GEMM", "1")
    mf = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    assert mf.decode_path(B) == "f8gemm" and ml.decode_path(B) == "lib" and mf.decode_path(129) == "lib"
    # sequence b: T prompt tokens in cache blocks 2 b and 2 b + 1, then one decode step
    seq, tok = torch.arange(B, **i32)[:, None], torch.arange(T, **i32)[None]
    ids, bt = ((seq * 31 + tok * 7) % 500 + 3).reshape(-1), torch.cat([2 * seq, 2 * seq + 1], 1).contiguous()
    hidden = []
    for m in (mb, ml, mf):
        kv = PagedKVCache(cfg.layers, 64, m.w.kv_heads, cfg.head_dim, "cuda")
        m.forward_prefill(ids, tok.repeat(B, 1).reshape(-1), (64 * seq + tok).reshape(-1),
                          torch.arange(B + 1, **i32) * T, torch.full((B,), T, **i32), bt, kv)
        pos = torch.full((B,), T, **i32)
        hidden.append(m.forward_decode(ids[::T].contiguous(), pos, 64 * seq[:, 0] + T, pos + 1, bt, kv, part_blocks=4))
    d_lib, d_f8 = rel(hidden[1], hidden[0]), rel(hidden[2], hidden[1])
    print(f"B={B}: rel(f8gemm, lib)={d_f8:.3e} rel(lib, bf16)={d_lib:.3e}")
    assert d_f8 <= d_lib / 4


def test_engine_generates_with_graph_capture(monkeypatch):
    monkeypatch.setenv("CFC_DECODE_FP8_GEMM", "1")
    cfg = get_config("tiny")
    model = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3).to_fp8())
    eng = LLMEngine(model, PagedKVCache(cfg.layers, 64, model.w.kv_heads, cfg.head_dim, "cuda"), prefix_cache=False)
    prompt = [1] + [(11 * i) % 500 + 3 for i in range(150)]
    res = eng.generate([prompt, prompt[:70]], 8, temperature=0.0, ignore_eos=True)
    assert model.decode_path(2) == "f8gemm" and eng.last_used_graph and [len(t) for t in res.tokens] == [8, 8]
