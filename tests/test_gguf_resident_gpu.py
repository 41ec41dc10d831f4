"""GGUF models resident in their quantized blocks only, on the GPU.

1. The unpack kernel (csrc/kernels/qunpack.hip) against the CPU oracle
   ref.pack_dgemm_weight(bf16(G.dequantize(raw)), bn), bit for bit.
2. A Q4_K_M-style model of the "small" preset loaded with resident="bf16" and resident="quant":
   prefill, decode at every dispatch (quantized GEMV, quantized decode GEMM, the scratch route),
   hipGraph replay, rowmajor_layer and the summarizer -- all bit-identical between the two: both
   run the same kernels on the same bf16 weight bits, so no comparison has a tolerance."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from copilot_for_consensus_amd.ops import reference as ref
from copilot_for_consensus_amd.runtime import gguf as G

pytestmark = pytest.mark.gpu

QTYPES = [G.Q4_K, G.Q6_K, G.Q8_0]
SENTINEL = 0x7A5B       # a bf16 bit pattern (~2.8e35) no dequantized weight takes


@functools.lru_cache(maxsize=None)
def _weight(qtype: int, N: int, K: int, seed: int = 0):
    """(QWeight on the GPU, its dequantized bf16 [N, K] on the CPU) -- computed once per shape."""
    from copilot_for_consensus_amd.ops import kernels as KK
    rng = np.random.default_rng(1000 * seed + qtype + N + K)
    raw = G.quantize(rng.standard_normal((N, K)).astype(np.float32) * 0.05, qtype)
    wb = torch.from_numpy(G.dequantize(raw, qtype, (N, K))).to(torch.bfloat16)
    return KK.QWeight.from_raw(raw, qtype, N, K, "cuda"), wb


def _dst(N: int, K: int, bn: int):
    from copilot_for_consensus_amd.ops import kernels as KK
    data = torch.full((N * K,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return KK.PackedWeight(data, N, K, bn)


def _sentinel_rows(n: int, K: int) -> torch.Tensor:
    return torch.full((n, K), SENTINEL, dtype=torch.int16).view(torch.bfloat16)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1).view(torch.int16).cpu()


def _oracle(w: torch.Tensor, bn: int) -> torch.Tensor:
    return _bits(ref.pack_dgemm_weight(w, bn))


# ------------------------------------------------------------------------------------- 1. kernel

@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("N,K,bns", [(2688, 256, (128, 112, 96, 64)), (2688, 1792, (128, 112, 96, 64)),
                                     (1344, 1792, (112, 96, 64)), (192, 256, (96, 64)), (192, 1792, (96, 64))])
def test_unpack_matches_cpu_oracle(qtype, N, K, bns):
    """One block (K = 256) and an odd count of seven (K = 1792); N = 2688 = lcm(128, 112, 96, 64) is
    the smallest row count every tile width divides (1344 = lcm(112, 96, 64) leaves half a 128-row
    tile), N = 192 two or three tiles."""
    from copilot_for_consensus_amd.ops import kernels as KK
    qw, wb = _weight(qtype, N, K)
    for bn in bns:
        assert KK.qunpack_ok(qw, bn)
        got = KK.qunpack(qw, _dst(N, K, bn))
        assert torch.equal(_bits(got.data), _oracle(wb, bn)), (qtype, N, K, bn)


@pytest.mark.parametrize("K", [256, 1792])
def test_unpack_every_k_split_writes_the_same_bits(K):
    from copilot_for_consensus_amd.ops import kernels as KK
    qw, wb = _weight(G.Q4_K, 192, K)
    want = _oracle(wb, 64)
    for split in range(1, K // 256 + 1):
        assert torch.equal(_bits(KK.qunpack(qw, _dst(192, K, 64), split=split).data), want), split


@pytest.mark.parametrize("bn", [128, 96, 64])
def test_unpack_mixed_type_qkv_fills_one_buffer(bn):
    """Q4_K q (256 rows), Q4_K k (64) and Q6_K v (64) into one 384-row destination via row0."""
    from copilot_for_consensus_amd.ops import kernels as KK
    K = 512
    (q, qb), (k, kb), (v, vb) = _weight(G.Q4_K, 256, K), _weight(G.Q4_K, 64, K, 1), _weight(G.Q6_K, 64, K, 2)
    dst = _dst(384, K, bn)
    KK.qunpack(q, dst)
    KK.qunpack(k, dst, row0=256)
    KK.qunpack(v, dst, row0=320)
    got = _bits(dst.data)
    assert not bool((got == SENTINEL).any())                    # every row overwritten
    assert torch.equal(got, _oracle(torch.cat([qb, kb, vb]), bn))


@pytest.mark.parametrize("qtype", [G.Q4_K, G.Q6_K])
@pytest.mark.parametrize("rows,bn", [(384, 128), (384, 96), (448, 112), (448, 64)])
def test_unpack_gate_up_interleave(qtype, rows, bn):
    """gate + up of F = 176 rows into one 8-row interleaved range (2 F = 352 rows is no multiple of a
    tile width: the destination's remaining rows keep their bytes)."""
    from copilot_for_consensus_amd.ops import kernels as KK
    F, K = 176, 512
    (g, gb), (u, ub) = _weight(qtype, F, K), _weight(qtype, F, K, 1)
    dst = _dst(rows, K, bn)
    KK.qunpack(g, dst, interleave="gate")
    KK.qunpack(u, dst, interleave="up")
    want = torch.cat([ref.interleave_gate_up(torch.cat([gb, ub])), _sentinel_rows(rows - 2 * F, K)])
    assert torch.equal(_bits(dst.data), _oracle(want, bn))


@pytest.mark.parametrize("bn", [96, 64])
def test_unpack_writes_stay_inside_the_row_range(bn):
    from copilot_for_consensus_amd.ops import kernels as KK
    K = 1792
    qw, wb = _weight(G.Q4_K, 64, K)
    dst = _dst(192, K, bn)
    KK.qunpack(qw, dst, row0=64)
    want = torch.cat([_sentinel_rows(64, K), wb, _sentinel_rows(64, K)])
    assert torch.equal(_bits(dst.data), _oracle(want, bn))


def test_unpack_argument_errors():
    from copilot_for_consensus_amd.ops import kernels as KK
    qw, _ = _weight(G.Q4_K, 64, 256)
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 256, 64), row0=8)                       # row0 % 16
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 256, 48))                               # no tile width of the decode GEMM
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 256, 128))                              # 192 rows are not whole 128-row tiles
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 256, 64), row0=144)                     # rows [144, 208) past 192
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 256, 64), row0=96, interleave="gate")   # a 128-row pair past 192
    with pytest.raises(ValueError):
        KK.qunpack(qw, _dst(192, 512, 64))                               # K mismatch
    q5 = KK.QWeight(G.Q5_K, 64, 256, qw.buf, qw.offs)
    assert not KK.qunpack_ok(q5, 64)
    with pytest.raises(ValueError):
        KK.qunpack(q5, _dst(192, 256, 64))                               # unsupported type
    with pytest.raises(ValueError):
        KK.qunpack(qw, KK.PackedWeight(torch.zeros(192 * 256, device="cuda"), 192, 256, 64))   # fp32 destination


# -------------------------------------------------------------------------------------- 2. model

def _write_q4km(path, cfg):
    """The Q4_K_M-style file of test_gguf.py: Q4_K projections, Q6_K v / every other down / output."""
    torch.manual_seed(0)
    sd = {}
    h, f = cfg.hidden, cfg.ffn
    sd["model.embed_tokens.weight"] = torch.randn(cfg.vocab_size, h).numpy()
    sd["lm_head.weight"] = (torch.randn(cfg.vocab_size, h) * 0.2).numpy()     # peaked logits (std ~6)
    sd["model.norm.weight"] = np.ones(h, np.float32)
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"] = np.ones(h, np.float32)
        sd[p + "post_attention_layernorm.weight"] = np.ones(h, np.float32)
        sd[p + "self_attn.q_proj.weight"] = (torch.randn(cfg.heads * cfg.head_dim, h) * 0.02).numpy()
        sd[p + "self_attn.k_proj.weight"] = (torch.randn(cfg.kv_heads * cfg.head_dim, h) * 0.02).numpy()
        sd[p + "self_attn.v_proj.weight"] = (torch.randn(cfg.kv_heads * cfg.head_dim, h) * 0.02).numpy()
        sd[p + "self_attn.o_proj.weight"] = (torch.randn(h, cfg.heads * cfg.head_dim) * 0.005).numpy()
        sd[p + "mlp.gate_proj.weight"] = (torch.randn(f, h) * 0.02).numpy()
        sd[p + "mlp.up_proj.weight"] = (torch.randn(f, h) * 0.02).numpy()
        sd[p + "mlp.down_proj.weight"] = (torch.randn(h, f) * 0.005).numpy()
    qt = {"output.weight": G.Q6_K, "token_embd.weight": G.Q4_K}
    for i in range(cfg.layers):
        qt[f"blk.{i}.attn_v.weight"] = G.Q6_K
        qt[f"blk.{i}.ffn_down.weight"] = G.Q6_K if i % 2 == 0 else G.Q4_K
    G.write_llama_gguf(path, cfg, sd, qtypes=qt, default_qtype=G.Q4_K)


def _under(env: dict, build):
    """build() with the flags set, as the existing tests do: set, build, pop."""
    os.environ.update(env)
    try:
        return build()
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """(bf16-resident, quant-resident) DecoderModels of one file.  The bf16-resident one is built
    under CFC_DECODE_QGEMV=1 CFC_DECODE_QGEMM=1: B <= 4 on the quantized GEMV, B <= 128 on the
    quantized decode GEMM, more rows on its packed bf16 decode GEMM."""
    from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
    path = tmp_path_factory.mktemp("resident") / "q4km.gguf"
    _write_q4km(path, get_config("small"))
    wb = DecoderWeights.from_gguf(path, "cuda", resident="bf16")
    wq = DecoderWeights.from_gguf(path, "cuda", resident="quant")
    mb = _under({"CFC_DECODE_QGEMV": "1", "CFC_DECODE_QGEMM": "1"}, lambda: DecoderModel(wb))
    mq = DecoderModel(wq)
    assert mb.w.packed is not None and mb.decode_qgemv and mb.decode_qgemm and mb.qgemm_max_m == 128
    return mb, mq


def test_quant_resident_structure(models):
    mb, mq = models
    w = mq.w
    assert w.quant_only and not mb.w.quant_only and w.packed is None and w.packed_lm_head is None
    assert all(layer[k] is None for layer in w.layers for k in ("qkv", "o", "gate_up", "down"))
    assert w.lm_head is None and w.q_lm_head is not None          # output.weight is Q6_K: quantized head only
    cfg = w.cfg
    biggest = max((cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim * cfg.hidden, cfg.hidden * cfg.heads * cfg.head_dim,
                  2 * cfg.ffn * cfg.hidden, cfg.hidden * cfg.ffn)
    rb, rbb = w.resident_bytes(), mb.w.resident_bytes()
    assert rb["bf16_projections"] == 0 and rb["scratch"] == 2 * biggest and rb["quant"] == rbb["quant"] > 0
    assert mq._scratch_data.numel() == biggest
    assert rbb["scratch"] == 0 and rbb["bf16_projections"] >= 2 * sum(
        n * k for n, k in mb.w.projection_shapes().values()) * cfg.layers
    assert rb["bf16_other"] == rbb["bf16_other"] - 2 * 2 * cfg.vocab_size * cfg.hidden   # no bf16 / packed head
    for B, path in ((1, "qgemv"), (4, "qgemv"), (5, "qgemm"), (128, "qgemm"), (129, "scratch"), (300, "scratch")):
        assert mq.decode_path(B) == path
    assert mb.decode_path(130) == "dgemm"


def test_quant_resident_refuses_modes_without_a_bf16_copy(models):
    from copilot_for_consensus_amd.models.decoder import DecoderModel
    _, mq = models
    for env in ({"CFC_DECODE_QGEMM": "0"}, {"CFC_PREFILL_GEMM": "lib"}, {"CFC_DECODE_GEMM": "splitk"}):
        with pytest.raises(ValueError):
            _under(env, lambda: DecoderModel(mq.w))


def _prefill(model, lens, seed: int = 3):
    """Prompts of ``lens`` tokens prefilled, packed, into a fresh cache.  Returns the last-token
    logits and the arguments of one decode step on that cache."""
    from copilot_for_consensus_amd.runtime.kv_cache import KV_BLOCK, PagedKVCache
    cfg, B = model.cfg, len(lens)
    i32 = dict(dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(seed)
    per = -(-(max(lens) + 1) // KV_BLOCK)
    kv = PagedKVCache(cfg.layers, per * B + 1, cfg.kv_heads, cfg.head_dim, "cuda")
    tables = [list(range(per * s, per * s + per)) for s in range(B)]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], **i32)
    pos = torch.tensor([p for n in lens for p in range(n)], **i32)
    slots = torch.tensor([tables[s][p // KV_BLOCK] * KV_BLOCK + p % KV_BLOCK for s in range(B) for p in range(lens[s])],
                         **i32)
    bt = torch.tensor(tables, **i32)
    cu = torch.tensor([0] + list(np.cumsum(lens)), **i32)
    last = torch.tensor(list(np.cumsum(lens) - 1), dtype=torch.int64, device="cuda")
    hidden = model.forward_prefill(ids, pos, slots, cu, torch.tensor(lens, **i32), bt, kv, last_idx=last)
    logits = model.logits(hidden).clone()
    nxt = torch.randint(3, cfg.vocab_size, (B,), generator=g).to(**i32)
    dpos = torch.tensor(lens, **i32)
    dslots = torch.tensor([tables[s][n // KV_BLOCK] * KV_BLOCK + n % KV_BLOCK for s, n in enumerate(lens)], **i32)
    return logits, dict(ids=nxt, positions=dpos, slots=dslots, ctx_lens=dpos + 1, block_tables=bt, kv=kv,
                        part_blocks=4)


def _short_lens(B: int) -> list[int]:
    return torch.randint(20, 41, (B,), generator=torch.Generator().manual_seed(B)).tolist()


@pytest.mark.parametrize("lens", [[300, 45], [45]], ids=["pgemm", "decode-gemm-rows"])
def test_prefill_logits_are_bit_identical(models, lens):
    """345 packed rows run the prefill GEMM, 45 rows the decode GEMM below PGEMM_MIN_ROWS -- both on
    the scratch in the quant-resident model."""
    (lb, _), (lq, _) = (_prefill(m, lens) for m in models)
    assert lb.shape == (len(lens), models[0].cfg.vocab_size)
    assert torch.equal(lb, lq)


@pytest.mark.parametrize("B", [2, 6, 33, 130])
def test_decode_step_is_bit_identical(models, B):
    mb, mq = models
    assert mb.decode_path(B) == {2: "qgemv", 6: "qgemm", 33: "qgemm", 130: "dgemm"}[B]
    lens = [300, 45] if B == 2 else _short_lens(B)
    out = []
    for m in models:                        # each model prefills its own cache, then decodes one step on it
        _, step = _prefill(m, lens)
        hidden = m.forward_decode(**step)
        out.append((hidden.clone(), m.logits(hidden).clone(), step["kv"]))
    (hb, lb, kvb), (hq, lq, kvq) = out
    assert all(torch.equal(a, b) for a, b in zip(kvb.k, kvq.k)) and all(torch.equal(a, b) for a, b in zip(kvb.v, kvq.v))
    assert torch.equal(hb, hq)
    assert lb.shape == (B, mb.cfg.vocab_size) and torch.equal(lb, lq)


@pytest.mark.parametrize("B", [6, 130])
def test_quant_resident_graph_replay_is_bit_identical(models, B):
    """A captured step holds the unpack launches (B = 130: every projection and the lm_head chunks)."""
    _, mq = models
    _, step = _prefill(mq, _short_lens(B))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.inference_mode():
        for _ in range(2):                      # eager warm-up on the capture stream: sizes its workspace
            eager = mq.logits(mq.forward_decode(**step)).clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = mq.logits(mq.forward_decode(**step))
        for _ in range(2):
            out.zero_()
            g.replay()
            s.synchronize()
            assert torch.equal(out, eager)
    torch.cuda.current_stream().wait_stream(s)


def test_rowmajor_layer_from_the_blocks(models):
    mb, mq = models
    a, b = mb.w.rowmajor_layer(0), mq.w.rowmajor_layer(0)
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def test_summarizer_generates_the_same_tokens(tmp_path):
    from copilot_for_consensus_amd.models.decoder import DecoderConfig
    from copilot_for_consensus_amd.summarization import HipLLMSummarizer
    toks = ["<unk>", "<s>", "</s>"] + [f"<0x{i:02X}>" for i in range(256)]
    chars = sorted(set("abcdefghijklmnopqrstuvwxyz:.,"))
    toks += ["▁"] + chars + ["▁" + c for c in chars] + ["▁ab", "▁the"]
    assert len(toks) == 320
    types = [2, 3, 3] + [6] * 256 + [1] * (len(toks) - 259)
    cfg = DecoderConfig("tiny-resident", len(toks), 256, 2, 2, 1, 128, 512, max_positions=1024)
    rng = np.random.default_rng(0)
    sd = {"model.embed_tokens.weight": rng.standard_normal((cfg.vocab_size, 256)).astype(np.float32),
          "lm_head.weight": rng.standard_normal((cfg.vocab_size, 256)).astype(np.float32) * 0.2,
          "model.norm.weight": np.ones(256, np.float32)}
    for i in range(2):
        p = f"model.layers.{i}."
        for n, shape in (("self_attn.q_proj", (256, 256)), ("self_attn.k_proj", (128, 256)),
                         ("self_attn.v_proj", (128, 256)), ("self_attn.o_proj", (256, 256)),
                         ("mlp.gate_proj", (512, 256)), ("mlp.up_proj", (512, 256)), ("mlp.down_proj", (256, 512))):
            sd[p + n + ".weight"] = rng.standard_normal(shape).astype(np.float32) * 0.05
        sd[p + "input_layernorm.weight"] = np.ones(256, np.float32)
        sd[p + "post_attention_layernorm.weight"] = np.ones(256, np.float32)
    path = tmp_path / "tiny.gguf"
    G.write_llama_gguf(path, cfg, sd, tokens=toks, token_types=types, default_qtype=G.Q4_K,
                       qtypes={"output.weight": G.Q6_K, "blk.1.attn_v.weight": G.Q8_0})
    kw = dict(gguf_path=str(path), max_new_tokens=8, kv_cache_tokens=4096, ignore_eos=True)
    sb = _under({"CFC_DECODE_QGEMV": "1", "CFC_DECODE_QGEMM": "1"}, lambda: HipLLMSummarizer(gguf_resident="bf16", **kw))
    sq = HipLLMSummarizer(gguf_resident="quant", **kw)
    assert sq.decoder.w.quant_only and not sb.decoder.w.quant_only
    ids = [s.tokenizer.encode(t) for s in (sb,) for t in ("summarize: the thread.", "a b, c.")]
    got = [s.generate_ids(ids).tokens for s in (sb, sq)]
    assert all(len(t) == 8 for t in got[0]) and got[0] == got[1]
