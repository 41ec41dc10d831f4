"""GGUF models resident in their quantized blocks only: the CPU side -- QWeight.to_rowmajor_bf16 (the
inverse of the planar GPU layout, the oracle of the unpack kernel), the loader's refusals and the
configuration key."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderConfig, DecoderWeights
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime import gguf as G


@pytest.mark.parametrize("qtype", [G.Q4_K, G.Q6_K, G.Q8_0])
@pytest.mark.parametrize("shape", [(32, 256), (48, 1792)])
@pytest.mark.parametrize("permute", [False, True])
def test_to_rowmajor_bf16_inverts_the_planar_layout(qtype, shape, permute):
    N, Kd = shape
    rng = np.random.default_rng(N + Kd + qtype)
    raw = G.quantize(rng.standard_normal(shape).astype(np.float32) * 0.05, qtype)
    rows = rng.permutation(N) if permute else None
    want = torch.from_numpy(G.dequantize(raw, qtype, shape)).to(torch.bfloat16)
    if permute:
        want = want[torch.from_numpy(rows)]
    got = K.QWeight.from_raw(raw, qtype, N, Kd, "cpu", rows=rows).to_rowmajor_bf16()
    assert got.dtype == torch.bfloat16 and got.shape == shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_row_range_of_a_quantized_weight():
    rng = np.random.default_rng(5)
    for qtype in (G.Q4_K, G.Q6_K, G.Q8_0):
        raw = G.quantize(rng.standard_normal((48, 512)).astype(np.float32), qtype)
        qw = K.QWeight.from_raw(raw, qtype, 48, 512, "cpu")
        assert torch.equal(qw.rows(16, 32).to_rowmajor_bf16().view(torch.int16),
                           qw.to_rowmajor_bf16()[16:48].view(torch.int16))
    with pytest.raises(ValueError):
        qw.rows(32, 32)


def _tiny_gguf(path, qtypes=None, default=G.Q4_K):
    cfg = DecoderConfig("tiny-resident", 64, 256, 1, 2, 1, 128, 256, max_positions=256)
    rng = np.random.default_rng(0)
    sd = {"model.embed_tokens.weight": rng.standard_normal((64, 256)).astype(np.float32),
          "lm_head.weight": rng.standard_normal((64, 256)).astype(np.float32),
          "model.norm.weight": np.ones(256, np.float32),
          "model.layers.0.input_layernorm.weight": np.ones(256, np.float32),
          "model.layers.0.post_attention_layernorm.weight": np.ones(256, np.float32)}
    for n, shape in (("self_attn.q_proj", (256, 256)), ("self_attn.k_proj", (128, 256)),
                     ("self_attn.v_proj", (128, 256)), ("self_attn.o_proj", (256, 256)),
                     ("mlp.gate_proj", (256, 256)), ("mlp.up_proj", (256, 256)), ("mlp.down_proj", (256, 256))):
        sd[f"model.layers.0.{n}.weight"] = rng.standard_normal(shape).astype(np.float32) * 0.05
    G.write_llama_gguf(path, cfg, sd, qtypes=qtypes, default_qtype=default)
    return cfg


def test_quant_resident_needs_a_gpu(tmp_path):
    _tiny_gguf(tmp_path / "t.gguf")
    with pytest.raises(ValueError, match="GPU"):
        DecoderWeights.from_gguf(tmp_path / "t.gguf", "cpu", resident="quant")
    w = DecoderWeights.from_gguf(tmp_path / "t.gguf", "cpu")             # the default is unchanged
    assert not w.quant_only and w.layers[0]["qkv"] is not None
    assert w.resident_bytes()["scratch"] == 0 and w.resident_bytes()["bf16_projections"] > 0


def test_unsupported_projection_type_is_named(tmp_path):
    """A file with one Q5_K projection (the Q5_K_M case): no quantized kernel takes it, so the loader
    refuses and names the tensor and its type (on any device: the check comes before the device's)."""
    rng = np.random.default_rng(1)
    w = G.GGUFWriter("llama")
    for key, v in (("general.name", "q5"), ("llama.context_length", 256), ("llama.embedding_length", 256),
                   ("llama.block_count", 1), ("llama.feed_forward_length", 256), ("llama.attention.head_count", 2),
                   ("llama.attention.head_count_kv", 1), ("llama.rope.dimension_count", 128),
                   ("llama.attention.key_length", 128), ("llama.rope.freq_base", 1e4),
                   ("llama.attention.layer_norm_rms_epsilon", 1e-5), ("llama.vocab_size", 64)):
        w.add(key, v)
    for name, shape in (("token_embd", (64, 256)), ("output", (64, 256)), ("blk.0.attn_q", (256, 256)),
                        ("blk.0.attn_k", (128, 256)), ("blk.0.attn_v", (128, 256)), ("blk.0.attn_output", (256, 256)),
                        ("blk.0.ffn_gate", (256, 256)), ("blk.0.ffn_up", (256, 256))):
        w.add_tensor(name + ".weight", rng.standard_normal(shape) * 0.05, G.Q4_K)
    for name in ("output_norm", "blk.0.attn_norm", "blk.0.ffn_norm"):
        w.add_tensor(name + ".weight", np.ones(256), G.F32)
    per, size = G.BLOCK[G.Q5_K]
    blocks = rng.integers(0, 256, (256 * 256 // per, size), dtype=np.uint8)
    blocks[:, 0:4] = np.frombuffer(np.float16(0.01).tobytes() * 2, np.uint8)
    w.add_tensor("blk.0.ffn_down.weight", None, G.Q5_K, raw=blocks.tobytes(), shape=(256, 256))
    w.write(tmp_path / "q5.gguf")
    assert DecoderWeights.from_gguf(tmp_path / "q5.gguf", "cpu").layers[0]["down"].shape == (256, 256)
    with pytest.raises(ValueError, match=r"blk\.0\.ffn_down\.weight \(Q5_K"):
        DecoderWeights.from_gguf(tmp_path / "q5.gguf", "cpu", resident="quant")


def test_unknown_resident_values_raise(tmp_path, monkeypatch):
    from copilot_for_consensus_amd.summarization import HipLLMSummarizer
    _tiny_gguf(tmp_path / "t.gguf", default=G.F32)
    with pytest.raises(ValueError, match="resident"):
        DecoderWeights.from_gguf(tmp_path / "t.gguf", "cpu", resident="q4")
    with pytest.raises(ValueError, match="gguf_resident"):
        HipLLMSummarizer(gguf_path=str(tmp_path / "t.gguf"), device="cpu", gguf_resident="int4")
    monkeypatch.setenv("CFC_GGUF_RESIDENT", "blocks")
    with pytest.raises(ValueError, match="CFC_GGUF_RESIDENT"):
        HipLLMSummarizer(gguf_path=str(tmp_path / "t.gguf"), device="cpu")


def test_spec_key_and_default(monkeypatch):
    from copilot_for_consensus_amd.config import loader
    from copilot_for_consensus_amd.config.specs import ADAPTERS
    assert ADAPTERS["llm_backend"][3]["hip"]["gguf_resident"][1:] == ("LLM_GGUF_RESIDENT", "bf16")
    monkeypatch.delenv("LLM_GGUF_RESIDENT", raising=False)
    assert loader.load_adapter_config("llm_backend", driver="hip").driver_config["gguf_resident"] == "bf16"
    monkeypatch.setenv("LLM_GGUF_RESIDENT", "quant")
    assert loader.load_adapter_config("llm_backend", driver="hip").driver_config["gguf_resident"] == "quant"
