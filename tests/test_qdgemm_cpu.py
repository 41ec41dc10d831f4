"""Host side of the quantized decode GEMM: the launch configuration, the shape gate and the decode
path the model reports -- no GPU needed."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime import gguf as G


def _projections(cfg):
    """(N, K, ggml type) of every projection of a Q4_K_M checkpoint of ``cfg`` (and Q8_0 of each)."""
    D = cfg.head_dim
    shapes = {"q": (cfg.heads * D, cfg.hidden), "k": (cfg.kv_heads * D, cfg.hidden), "v": (cfg.kv_heads * D, cfg.hidden),
              "o": (cfg.hidden, cfg.heads * D), "gate": (cfg.ffn, cfg.hidden), "up": (cfg.ffn, cfg.hidden),
              "gate_up": (2 * cfg.ffn, cfg.hidden), "qkv": ((cfg.heads + 2 * cfg.kv_heads) * D, cfg.hidden),
              "down": (cfg.hidden, cfg.ffn), "lm_head": (cfg.vocab_size, cfg.hidden)}
    return [(n, k, t) for n, k in shapes.values() for t in (G.Q4_K, G.Q6_K, G.Q8_0)]


@pytest.mark.parametrize("preset", ["mistral-7b", "llama-3-8b"])
@pytest.mark.parametrize("M", [5, 16, 64, 128])
def test_qdgemm_config_is_launchable(preset, M):
    for N, Kd, qtype in _projections(get_config(preset)):
        bn, split = K.qdgemm_config(M, N, Kd, qtype)
        assert 1 <= split <= Kd // 256, (N, Kd, qtype, split)
        assert bn % 16 == 0 and bn in K.QDGEMM_BNS, (N, Kd, qtype, bn)
        assert bn >= 8 * -(-M // 16)        # what the kernel's X staging needs (qdgemm.hip)


def test_qdgemm_config_splits_small_n_and_not_wide_n():
    # k / v of Mistral-7B: 1024 rows are 8-64 workgroups -- the K parts fill the chip; gate + up are
    # hundreds of workgroups on their own
    assert K.qdgemm_config(128, 1024, 4096, G.Q4_K)[1] > 1
    assert K.qdgemm_config(128, 2 * 14336, 4096, G.Q4_K)[1] <= 2
    assert K.qdgemm_config(8, 4096, 256, G.Q4_K)[1] == 1   # one block: nothing to split


def _qw(N, Kd, qtype=G.Q4_K):
    return K.QWeight(qtype, N, Kd, torch.empty(0, dtype=torch.uint8), (0, 0, 0))


def test_qdgemm_ok_gates_shapes_and_types():
    assert K.QDGEMM_MAX_M == 128
    assert K.qdgemm_ok(1, _qw(208, 256)) and K.qdgemm_ok(128, _qw(4096, 14336, G.Q6_K))
    assert K.qdgemm_ok(5, _qw(64, 512, G.Q8_0))
    assert not K.qdgemm_ok(129, _qw(208, 256))
    assert not K.qdgemm_ok(0, _qw(208, 256))
    assert not K.qdgemm_ok(8, _qw(200, 256))
    assert not K.qdgemm_ok(8, _qw(208, 384))
    assert not K.qdgemm_ok(8, _qw(208, 256, G.Q4_0))
    assert not K.qdgemm_ok(8, torch.zeros(208, 256))


def _model(monkeypatch, quant: bool, flag: str | None = None):
    w = DecoderWeights.random(get_config("tiny"), "cpu", seed=1)
    if quant:
        K.attach_random_quant(w)
    if flag is None:
        monkeypatch.delenv("CFC_DECODE_QGEMM", raising=False)
    else:
        monkeypatch.setenv("CFC_DECODE_QGEMM", flag)
    return DecoderModel(w)


def test_decode_path_of_a_quantized_model(monkeypatch):
    m = _model(monkeypatch, True, "1")           # 1: every batch the kernel supports
    assert m.decode_qgemm and m.decode_qgemv and m.qgemm_max_m == K.QDGEMM_MAX_M
    for B in (1, 2, 4):
        assert m.decode_path(B, on_gpu=True) == "qgemv"
    for B in (5, 6, 8, 33, 64, 127, 128):
        assert m.decode_path(B, on_gpu=True) == "qgemm"
    for B in (129, 256, 300):
        assert m.decode_path(B, on_gpu=True) in ("dgemm", "splitk", "lib")
    assert m.decode_path(6) == "qgemm"                     # on_gpu defaults to True
    assert m.decode_path(6, on_gpu=False) == "lib"         # nothing quantized runs on the CPU


def test_decode_path_default_bound_is_the_measured_gate(monkeypatch):
    """Unset, the quantized GEMM is on up to the largest batch bucket at which it measured faster
    than the bf16 decode GEMM (K.QDGEMM_DEFAULT_MAX_M); an integer sets another bound."""
    m = _model(monkeypatch, True)
    assert m.decode_qgemm and 8 <= K.QDGEMM_DEFAULT_MAX_M <= K.QDGEMM_MAX_M
    for B in range(1, 300):
        want = "qgemv" if B <= 4 else "qgemm" if B <= K.QDGEMM_DEFAULT_MAX_M else None
        if want:
            assert m.decode_path(B) == want
        else:
            assert m.decode_path(B) in ("dgemm", "splitk")
    m = _model(monkeypatch, True, "64")
    assert m.decode_path(64) == "qgemm" and m.decode_path(65) in ("dgemm", "splitk")
    with pytest.raises(ValueError):
        _model(monkeypatch, True, "yes")


def test_decode_path_with_the_quantized_gemm_switched_off(monkeypatch):
    on, off = _model(monkeypatch, True, "1"), _model(monkeypatch, True, "0")
    assert not off.decode_qgemm and off.decode_qgemv
    for B in range(1, 300):
        assert off.decode_path(B) != "qgemm"
        if not 4 < B <= 128:
            assert off.decode_path(B) == on.decode_path(B)
    assert off.decode_path(2) == "qgemv" and off.decode_path(6) in ("dgemm", "splitk")


def test_decode_path_of_a_model_without_quantized_copies(monkeypatch):
    plain = _model(monkeypatch, False)
    assert not plain.decode_qgemm
    for flag in ("0", "1"):
        m = _model(monkeypatch, False, flag)
        for B in (1, 4, 5, 128, 129, 300):
            assert m.decode_path(B) == plain.decode_path(B)
            assert m.decode_path(B) in ("gemv", "dgemm", "splitk", "lib")
    assert plain.decode_path(1) == "gemv" and plain.decode_path(8) in ("dgemm", "splitk")
    assert plain.decode_path(8, on_gpu=False) == "lib"
