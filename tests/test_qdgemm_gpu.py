"""The quantized decode GEMM (csrc/kernels/qdgemm.hip): batched decode (4 < B <= 128) straight from
the ggml Q4_K / Q6_K / Q8_0 blocks, from the kernel up to the engine.

Kernel results are compared on the CPU against two references of the same quantized weight,
``R32 = x @ dequantize(raw)^T`` and ``Rbf = x @ bf16(dequantize(raw))^T`` (the kernel may multiply
the exact fp32 dequantized value or its bf16 rounding), and pass when they are close to EITHER at
the tolerances of the quantized GEMV's test: fp32 slabs rtol 2e-3 / atol 2e-3 max|want|, the bf16
epilogue 1e-2 / 1e-2, SwiGLU 2e-2 / 2e-2.  References are computed once per weight at M = 128 and
sliced."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from copilot_for_consensus_amd.runtime import gguf as G

pytestmark = pytest.mark.gpu

QTYPES = [G.Q4_K, G.Q6_K, G.Q8_0]
MAX_M = 128


@functools.lru_cache(maxsize=None)
def _x(K: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + K)
    return torch.randn(MAX_M, K, generator=g).bfloat16()


@functools.lru_cache(maxsize=None)
def _weight(qtype: int, N: int, K: int, seed: int = 7):
    """(QWeight on the GPU, R32 [128, N], Rbf [128, N]) of one random quantized weight."""
    from copilot_for_consensus_amd.ops import kernels as KK
    rng = np.random.default_rng(seed + 131 * qtype + N + K)
    raw = G.quantize(rng.standard_normal((N, K)).astype(np.float32) * 0.05, qtype)
    wf = torch.from_numpy(G.dequantize(raw, qtype, (N, K)))
    x = _x(K).float()
    return KK.QWeight.from_raw(raw, qtype, N, K, "cuda"), x @ wf.t(), x @ wf.bfloat16().float().t()


def _assert_either(got: torch.Tensor, wants, rtol: float, frac: float, what: str):
    """``got`` is assert_close to at least one of ``wants`` (atol = frac * max|want|)."""
    errs = []
    for want in wants:
        atol = frac * float(want.abs().max())
        excess = float(((got - want).abs() - rtol * want.abs()).max()) / atol   # <= 1 passes
        print(f"{what}: worst (|err| - rtol |want|) / atol = {excess:.3f}")
        try:
            torch.testing.assert_close(got, want, rtol=rtol, atol=atol)
            return
        except AssertionError as e:
            errs.append(str(e))
    raise AssertionError(f"{what}: close to neither reference\n" + "\n".join(errs))


# ------------------------------------------------------------------------------------ 1. main sweep

@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("M", [5, 16, 17, 128])
@pytest.mark.parametrize("N,K", [(208, 256), (208, 1792), (64, 14336)])
def test_qdgemm_matches_dequantized_linear(qtype, M, N, K):
    from copilot_for_consensus_amd.ops import kernels as KK
    qw, r32, rbf = _weight(qtype, N, K)
    x = _x(K)[:M].cuda()
    wants = (r32[:M], rbf[:M])
    assert KK.qdgemm_ok(M, qw)
    bn, csplit = KK.qdgemm_config(M, N, K, qtype)
    assert 1 <= csplit <= K // 256 and bn % 16 == 0
    splits = {csplit, 1} | ({2, 3} if K == 1792 else set())
    for split in sorted(splits):
        part = KK.qdgemm(x, qw, "part", split=split)
        assert part.shape == (split, M, N) and part.dtype == torch.float32
        _assert_either(part.sum(0).cpu(), wants, 2e-3, 2e-3, f"slabs split={split}")
    for b in KK.QDGEMM_BNS:             # every workgroup width the kernel is built for at this M
        if b >= 8 * -(-M // 16) and b != bn:
            part = KK.qdgemm(x, qw, "part", split=1, bn=b)
            _assert_either(part.sum(0).cpu(), wants, 2e-3, 2e-3, f"slabs bn={b}")
    out = KK.qdgemm(x, qw, "bf16")
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _assert_either(out.float().cpu(), wants, 1e-2, 1e-2, "bf16")


# ------------------------------------------------------------------------- 2. writes stay in bounds

@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("M", [5, 17])
def test_qdgemm_writes_only_its_column_range(qtype, M):
    from copilot_for_consensus_amd.ops import kernels as KK
    N, K, split = 208, 1792, 3
    qw, r32, rbf = _weight(qtype, N, K)
    x = _x(K)[:M].cuda()
    sent = -12345.0
    # fp32 slabs: one spare slab, one spare row, the range in the middle of a 3 N wide buffer
    buf = torch.full((split + 1, M + 1, 3 * N), sent, dtype=torch.float32, device="cuda")
    KK.qdgemm(x, qw, "part", split=split, out=buf[:split, :M], col0=N)
    got = buf.cpu()
    inside = torch.zeros_like(got, dtype=torch.bool)
    inside[:split, :M, N:2 * N] = True
    assert bool((got[~inside] == sent).all())
    assert bool((got[inside] != sent).all())
    _assert_either(got[:split, :M, N:2 * N].sum(0), (r32[:M], rbf[:M]), 2e-3, 2e-3, "slabs in a slice")
    # interleaved halves: "gate" writes columns 16 t .. 16 t + 7 of a 2 N range, "up" the other eight
    buf = torch.full((split + 1, M + 1, 4 * N), sent, dtype=torch.float32, device="cuda")
    KK.qdgemm(x, qw, "part", split=split, out=buf[:split, :M], col0=N, interleave="up")
    got = buf.cpu()
    inside = torch.zeros_like(got, dtype=torch.bool)
    cols = torch.arange(2 * N)
    inside[:split, :M, N:3 * N] = (cols % 16 >= 8)
    assert bool((got[~inside] == sent).all())
    assert bool((got[inside] != sent).all())
    # bf16 rows
    bb = torch.full((M + 1, 3 * N), sent, dtype=torch.bfloat16, device="cuda")
    ref = bb.clone()
    KK.qdgemm(x, qw, "bf16", out=bb[:M], col0=N)
    got, ref = bb.cpu(), ref.cpu()
    inside = torch.zeros_like(got, dtype=torch.bool)
    inside[:M, N:2 * N] = True
    assert torch.equal(got[~inside], ref[~inside])
    _assert_either(got[:M, N:2 * N].float(), (r32[:M], rbf[:M]), 1e-2, 1e-2, "bf16 in a slice")


# ------------------------------------------------------------------------------- 3. mixed-type qkv

def test_qdgemm_mixed_type_qkv_slabs():
    from copilot_for_consensus_amd.ops import kernels as KK
    K, M = 512, 6
    parts = [(G.Q4_K, 128), (G.Q4_K, 32), (G.Q6_K, 32)]
    x = _x(K)[:M].cuda()
    for split in (1, 2):
        buf = torch.zeros(split, M, 192, dtype=torch.float32, device="cuda")
        col = 0
        for qtype, N in parts:
            KK.qdgemm(x, _weight(qtype, N, K, seed=11 + col)[0], "part", out=buf, col0=col)
            col += N
        got = KK.splitk_reduce(buf).float().cpu()
        col = 0
        for qtype, N in parts:
            _, r32, rbf = _weight(qtype, N, K, seed=11 + col)
            _assert_either(got[:, col:col + N], (r32[:M], rbf[:M]), 1e-2, 1e-2, f"qkv columns {col}..{col + N}")
            col += N


# --------------------------------------------------------------------------- 4. gate / up interleave

@pytest.mark.parametrize("qtype", [G.Q4_K, G.Q6_K])
@pytest.mark.parametrize("split", [1, 2])
def test_qdgemm_gate_up_interleave_swiglu(qtype, split):
    from copilot_for_consensus_amd.ops import kernels as KK
    N, K, M = 208, 512, 17
    gate, g32, gbf = _weight(qtype, N, K, seed=21)
    up, u32, ubf = _weight(qtype, N, K, seed=22)
    x = _x(K)[:M].cuda()
    buf = torch.zeros(split, M, 2 * N, dtype=torch.float32, device="cuda")
    KK.qdgemm(x, gate, "part", out=buf, interleave="gate")
    KK.qdgemm(x, up, "part", out=buf, interleave="up")
    # the slab holds the 8-row interleaved order: columns 16 t .. + 7 gate rows 8 t .., the next 8 up
    s = buf.sum(0).cpu().view(M, N // 8, 2, 8)
    _assert_either(s[:, :, 0].reshape(M, N), (g32[:M], gbf[:M]), 2e-3, 2e-3, "gate columns")
    _assert_either(s[:, :, 1].reshape(M, N), (u32[:M], ubf[:M]), 2e-3, 2e-3, "up columns")
    got = KK.splitk_reduce(buf, swiglu=True).float().cpu()
    assert got.shape == (M, N)
    refs = [torch.nn.functional.silu(g[:M].bfloat16().float()) * u[:M].bfloat16().float()
            for g, u in ((g32, u32), (gbf, ubf))]
    _assert_either(got, refs, 2e-2, 2e-2, "swiglu")


# ----------------------------------------------------------------------------- 5. agrees with qgemv

@pytest.mark.parametrize("qtype", QTYPES)
def test_qdgemm_agrees_with_qgemv_at_m4(qtype):
    from copilot_for_consensus_amd.ops import kernels as KK
    N, K = 208, 1792
    qw, _, _ = _weight(qtype, N, K)
    x = _x(K)[:4].cuda()
    want = KK.qgemv(x, qw, "f32").cpu()
    got = KK.qdgemm(x, qw, "part", split=1)[0].cpu()
    torch.testing.assert_close(got, want, rtol=2e-3, atol=2e-3 * float(want.abs().max()))


# -------------------------------------------------------------------------------- 6. determinism

@pytest.mark.parametrize("qtype", QTYPES)
def test_qdgemm_is_deterministic(qtype):
    from copilot_for_consensus_amd.ops import kernels as KK
    N, K, M = 208, 1792, 33
    qw, _, _ = _weight(qtype, N, K)
    x = _x(K)[:M].cuda()
    a = KK.qdgemm(x, qw, "part", split=3).clone()
    b = KK.qdgemm(x, qw, "part", split=3).clone()
    assert torch.equal(a, b)


def test_qdgemm_argument_errors():
    from copilot_for_consensus_amd.ops import kernels as KK
    qw, _, _ = _weight(G.Q4_K, 208, 1792)
    x = _x(1792).cuda()
    with pytest.raises(ValueError):
        KK.qdgemm(x[:5, :1536].contiguous(), qw)                      # K mismatch
    with pytest.raises(ValueError):
        KK.qdgemm(x[:5], qw, "part", split=8)                         # more parts than blocks
    with pytest.raises(ValueError):
        KK.qdgemm(x[:5], qw, "bf16", split=2)
    with pytest.raises(ValueError):
        KK.qdgemm(x[:5], qw, "part", out=torch.zeros(1, 5, 100, device="cuda"))   # too narrow
    with pytest.raises(ValueError):
        KK.qdgemm(torch.cat([x, x[:1]]), qw)                          # M = 129


# --------------------------------------------------------------------------------- 7-9. model level

@pytest.fixture(scope="module")
def gguf_weights(tmp_path_factory):
    """The Q4_K_M-style GGUF of the "small" preset (Q4_K projections, Q6_K v / every other down /
    output), as test_gguf.py builds it."""
    from copilot_for_consensus_amd.models.decoder import DecoderWeights, get_config
    cfg = get_config("small")
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
    path = tmp_path_factory.mktemp("qdgemm") / "q4km.gguf"
    G.write_llama_gguf(path, cfg, sd, qtypes=qt, default_qtype=G.Q4_K)
    wq = DecoderWeights.from_gguf(path, "cuda")
    assert wq.qlayers is not None and wq.q_lm_head is not None
    return wq


def _model(wq, flag: str):
    from copilot_for_consensus_amd.models.decoder import DecoderModel
    os.environ["CFC_DECODE_QGEMM"] = flag
    try:
        return DecoderModel(wq)
    finally:
        os.environ.pop("CFC_DECODE_QGEMM", None)


@pytest.fixture(scope="module")
def models(gguf_weights):
    on, off = _model(gguf_weights, "1"), _model(gguf_weights, "0")
    assert on.decode_qgemm and not off.decode_qgemm
    return on, off


def _prefilled(model, B: int, seed: int = 3):
    """B prompts of 20-60 tokens prefilled into a fresh cache; returns the arguments of one decode step."""
    from copilot_for_consensus_amd.runtime.kv_cache import KV_BLOCK, PagedKVCache
    cfg = model.cfg
    i32 = dict(dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(20, 61, (B,), generator=g).tolist()
    kv = PagedKVCache(cfg.layers, 2 * B + 2, cfg.kv_heads, cfg.head_dim, "cuda")
    tables = [[2 * s, 2 * s + 1] for s in range(B)]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]
    ids = torch.tensor([t for p in prompts for t in p], **i32)
    pos = torch.tensor([p for n in lens for p in range(n)], **i32)
    slots = torch.tensor([tables[s][p // KV_BLOCK] * KV_BLOCK + p % KV_BLOCK for s in range(B) for p in range(lens[s])],
                         **i32)
    bt = torch.tensor(tables, **i32)
    cu = torch.tensor([0] + list(np.cumsum(lens)), **i32)
    model.forward_prefill(ids, pos, slots, cu, torch.tensor(lens, **i32), bt, kv)
    nxt = torch.randint(3, cfg.vocab_size, (B,), generator=g).to(**i32)
    dpos = torch.tensor(lens, **i32)
    dslots = torch.tensor([tables[s][n // KV_BLOCK] * KV_BLOCK + n % KV_BLOCK for s, n in enumerate(lens)], **i32)
    return dict(ids=nxt, positions=dpos, slots=dslots, ctx_lens=dpos + 1, block_tables=bt, kv=kv, part_blocks=4)


@pytest.mark.parametrize("B", [6, 33])
def test_model_decode_on_quantized_gemm_matches_dequantized(models, B):
    on, off = models
    assert on.decode_path(6) == "qgemm" and on.decode_path(128) == "qgemm" and on.decode_path(2) == "qgemv"
    assert off.decode_path(6) in ("dgemm", "splitk") and off.decode_path(2) == "qgemv"
    assert on.decode_path(B) == "qgemm" and off.decode_path(B) in ("dgemm", "splitk")
    step = _prefilled(off, B)
    logits = [m.logits(m.forward_decode(**step)).float().cpu() for m in (on, off)]   # the step rewrites one slot
    a, b = logits
    cos = torch.nn.functional.cosine_similarity(a, b, dim=-1)
    print(f"B={B}: min cos {float(cos.min()):.6f}, max |d| / std {float((a - b).abs().max() / b.std()):.4f}")
    assert float(cos.min()) > 0.999, cos
    assert float((a - b).abs().max()) < 0.5 * float(b.std()), (a - b).abs().max()


def test_model_decode_on_quantized_gemm_graph_replay_is_bit_identical(models):
    on, _ = models
    step = _prefilled(on, 6)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.inference_mode():
        for _ in range(2):                      # eager warm-up on the capture stream: sizes its workspace
            eager = on.logits(on.forward_decode(**step)).clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = on.logits(on.forward_decode(**step))
        for _ in range(2):
            out.zero_()
            g.replay()
            s.synchronize()
            assert torch.equal(out, eager)
    torch.cuda.current_stream().wait_stream(s)


def test_engine_generates_same_tokens_with_and_without_graphs(models):
    from copilot_for_consensus_amd.runtime.engine import LLMEngine
    from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache
    on, _ = models
    cfg = on.cfg
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(20, 61, (6,), generator=g).tolist()
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in lens]
    toks = []
    for use_graph in (True, False):
        kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, cfg.head_dim, "cuda")
        eng = LLMEngine(on, kv, max_prefill_tokens=512, use_graph=use_graph, prefix_cache=False)
        toks.append(eng.generate(prompts, 8, ignore_eos=True).tokens)
        assert eng.last_used_graph == use_graph
    assert all(len(t) == 8 for t in toks[0])
    assert toks[0] == toks[1]
