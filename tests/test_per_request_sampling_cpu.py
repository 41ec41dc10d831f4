"""Per-request sampler settings in one slot engine (``per_request_sampling``): the scheduler's
grouping, the CPU reference of ``sample_rows``, the slot reset, the configuration key and the
refusal under tensor parallel -- all on the CPU path, tiny preset."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.config.loader import load_adapter_config
from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.ops import reference as R
from copilot_for_consensus_amd.runtime.continuous import ContinuousEngine
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache
from copilot_for_consensus_amd.runtime.tokenizer import synthetic_bpe
from copilot_for_consensus_amd.serving import build_from_config
from copilot_for_consensus_amd.serving.llm_server import BatchScheduler, GenRequest

# (temperature, top_k, top_p, min_p, seed): six distinct configurations, two of them greedy (a
# negative temperature is greedy too, and GenRequest.key() keeps the temperature: six keys)
CONFIGS = [(0.0, 0, 1.0, 0.0, 0), (-1.0, 40, 0.9, 0.0, 7), (0.7, 0, 1.0, 0.0, 1), (0.8, 1, 1.0, 0.0, 2),
           (0.9, 40, 0.95, 0.05, 3), (1.2, 5, 0.5, 0.1, 4)]
PROMPTS = [[1, 2, 3, 4], [1, 5, 6], [2, 7, 9, 11, 3], [4, 4, 8], [1, 2, 3, 4], [9, 8, 7, 6, 5]]
NEW = 8


@pytest.fixture(scope="module")
def engine():
    cfg = get_config("tiny")
    m = DecoderModel(DecoderWeights.random(cfg, "cpu", seed=0))
    kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, cfg.head_dim, "cpu")
    return LLMEngine(m, kv)


def _requests():
    return [GenRequest(list(p), NEW, t, k, tp, mp, sd, ignore_eos=True)
            for p, (t, k, tp, mp, sd) in zip(PROMPTS, CONFIGS)]


def _serve(engine, monkeypatch, **kw):
    """The six requests through a fresh scheduler, queued before its loop first looks (one batch):
    (tokens per request, engines built, calls of engine.generate)."""
    calls = []
    generate = engine.generate
    monkeypatch.setattr(engine, "generate", lambda *a, **k: calls.append(1) or generate(*a, **k))
    sched = BatchScheduler(engine, synthetic_bpe(engine.cfg.vocab_size), max_batch=8, batch_wait_ms=50.0,
                           max_prompt=64, max_new_cap=16, steps_per_sync=4, **kw)
    try:
        reqs = _requests()
        for r in reqs:
            sched.q.put(r)
        for r in reqs:
            assert r.done.wait(120) and r.error is None, r.error
        return [r.tokens for r in reqs], len(sched.engines), len(calls)
    finally:
        sched.close()
        for ce in sched.engines.values():
            ce.close()


@pytest.fixture(scope="module")
def served(engine):
    mp = pytest.MonkeyPatch()
    try:
        on = _serve(engine, mp, per_request_sampling=True)
        again = _serve(engine, mp, per_request_sampling=True)
        off = _serve(engine, mp)
    finally:
        mp.undo()
    greedy = engine.generate([list(p) for p in PROMPTS], NEW, ignore_eos=True).tokens
    return on, again, off, greedy


def test_one_engine_no_legacy_path(served):
    (tokens, engines, generates), _, _, _ = served
    assert engines == 1 and generates == 0
    assert all(len(t) == NEW for t in tokens)


def test_greedy_unchanged(served):
    (on, _, _), _, (off, _, _), greedy = served
    for i in (0, 1):
        assert on[i] == off[i] == greedy[i]


def test_top_k_1_is_greedy(served):
    (on, _, _), _, _, greedy = served
    assert CONFIGS[3][:2] == (0.8, 1) and on[3] == greedy[3]


def test_determinism(served):
    (on, _, _), (again, _, _), _, _ = served
    assert on == again


def test_defaults_unchanged(served):
    _, _, (tokens, engines, generates), _ = served
    assert engines == 4 and generates == 2
    assert all(len(t) == NEW for t in tokens)


def test_key_unchanged():
    assert GenRequest([1], 4, 0.7, 40, 0.95, 0.05, 3).key() == (0.7, 40, 0.95, 0.05, 3, False)
    a, b = GenRequest([1], 4, 0.7, 40, 0.95, 0.05, 3), GenRequest([1, 2], 8, 0.0, 0, 1.0, 0.0, 9)
    assert a.engine_key() == b.engine_key() == (False,)
    assert GenRequest([1], 4, ignore_eos=True).engine_key() == (True,)
    c = GenRequest([1], 4, 0.7, frequency_penalty=0.5)
    d = GenRequest([1], 4, 0.0, seed=5, logit_bias={3: 1.0})
    assert c.engine_key() == d.engine_key() == (False, (True, False)) != a.engine_key()
    assert GenRequest([1], 4, n_probs=2).engine_key() == (False, (False, True))


def test_neutral_reset(engine):
    greedy = engine.generate([PROMPTS[1]], NEW, ignore_eos=True).tokens[0]
    ce = ContinuousEngine(engine, max_slots=2, max_new_cap=16, max_prompt=64, steps_per_sync=4,
                          per_request_sampling=True)
    a = ce.submit(PROMPTS[0], NEW, sampling=K.SamplingParams(1.5, 0, 1.0, 0.0), seed=11)
    ce.run()
    assert a.slot is None and len(a.tokens) == NEW
    rows = ce.sampler_rows
    assert rows.temperature.tolist() == [0.0, 0.0] and rows.seed.tolist() == [0, 0] and rows.pos.tolist() == [0, 0]
    assert rows.top_k.tolist() == [0, 0] and rows.top_p.tolist() == [1.0, 1.0] and rows.min_p.tolist() == [0.0, 0.0]
    b = ce.submit(PROMPTS[1], NEW)          # the freed slot 0, now greedy
    ce.run()
    ce.close()
    assert b.tokens == greedy


def test_stream_depends_on_seed_and_own_index_only(engine):
    """A seeded request draws the same tokens alone in slot 0 of a fresh engine and in slot 1 of an
    engine that has already run another request (the CPU path's logits do not depend on the batch)."""
    sp = K.SamplingParams(1.0, 20, 0.95, 0.0)
    alone = ContinuousEngine(engine, max_slots=2, max_new_cap=16, max_prompt=64, steps_per_sync=4,
                             per_request_sampling=True)
    a = alone.submit(PROMPTS[2], NEW, sampling=sp, seed=5)
    alone.run()
    alone.close()
    busy = ContinuousEngine(engine, max_slots=2, max_new_cap=16, max_prompt=64, steps_per_sync=4,
                            per_request_sampling=True)
    busy.submit(PROMPTS[0], 5, sampling=0.9, seed=1)
    busy.run()
    busy.submit(PROMPTS[0], 16, sampling=1.3, seed=2)
    b = busy.submit(PROMPTS[2], NEW, sampling=sp, seed=5)
    busy.run()
    busy.close()
    assert b.tokens == a.tokens
    other = ContinuousEngine(engine, max_slots=2, max_new_cap=16, max_prompt=64, per_request_sampling=True)
    c = other.submit(PROMPTS[2], NEW, sampling=sp, seed=6)
    other.run()
    other.close()
    assert c.tokens != a.tokens           # 8 draws over ~20 candidates each: another seed, another text


def test_reference_sample_rows():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 50, generator=g).to(torch.bfloat16)
    args = ([0.0, 0.7, 0.8, 1.0], [0, 0, 1, 10], [1.0, 1.0, 1.0, 0.9], [0.0, 0.0, 0.0, 0.05], [1, 2, 3, 4])
    out = R.sample_rows(x, *args, [0, 3, 5, 7])
    assert out.dtype == torch.int32 and out[0] == R.sample_greedy(x)[0] and out[2] == R.sample_greedy(x)[2]
    # rows are independent: row 3 alone, at another row index, beside other rows
    alone = R.sample_rows(x[3:4], [1.0], [10], [0.9], [0.05], [4], [7])
    assert int(alone[0]) == int(out[3])
    # K.sample_rows on CPU tensors: the same ids, pos advanced over the width only
    rows = K.SamplerRows(6, "cpu")
    rows.set_rows(range(4), [K.SamplingParams(*v) for v in zip(*args[:4])], args[4])
    rows.pos[:4] = torch.tensor([0, 3, 5, 7], dtype=torch.int32)
    ids = torch.full((6,), -1, dtype=torch.int32)
    K.sample_rows(x, ids, rows, 4)
    assert ids.tolist() == out.tolist() + [-1, -1] and rows.pos.tolist() == [1, 4, 6, 8, 0, 0]
    rows.reset(1)
    assert rows.temperature[1] == 0 and rows.pos[1] == 0 and rows.seed[1] == 0
    rows.set(2, K.SamplingParams(0.5, 3, 0.5, 0.25), seed=0xFFFFFFFF)
    assert rows.seed[2] == -1 and rows.top_k[2] == 3 and rows.min_p[2] == 0.25
    with pytest.raises(ValueError):
        rows.set(0, K.SamplingParams(0.7, 0, 0.0, 0.0))


def test_engine_refusals(engine):
    off = ContinuousEngine(engine, max_slots=2, max_new_cap=8, max_prompt=64)
    assert off.sampler_rows is None
    with pytest.raises(ValueError):
        off.submit(PROMPTS[0], 4, sampling=K.SamplingParams(0.7))
    with pytest.raises(ValueError):
        off.submit(PROMPTS[0], 4, seed=3)
    off.close()


def test_flag_off_never_reaches_sample_rows(engine, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine without per_request_sampling reached sample_rows")
    monkeypatch.setattr(K, "sample_rows", boom)
    monkeypatch.setattr(K, "SamplerRows", boom)
    ce = ContinuousEngine(engine, max_slots=2, max_new_cap=8, max_prompt=64, steps_per_sync=2, temperature=0.7, seed=3)
    r = ce.submit(PROMPTS[0], 4)
    ce.run()
    ce.close()
    assert len(r.tokens) == 4


def test_composes_with_processors_and_logprobs(engine):
    greedy = engine.generate([PROMPTS[0]], 6, ignore_eos=True).tokens[0]
    ce = ContinuousEngine(engine, max_slots=3, max_new_cap=16, max_prompt=64, steps_per_sync=4, processors=True,
                          logprobs=2, per_request_sampling=True)
    ref = ContinuousEngine(engine, max_slots=3, max_new_cap=16, max_prompt=64, steps_per_sync=4, processors=True,
                           logprobs=2)
    ban = {greedy[0]: False}
    a = ce.submit(PROMPTS[0], 6, sampling=K.SamplingParams(0.8, 1), seed=9, logit_bias=ban, logprobs=2)
    b = ce.submit(PROMPTS[0], 6)
    c = ref.submit(PROMPTS[0], 6, logit_bias=ban, logprobs=2)
    ce.run()
    ref.run()
    ce.close()
    ref.close()
    assert b.tokens == greedy and a.tokens == c.tokens and a.tokens[0] != greedy[0]
    assert a.logprobs == c.logprobs and len(a.logprobs) == 6


def test_config_reaches_the_scheduler(monkeypatch):
    monkeypatch.setenv("LLM_PER_REQUEST_SAMPLING", "1")
    cfg = load_adapter_config("llm_backend", driver="hip").driver_config
    assert cfg["per_request_sampling"] is True
    cfg.update({"model": "tiny", "device": "cpu", "max_new_tokens": 8, "kv_cache_tokens": 1 << 12, "max_batch": 4})
    app, _ = build_from_config(cfg, max_prompt=64, max_new_cap=16)
    try:
        assert app.state.scheduler.per_request_sampling is True
    finally:
        app.state.scheduler.close()
    monkeypatch.delenv("LLM_PER_REQUEST_SAMPLING")
    assert load_adapter_config("llm_backend", driver="hip").driver_config["per_request_sampling"] is False


def test_tensor_parallel_is_refused():
    cfg = get_config("tiny")
    m = DecoderModel(DecoderWeights.random(cfg, "cpu", seed=0, tp_rank=0, tp_size=2))
    kv = PagedKVCache(cfg.layers, 16, m.w.kv_heads, cfg.head_dim, "cpu")
    eng = LLMEngine(m, kv)
    with pytest.raises(ValueError, match="TP"):
        ContinuousEngine(eng, max_slots=2, max_new_cap=8, max_prompt=64, per_request_sampling=True)
    ContinuousEngine(eng, max_slots=2, max_new_cap=8, max_prompt=64).close()      # the flag alone is refused
