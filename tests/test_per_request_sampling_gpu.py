"""The continuous engine with ``per_request_sampling``: greedy, ``top_k = 1`` and sampled requests
in one captured decode step ("small" preset, graphs on), against an engine without the option."""
from __future__ import annotations

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime.continuous import ContinuousEngine
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
NEW = 16


@pytest.fixture(scope="module")
def model():
    return DecoderModel(DecoderWeights.random(get_config("small"), "cuda", seed=5))


@pytest.fixture()
def eng(model):
    return _engine(model)


def _engine(model):
    """A fresh KV cache and prefix cache per engine under comparison: every run then starts from
    the same state (zeroed blocks, no cached prefixes), as the runs it is compared with."""
    cfg = model.cfg
    kv = PagedKVCache(cfg.layers, 96, cfg.kv_heads, cfg.head_dim, "cuda")
    return LLMEngine(model, kv, max_prefill_tokens=256, use_graph=True)


def _prompts(vocab):
    g = torch.Generator().manual_seed(4)
    return [[1] + torch.randint(3, vocab, (n,), generator=g).tolist() for n in (9, 33, 17, 5, 21, 12)]


# per prompt: greedy, top_k = 1, sampled (untruncated), sampled (truncated), greedy, top_k = 1
MIX = [(K.SamplingParams(0.0), 0), (K.SamplingParams(0.8, top_k=1), 3), (K.SamplingParams(0.9), 4),
       (K.SamplingParams(1.0, top_k=40, top_p=0.95, min_p=0.05), 5), (K.SamplingParams(-1.0, top_k=7), 6),
       (K.SamplingParams(1.4, top_k=1, top_p=0.3), 7)]


def _run(eng, per_request, mix=None, **kw):
    ce = ContinuousEngine(eng, max_slots=8, max_new_cap=NEW, max_prompt=64, steps_per_sync=5, min_admit=6,
                          per_request_sampling=per_request, **kw)
    assert ce.use_graph
    prompts = _prompts(eng.cfg.vocab_size)
    if per_request:
        reqs = [ce.submit(p, NEW, sampling=sp, seed=sd) for p, (sp, sd) in zip(prompts, mix or MIX)]
    else:
        reqs = [ce.submit(p, NEW) for p in prompts]
    ce.run()
    assert ce.graphs and set(ce.graphs) == {8}, "one captured step at the width of six occupied slots"
    ce.close()
    return [r.tokens for r in reqs]


@pytest.fixture(scope="module")
def greedy(model):
    return _run(_engine(model), False)


@pytest.fixture(scope="module")
def mixed(model):
    return _run(_engine(model), True)


def test_mixed_batch_against_a_greedy_engine(greedy, mixed):
    assert all(len(t) == NEW for t in greedy + mixed)
    for i in (0, 1, 4, 5):
        assert mixed[i] == greedy[i]
    vocab = get_config("small").vocab_size
    assert all(0 <= t < vocab for row in mixed for t in row)
    assert mixed[2] != greedy[2]            # T = 0.9 over a random model's 32000 logits: not the argmax text


def test_seeded_rows_are_deterministic(model, eng, mixed):
    again = _run(_engine(model), True)
    assert again == mixed
    # the seeded rows again, in other slots and beside other requests: the draws depend on the
    # request's seed and its own token index (the logits on the batch width, which is the same)
    order = [3, 2, 1, 0, 5, 4]
    ce = ContinuousEngine(eng, max_slots=8, max_new_cap=NEW, max_prompt=64, steps_per_sync=3, min_admit=6,
                          per_request_sampling=True)
    prompts = _prompts(eng.cfg.vocab_size)
    eng.lpt, lpt = False, eng.lpt            # keep the submission order as the slot order
    try:
        reqs = {i: ce.submit(prompts[i], NEW, sampling=MIX[i][0], seed=MIX[i][1]) for i in order}
        ce.run()
    finally:
        eng.lpt = lpt
        ce.close()
    assert reqs[3].tokens == mixed[3] and reqs[2].tokens == mixed[2]


def test_composition_with_logit_processors(model, eng, greedy):
    prompts = _prompts(eng.cfg.vocab_size)
    ban = {greedy[0][0]: False}
    ref = ContinuousEngine(_engine(model), max_slots=8, max_new_cap=NEW, max_prompt=64, steps_per_sync=5, min_admit=2,
                           processors=True)
    want = ref.submit(prompts[0], NEW, logit_bias=ban)
    ref.submit(prompts[1], NEW)
    ref.run()
    ref.close()
    ce = ContinuousEngine(eng, max_slots=8, max_new_cap=NEW, max_prompt=64, steps_per_sync=5, min_admit=2,
                          processors=True, per_request_sampling=True)
    got = ce.submit(prompts[0], NEW, sampling=K.SamplingParams(0.8, top_k=1), seed=9, logit_bias=ban)
    other = ce.submit(prompts[1], NEW, sampling=K.SamplingParams(1.2), seed=1)
    ce.run()
    assert ce.graphs
    ce.close()
    assert want.tokens[0] != greedy[0][0] and got.tokens == want.tokens
    assert len(other.tokens) == NEW
