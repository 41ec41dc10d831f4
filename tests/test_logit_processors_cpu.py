"""Logit processors (logit_bias, repeat / frequency / presence penalties) and token
log-probabilities: the fp32 oracles (ops/reference.py) against hand-checked values, the window
rules, the engines on the CPU path and the HTTP server's four response shapes and refusals."""
from __future__ import annotations

import math

import pytest
import torch
from fastapi.testclient import TestClient

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.ops import reference as R
from copilot_for_consensus_amd.runtime.continuous import ContinuousEngine
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache
from copilot_for_consensus_amd.serving import build_from_config
from copilot_for_consensus_amd.serving.llm_server import GenRequest

BF = torch.bfloat16


# ----------------------------------------------------------------------------- hand-checked cases

def test_hand_checked_processors():
    x = torch.tensor([[2, -1, 0.5, 3, 0, -2, 1, 4]], dtype=BF)
    out = R.logit_processors(x, [[3, 1, 3, 4]], [64], [2.0], [0.25], [0.5], [[(7, -100.0), (2, 1.5)]])
    assert torch.equal(out, torch.tensor([[2, -2.75, 2, 0.5, -0.75, -2, 1, -96]], dtype=BF))
    assert int(R.sample_greedy(x)[0]) == 7 and int(R.sample_greedy(out)[0]) == 0    # tie at 2.0: lowest id


def test_hand_checked_logprobs_equal_logits():
    lp, ids, top = R.token_logprobs(torch.zeros(1, 4, dtype=BF), torch.tensor([3], dtype=torch.int32), 2)
    assert torch.equal(lp, torch.tensor([-1.3862944])) and torch.equal(top, torch.tensor([[-1.3862944] * 2]))
    assert ids.tolist() == [[0, 1]]


def test_hand_checked_logprobs_1_2_3():
    """The issue states the values to 8 digits, cut off, not rounded (-0.40760596 is written
    -0.4076059): the comparison is to one unit of the last digit stated, 1e-7."""
    want = torch.tensor([-2.4076059, -1.4076059, -0.4076059])
    for c in range(3):
        lp, ids, top = R.token_logprobs(torch.tensor([[1.0, 2.0, 3.0]], dtype=BF), torch.tensor([c], dtype=torch.int32), 3)
        assert abs(float(lp[0]) - float(want[c])) <= 1e-7
        assert ids.tolist() == [[2, 1, 0]] and float((top[0] - want.flip(0)).abs().max()) <= 1e-7


def test_logprobs_nan_ranks_as_neg_inf():
    x = torch.tensor([[0.0, float("nan"), 1.0, float("-inf")]], dtype=BF)
    lp, ids, top = R.token_logprobs(x, torch.tensor([2], dtype=torch.int32), 4)
    assert ids.tolist() == [[2, 0, 1, 3]] and top[0, 2:].tolist() == [-math.inf, -math.inf]
    assert abs(float(lp[0]) + math.log(1 + math.exp(-1))) < 1e-6


# ----------------------------------------------------------------------------- window rules

def _pen(history, last_n, V=10, tail=None):
    x = torch.ones(1, V, dtype=BF)
    return R.logit_processors(x, [list(tail or []) + history], [last_n], [1.0], [1.0], [0.0])[0].float().tolist()


def test_window_rules():
    assert _pen([5, 5, 6, 7], 0) == [1.0] * 10                                     # last_n = 0: no-op
    two = _pen([5, 5, 6, 7], 2)
    assert [i for i, v in enumerate(two) if v != 1.0] == [6, 7] and two[6] == 0.0
    alln = _pen([5, 5, 6, 7], -1)
    assert alln[5] == -1.0 and alln[6] == 0.0 and alln[7] == 0.0                   # everything kept
    assert R.penalty_window(list(range(3000)), -1, 1024) == list(range(3000 - 1024, 3000))
    assert R.penalty_window(list(range(3000)), 5000, 1024) == list(range(3000 - 1024, 3000))


def test_prompt_tail_used_only_when_supplied():
    """Through the op and its state object: the same generated tokens with and without a tail."""
    V = 12
    toks = torch.tensor([[6, 7, 0, 0]], dtype=torch.int32)
    step = torch.tensor([2], dtype=torch.int32)
    outs = {}
    for name, p in (("tail", K.LogitParams.make(frequency_penalty=1.0, repeat_last_n=4)),
                    ("no_tail", K.LogitParams.make(frequency_penalty=1.0, repeat_last_n=4, penalize_prompt=False))):
        st = K.LogitState(1, "cpu")
        st.set_rows([0], [p], [[1, 2, 3, 4, 5]])
        x = torch.ones(1, V, dtype=BF)
        K.logit_processors(x, K.LogitCtx(st, tokens=toks, step=step))
        outs[name] = [i for i, v in enumerate(x[0].tolist()) if v != 1.0]
    assert outs["no_tail"] == [6, 7]
    assert outs["tail"] == [4, 5, 6, 7]            # window of 4 over [2, 3, 4, 5] ++ [6, 7]


def test_neutral_row_keeps_every_bit():
    x = torch.randn(2, 64).to(BF)
    x[0, 3] = float("nan")
    st = K.LogitState(2, "cpu")
    st.set_rows([0, 1], [K.LogitParams(), K.LogitParams.make(repeat_last_n=0, frequency_penalty=3.0)], [[1, 2], [3]])
    y = x.clone()
    K.logit_processors(y, K.LogitCtx(st, tokens=torch.tensor([[1], [3]], dtype=torch.int32),
                                     gen=torch.tensor([1, 1], dtype=torch.int32)))
    assert torch.equal(y.view(torch.int16), x.view(torch.int16))


def test_argument_checks():
    with pytest.raises(ValueError):
        K.LogitParams.make(repeat_penalty=0.0)
    with pytest.raises(ValueError):
        K.LogitParams.make(logit_bias={600: 1.0}, vocab=512)
    with pytest.raises(ValueError):
        K.LogitParams.make(logit_bias={i: 1.0 for i in range(K.LOGIT_BIAS_MAX + 1)})
    assert K.LogitParams.make(logit_bias=[(3, 1.0), (3, False)]).logit_bias == ((3, -math.inf),)   # last wins
    st = K.LogitState(1, "cpu", rec_cap=2, top_n=20)
    with pytest.raises(ValueError):
        K.token_logprobs(torch.zeros(1, 8, dtype=BF), torch.zeros(1, dtype=torch.int32), K.LogitCtx(st), 21)
    with pytest.raises(TypeError):
        K.token_logprobs(torch.zeros(1, 8, dtype=BF), torch.zeros(1, dtype=torch.int64), K.LogitCtx(st), 1)
    with pytest.raises(ValueError):
        K.LogitState(1, "cpu", window=K.PENALTY_WINDOW_MAX + 1)
    assert K.SamplingParams(0.7, 40, 0.95, 0.05) == K.SamplingParams(0.7, 40, 0.95, 0.05, False, -1)


# ----------------------------------------------------------------------------- engines (CPU path)

@pytest.fixture(scope="module")
def engine():
    cfg = get_config("tiny")
    m = DecoderModel(DecoderWeights.random(cfg, "cpu", seed=0))
    kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, cfg.head_dim, "cpu")
    return LLMEngine(m, kv)


PROMPTS = [[1, 2, 3, 4], [1, 5, 6]]


def test_engine_frequency_penalty_gives_distinct_tokens(engine):
    V = engine.cfg.vocab_size
    # bias three tokens far above the rest: unpenalised the model would repeat the best of them
    bias = {10: 60.0, 11: 59.0, 12: 58.0}
    plain = engine.generate(PROMPTS, 3, ignore_eos=True, logit_bias=bias).tokens
    assert all(len(set(t)) == 1 for t in plain)
    res = engine.generate(PROMPTS, 3, ignore_eos=True, logit_bias=bias, frequency_penalty=100.0,
                          penalize_prompt=False).tokens
    assert all(sorted(t) == [10, 11, 12] for t in res)
    long = engine.generate(PROMPTS, 24, ignore_eos=True, frequency_penalty=100.0).tokens
    assert 24 < V and all(len(set(t)) == len(t) == 24 for t in long)


def test_engine_logit_bias_and_neutral(engine):
    assert engine.generate(PROMPTS, 6, ignore_eos=True, logit_bias={7: 100.0}).tokens == [[7] * 6] * 2
    plain = engine.generate(PROMPTS, 8, ignore_eos=True)
    assert plain.logprobs is None
    neutral = engine.generate(PROMPTS, 8, ignore_eos=True, temperature=K.SamplingParams(processors=True))
    assert neutral.tokens == plain.tokens
    banned = engine.generate(PROMPTS, 8, ignore_eos=True, logit_bias={plain.tokens[0][0]: False}).tokens
    assert plain.tokens[0][0] not in banned[0]


def test_plain_requests_never_reach_the_new_ops(engine, monkeypatch):
    """With neither feature on, the step's calls are the old ones: logits -> K.sample, no state."""
    def boom(*a, **k):
        raise AssertionError("a plain request reached a logit op")
    monkeypatch.setattr(K, "logit_processors", boom)
    monkeypatch.setattr(K, "token_logprobs", boom)
    monkeypatch.setattr(K, "LogitState", boom)
    calls = []
    sample = K.sample
    monkeypatch.setattr(K, "sample", lambda *a, **k: calls.append(len(a) + len(k)) or sample(*a, **k))
    res = engine.generate(PROMPTS, 4, ignore_eos=True, repeat_penalty=1.0, repeat_last_n=64, presence_penalty=0.0,
                          frequency_penalty=0.0, logit_bias={}, logprobs=None)
    assert [len(t) for t in res.tokens] == [4, 4] and calls == [5] * 4      # 1 prefill + 3 decode steps
    ce = ContinuousEngine(engine, max_slots=2, max_new_cap=8, max_prompt=64, steps_per_sync=2)
    r = ce.submit(PROMPTS[0], 4)
    ce.run()
    ce.close()
    assert r.tokens == res.tokens[0] and ce.logit_state is None


def test_engine_logprobs(engine):
    plain = engine.generate(PROMPTS, 6, ignore_eos=True)
    res = engine.generate(PROMPTS, 6, ignore_eos=True, logprobs=3)
    assert res.tokens == plain.tokens
    for toks, recs in zip(res.tokens, res.logprobs):
        assert len(recs) == len(toks)
        for t, (lp, top) in zip(toks, recs):
            assert len(top) == 3 and top[0] == (t, lp) and lp <= 0
            assert all(a[1] >= b[1] for a, b in zip(top, top[1:]))
    # the records are of the raw logits: a bias moves the choice, not the distribution
    both = engine.generate(PROMPTS, 1, ignore_eos=True, logprobs=1, logit_bias={7: 100.0})
    assert both.tokens == [[7], [7]]
    assert [r[0][1][0] for r in both.logprobs] == [r[0][1][0] for r in res.logprobs]
    assert all(r[0][0] < r[0][1][0][1] for r in both.logprobs)
    with pytest.raises(ValueError):
        engine.generate(PROMPTS, 1, logprobs=21)


def test_continuous_engine_per_request_parameters(engine):
    plain = engine.generate(PROMPTS, 10, ignore_eos=True).tokens
    ce = ContinuousEngine(engine, max_slots=3, max_new_cap=16, max_prompt=64, steps_per_sync=4, processors=True,
                          logprobs=2)
    a = ce.submit(PROMPTS[0], 10)
    b = ce.submit(PROMPTS[0], 10, frequency_penalty=100.0, logprobs=2)
    c = ce.submit(PROMPTS[1], 10, logit_bias={9: 100.0}, logprobs=0)
    ce.run()
    assert a.tokens == plain[0] and a.logprobs is None
    assert len(set(b.tokens)) == len(b.tokens) == 10 and len(b.logprobs) == 10
    assert c.tokens == [9] * 10 and [len(r[1]) for r in c.logprobs] == [0] * 10
    d = ce.submit(PROMPTS[1], 10)          # a freed slot: nothing of its previous occupant remains
    ce.run()
    assert d.tokens == plain[1]
    with pytest.raises(ValueError):
        ce.submit(PROMPTS[0], 4, logprobs=3)
    ce.close()
    off = ContinuousEngine(engine, max_slots=2, max_new_cap=8, max_prompt=64)
    with pytest.raises(ValueError):
        off.submit(PROMPTS[0], 4, presence_penalty=1.0)
    off.close()


# ----------------------------------------------------------------------------- server

def test_request_key():
    plain = GenRequest([1, 2], 4, 0.7, 40, 0.95, 0.05, 3)
    assert plain.key() == (0.7, 40, 0.95, 0.05, 3, False)             # today's key
    assert GenRequest([1], 4).key() == (0.0, 0, 1.0, 0.0, 0, False)
    a = GenRequest([1], 4, frequency_penalty=0.5, repeat_last_n=-1)
    b = GenRequest([1], 4, frequency_penalty=1.5, presence_penalty=0.25, logit_bias={3: 1.0})
    assert a.key() == b.key() != GenRequest([1], 4).key()
    assert GenRequest([1], 4, n_probs=2).key() == GenRequest([1], 4, n_probs=5).key() != a.key()


@pytest.fixture(scope="module")
def client():
    app, s = build_from_config({"model": "tiny", "device": "cpu", "max_new_tokens": 16, "kv_cache_tokens": 1 << 15,
                                "max_batch": 16}, max_prompt=256, max_new_cap=64)
    with TestClient(app) as c:
        yield c, s
    app.state.scheduler.close()


PROMPT = "Summarize this email thread: the working group agreed on the draft."


def test_server_llamacpp_shape(client):
    c, s = client
    base = {"prompt": PROMPT, "n_predict": 8, "temperature": 0.0, "ignore_eos": True}
    plain = c.post("/completion", json=base).json()
    assert "completion_probabilities" not in plain
    assert set(plain) == {"content", "model", "stop", "tokens_predicted", "tokens_evaluated", "stopped_eos",
                          "stopped_word", "stopped_limit", "stopping_word", "truncated", "timings"}
    r = c.post("/completion", json={**base, "n_probs": 3}).json()
    assert set(r) == set(plain) | {"completion_probabilities"} and r["content"] == plain["content"]
    probs = r["completion_probabilities"]
    assert len(probs) == r["tokens_predicted"] == 8
    for e in probs:
        assert set(e) == {"id", "token", "bytes", "logprob", "top_logprobs"} and len(e["top_logprobs"]) == 3
        assert e["top_logprobs"][0]["id"] == e["id"] and e["top_logprobs"][0]["logprob"] == e["logprob"]
        assert bytes(e["bytes"]).decode() == e["token"]
    assert "".join(e["token"] for e in probs) == r["content"]
    assert len(c.post("/completion", json={**base, "n_probs": 50}).json()
               ["completion_probabilities"][0]["top_logprobs"]) == 20                      # clamped
    # the processors reach the engine: a bias of +100 emits that token only; false bans a token
    tok = s.tokenizer.encode("draft")[-1]
    forced = c.post("/completion", json={**base, "logit_bias": [[tok, 100]], "n_probs": 1}).json()
    assert {e["id"] for e in forced["completion_probabilities"]} == {tok}
    first = probs[0]["id"]
    ban = c.post("/completion", json={**base, "logit_bias": [[first, False]], "n_probs": 1}).json()
    assert first not in {e["id"] for e in ban["completion_probabilities"]}
    pen = c.post("/completion", json={**base, "n_predict": 24, "frequency_penalty": 100.0, "repeat_last_n": -1,
                                      "n_probs": 1}).json()
    ids = [e["id"] for e in pen["completion_probabilities"]]
    assert len(ids) == 24 and len(set(ids)) == 24 and not set(ids) & set(s.tokenizer.encode(PROMPT))


def test_server_entries_stop_at_the_cut(client):
    c, _ = client
    base = {"prompt": "The quick brown fox", "n_predict": 16, "temperature": 0.0, "n_probs": 1}
    full = c.post("/completion", json=base).json()
    text = full["content"]
    if len(text) > 4:
        word = text[2:4]
        cut = c.post("/completion", json={**base, "stop": [word]}).json()
        assert cut["stopped_word"] and "".join(e["token"] for e in cut["completion_probabilities"]) == cut["content"]
        assert len(cut["completion_probabilities"]) < len(full["completion_probabilities"])


def test_server_ollama_shape(client):
    c, _ = client
    body = {"prompt": PROMPT, "stream": False, "options": {"num_predict": 6, "temperature": 0}}
    plain = c.post("/api/generate", json=body).json()
    assert "logprobs" not in plain
    r = c.post("/api/generate", json={**body, "logprobs": True, "top_logprobs": 2}).json()
    assert set(r) == set(plain) | {"logprobs"} and r["response"] == plain["response"]
    assert len(r["logprobs"]) == r["eval_count"]
    for e in r["logprobs"]:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and len(e["top_logprobs"]) == 2
        assert e["top_logprobs"][0]["logprob"] == e["logprob"] and e["top_logprobs"][0]["token"] is not None
    ch = c.post("/api/chat", json={"messages": [{"role": "user", "content": PROMPT}], "stream": False,
                                   "logprobs": True, "top_logprobs": 1,
                                   "options": {"num_predict": 5, "temperature": 0, "repeat_penalty": 1.3,
                                               "repeat_last_n": 32, "presence_penalty": 0.5}}).json()
    assert len(ch["logprobs"]) == ch["eval_count"] and ch["message"]["role"] == "assistant"
    assert all(e["top_logprobs"][0]["logprob"] >= e["logprob"] for e in ch["logprobs"])    # penalised choice


def test_server_openai_shapes(client):
    c, _ = client
    body = {"prompt": PROMPT, "max_tokens": 6, "temperature": 0}
    plain = c.post("/v1/completions", json=body).json()
    assert plain["choices"][0]["logprobs"] is None and set(plain["choices"][0]) == {"text", "index", "logprobs",
                                                                                   "finish_reason"}
    r = c.post("/v1/completions", json={**body, "logprobs": 2, "presence_penalty": 0.0}).json()
    assert set(r) == set(plain) and r["choices"][0]["text"] == plain["choices"][0]["text"]
    lp = r["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    n = r["usage"]["completion_tokens"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == n
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert max(top.values()) == v and v <= 0
    assert "".join(lp["tokens"]) == r["choices"][0]["text"] and lp["text_offset"][0] == 0

    chat = {"messages": [{"role": "user", "content": PROMPT}], "max_tokens": 5, "temperature": 0}
    cp = c.post("/v1/chat/completions", json=chat).json()
    assert set(cp["choices"][0]) == {"index", "message", "finish_reason"}
    cr = c.post("/v1/chat/completions", json={**chat, "logprobs": True, "top_logprobs": 20,
                                              "frequency_penalty": 0.0, "logit_bias": {}}).json()
    assert cr["choices"][0]["message"] == cp["choices"][0]["message"]
    content = cr["choices"][0]["logprobs"]["content"]
    assert len(content) == cr["usage"]["completion_tokens"]
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and len(e["top_logprobs"]) == 20
        assert e["top_logprobs"][0]["logprob"] == e["logprob"] and e["top_logprobs"][0]["token"] == e["token"]
    # OpenAI's window is the generated text only: a prompt token is not penalised on the first step
    pen = c.post("/v1/chat/completions", json={**chat, "frequency_penalty": 2.0, "logit_bias": {"7": 100},
                                               "logprobs": True}).json()
    assert pen["usage"]["completion_tokens"] == 5 and len(pen["choices"][0]["logprobs"]["content"]) == 5


@pytest.mark.parametrize("route,body,field", [
    ("/completion", {"prompt": "x", "repeat_penalty": 0}, "repeat_penalty"),
    ("/completion", {"prompt": "x", "repeat_penalty": -1.5}, "repeat_penalty"),
    ("/api/generate", {"prompt": "x", "stream": False, "options": {"repeat_penalty": 0}}, "repeat_penalty"),
    ("/completion", {"prompt": "x", "logit_bias": [[512, 1.0]]}, "logit_bias"),
    ("/completion", {"prompt": "x", "logit_bias": [[-1, 1.0]]}, "logit_bias"),
    ("/v1/completions", {"prompt": "x", "logit_bias": {"100000": 1}}, "logit_bias"),
    ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "logit_bias": {"999": 1}}, "logit_bias"),
    ("/completion", {"prompt": "x", "logit_bias": [[i % 512, 1.0] for i in range(513)]}, "logit_bias: more than 512"),
    ("/v1/completions", {"prompt": "x", "logit_bias": {f"{i:04d}" if i < 512 else "0": 1 for i in range(513)}},
     "logit_bias: more than 512"),
    ("/completion", {"prompt": "x", "logit_bias": [[i, 0.0] for i in range(512)]}, None),
    ("/v1/completions", {"prompt": "x", "logprobs": 6}, "logprobs"),
    ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "logprobs": True, "top_logprobs": 21},
     "top_logprobs"),
    ("/completion", {"prompt": "x", "stream": True, "n_probs": 2}, "stream"),
    ("/api/generate", {"prompt": "x", "logprobs": True}, "stream"),
    ("/api/chat", {"messages": [{"role": "user", "content": "x"}], "logprobs": True}, "stream"),
    ("/v1/completions", {"prompt": "x", "stream": True, "logprobs": 1}, "stream"),
    ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "stream": True, "logprobs": True},
     "stream"),
])
def test_server_refusals(client, route, body, field):
    c, _ = client
    resp = c.post(route, json={"n_predict": 2, "max_tokens": 2, **body})
    if field is None:              # 512 entries are within the cap
        assert resp.status_code == 200
        return
    assert resp.status_code == 400 and field in resp.json()["detail"]
