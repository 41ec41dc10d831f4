"""The two HIP kernels of csrc/kernels/logits.hip against their fp32 oracles, the placement of
the log-probability records, and both engines with the kernels inside the captured decode step."""
from __future__ import annotations

import math

import pytest
import torch

from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config
from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime.continuous import ContinuousEngine
from copilot_for_consensus_amd.runtime.engine import LLMEngine
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NEG = -math.inf


def _ordered(x: torch.Tensor) -> torch.Tensor:
    """bf16 bits as integers that step by one per representable value."""
    b = x.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


# ----------------------------------------------------------------------------- processors

def _rows(V, g):
    """Two batches of three rows: (prompt tail, generated, last_n, repeat, frequency, presence, bias)."""
    def toks(n, hi):
        return torch.randint(0, hi, (n,), generator=g).tolist()

    def bias(n, ninf_every=0):
        ids = torch.randperm(V, generator=g)[:n].tolist()
        vals = (torch.randn(n, generator=g) * 4).tolist()
        if ninf_every:
            vals = [NEG if i % ninf_every == 0 else v for i, v in enumerate(vals)]
        return dict(zip(ids, vals))

    a = [([], [], 64, 1.3, 0.7, 0.4, {}),                                      # empty window: untouched
         ([], toks(1, V), 64, 1.3, 0.7, 0.4, bias(1)),                         # window 1, one bias entry
         (toks(40, 30), toks(24, 30), 64, 1.1, 0.25, 0.0, bias(512, 7))]       # window 64, repeats, 512 entries
    full = toks(700, 60) + [V - 1, 0, V - 1]
    b = [(full, toks(321, 60), -1, 1.7, 0.3, 1.1, bias(512, 5)),               # window 1024 = 703 + 321
         (toks(50, 30), toks(14, 30), 64, 1.0, 0.0, 0.0, {}),                  # neutral
         (toks(100, 30), toks(30, 30), 64, 0.8, 0.0, 0.5, {})]                 # window 64 of 130, no bias
    return [a, b]


@pytest.mark.parametrize("V", [1003, 32000])
@pytest.mark.parametrize("mode", ["gen", "step"])
def test_processors_match_oracle(V, mode):
    g = torch.Generator().manual_seed(V)
    for batch in _rows(V, g):
        if mode == "step":            # one counter for the batch: the same generated count per row
            n = min(len(r[1]) for r in batch)
            batch = [(r[0], r[1][:n], *r[2:]) for r in batch]
        B, cap = len(batch), 400
        logits = (torch.randn(B, V, generator=g) * 3).to(BF)
        logits[:, 5] = NEG
        params = [K.LogitParams.make(rep, n, pres, freq, bias, vocab=V) for _, _, n, rep, freq, pres, bias in batch]
        tokens = torch.zeros(B, cap, dtype=torch.int32)
        for b, r in enumerate(batch):
            tokens[b, :len(r[1])] = torch.tensor(r[1], dtype=torch.int32)
        tokens[:, cap - 1] = 3                                  # past every count: never read
        gen = torch.tensor([len(r[1]) for r in batch], dtype=torch.int32)
        count = dict(gen=gen) if mode == "gen" else dict(step=gen[:1].clone())
        got = {}
        for dev in ("cpu", "cuda"):
            st = K.LogitState(B, dev)
            st.set_rows(range(B), params, [r[0] for r in batch])     # the tail: the end of each row's "prompt"
            x = logits.clone().to(dev)
            K.logit_processors(x, K.LogitCtx(st, tokens=tokens.to(dev), **{k: v.to(dev) for k, v in count.items()}))
            got[dev] = x.cpu()
        want, have = got["cpu"], got["cuda"]
        touched = torch.zeros(B, V, dtype=torch.bool)
        for b, (tail, gen_t, n, rep, freq, pres, bias) in enumerate(batch):
            w = (tail + gen_t)[-(1024 if n < 0 else n):] if params[b].penalised else []
            if w:
                touched[b, torch.tensor(w, dtype=torch.long)] = True
            for i in bias:
                touched[b, i] = True
        assert torch.equal(have.view(torch.int16)[~touched], logits.view(torch.int16)[~touched])   # bits kept
        assert torch.equal(want.view(torch.int16)[~touched], logits.view(torch.int16)[~touched])
        fin = torch.isfinite(want.float())
        assert torch.equal(torch.isfinite(have.float()), fin) and torch.equal(have[~fin].float(), want[~fin].float())
        ulp = (_ordered(have) - _ordered(want)).abs()[fin]
        assert int(ulp.max()) <= 1, int(ulp.max())
        assert int(touched.sum()) > 0


def test_processors_prompt_tail_window_split():
    """A prompt longer than the window keeps its last 1024 tokens; last_n = -1 then looks back
    over 1024 tokens of tail ++ generated."""
    st = K.LogitState(1, "cuda")
    p = K.LogitParams.make(frequency_penalty=1.0, repeat_last_n=-1)
    prompt = list(range(100, 1500))                       # longer than the window: its last 1024 are kept
    st.set_rows([0], [p], [prompt])
    assert int(st.tail_len[0]) == 1024 and st.prompt_tail[0, 0].item() == 1500 - 1024
    x = torch.zeros(1, 2000, dtype=BF, device="cuda")
    toks = torch.tensor([[7, 8, 9, 0]], dtype=torch.int32, device="cuda")
    K.logit_processors(x, K.LogitCtx(st, tokens=toks, gen=torch.tensor([3], dtype=torch.int32, device="cuda")))
    hit = (x[0] != 0).nonzero().flatten().tolist()
    assert hit == [7, 8, 9] + list(range(1500 - 1021, 1500))      # 3 generated + the newest 1021 of the tail


def test_processors_hand_checked_bit_exact_and_done_rows():
    x = torch.tensor([[2, -1, 0.5, 3, 0, -2, 1, 4]] * 2, dtype=BF, device="cuda")
    st = K.LogitState(2, "cuda")
    p = K.LogitParams.make(2.0, 64, 0.5, 0.25, {7: -100, 2: 1.5}, vocab=8)
    st.set_rows([0, 1], [p, p], [[], []])
    toks = torch.tensor([[3, 1, 3, 4, 0]] * 2, dtype=torch.int32, device="cuda")
    done = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    K.logit_processors(x, K.LogitCtx(st, tokens=toks, gen=torch.tensor([4, 4], dtype=torch.int32, device="cuda"),
                                     done=done))
    assert torch.equal(x[0].cpu(), torch.tensor([2, -2.75, 2, 0.5, -0.75, -2, 1, -96], dtype=BF))
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    K.sample(x, out)
    assert out.tolist()[0] == 0                          # the tie at 2.0 goes to the lower id
    assert toks.cpu().tolist() == [[3, 1, 3, 4, 0]] * 2 and done.tolist() == [0, 1]    # nothing else written


# ----------------------------------------------------------------------------- log-probabilities

def _logprob_rows(V, g):
    normal = torch.randn(V, generator=g) * 3
    ties = (torch.randn(V, generator=g) * 2).round() / 2                  # ~25 distinct values
    holes = torch.randn(V, generator=g) * 3
    holes[torch.randperm(V, generator=g)[:V // 3]] = NEG
    holes[V // 2] = float("nan")
    holes[1] = float("nan")
    equal = torch.full((V,), 1.5)
    top_ties = torch.randn(V, generator=g)
    top_ties[torch.randperm(V, generator=g)[:min(5000, V // 2)]] = 6.0     # a long run of ties at the top
    ramp = torch.linspace(8, -8, V)                                        # sorted: neighbours share a thread
    return [torch.stack([normal, ties, holes]).to(BF), torch.stack([equal, top_ties, ramp]).to(BF)]


def _check_logprobs(x, N, chosen):
    B, V = x.shape
    clean = torch.nan_to_num(x.float(), nan=NEG, posinf=math.inf, neginf=NEG)
    ref64 = torch.log_softmax(clean.double(), -1)
    cpu32 = torch.log_softmax(clean, -1).double()
    ok = torch.isfinite(ref64)
    cpu_err = float((cpu32 - ref64)[ok].abs().max())
    bound = max(8 * cpu_err, 1e-5)
    st = K.LogitState(B, "cuda", rec_cap=1, top_n=N)
    K.token_logprobs(x.cuda(), chosen.cuda(), K.LogitCtx(st), N)
    lp, ids, top = st.lp[:, 0].cpu().double(), st.top_ids[:, 0, :N].cpu(), st.top_lp[:, 0, :N].cpu().double()
    want_lp = ref64.gather(1, chosen.long().view(B, 1))[:, 0]
    _, order = torch.sort(clean, dim=-1, descending=True, stable=True)
    k = min(N, V)
    assert torch.equal(ids[:, :k].long(), order[:, :k]), (ids[:, :k], order[:, :k])
    want_top = ref64.gather(1, order[:, :k])
    err = 0.0
    for got, want in ((lp, want_lp), (top[:, :k].reshape(-1), want_top.reshape(-1))):
        f = torch.isfinite(want)
        assert torch.equal(got[~f], want[~f])
        if f.any():
            err = max(err, float((got[f] - want[f]).abs().max()))
    print(f"logprobs V={V} N={N}: worst |error| vs float64 {err:.3e}, CPU fp32 {cpu_err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("V", [1003, 32000])
@pytest.mark.parametrize("N", [0, 1, 20])
def test_logprobs_match_float64(V, N):
    g = torch.Generator().manual_seed(7 * V + N)
    for x in _logprob_rows(V, g):
        chosen = torch.randint(0, V, (3,), generator=g).to(torch.int32)
        chosen[0] = int(x[0].float().argmax())
        _check_logprobs(x, N, chosen)
    holes = _logprob_rows(V, g)[0]
    masked = int((holes[2].float() == NEG).nonzero()[0])
    _check_logprobs(holes, N, torch.tensor([0, 0, masked], dtype=torch.int32))     # a masked token was "chosen"


def test_logprobs_few_threads_hold_the_largest():
    """A row whose largest logits all sit in the 16-byte vectors of 19 of the 1024 threads: the
    lower bound taken from the threads' maxima admits more candidates than the kernel's list
    holds, so it selects the exact 20th key over the row instead.  That needs a row this long."""
    V = 128256
    idx = torch.arange(V)
    x = torch.randn(V, generator=torch.Generator().manual_seed(1)) - 20
    big = ((idx // 8) % 1024) < 19
    x[big] = torch.linspace(30, 5, int(big.sum()))
    _check_logprobs(x.view(1, V).to(BF), 20, torch.tensor([8], dtype=torch.int32))


def test_hand_checked_logprobs():
    st = K.LogitState(2, "cuda", rec_cap=1, top_n=2)
    K.token_logprobs(torch.zeros(2, 4, dtype=BF, device="cuda"), torch.tensor([3, 0], dtype=torch.int32, device="cuda"),
                     K.LogitCtx(st), 2)
    assert st.top_ids[:, 0].tolist() == [[0, 1]] * 2
    assert float((st.lp[:, 0].cpu() + math.log(4)).abs().max()) < 1e-6
    st = K.LogitState(1, "cuda", rec_cap=1, top_n=20)      # fewer tokens than N: the rest stays empty
    K.token_logprobs(torch.tensor([[1.0, 2.0, 3.0]], dtype=BF, device="cuda"),
                     torch.tensor([1], dtype=torch.int32, device="cuda"), K.LogitCtx(st), 20)
    assert st.top_ids[0, 0].tolist() == [2, 1, 0] + [-1] * 17
    want = torch.tensor([-0.40760596, -1.40760596, -2.40760596])
    assert float((st.top_lp[0, 0, :3].cpu() - want).abs().max()) < 1e-6 and abs(float(st.lp[0, 0]) + 1.40760596) < 1e-6
    assert st.top_lp[0, 0, 3:].tolist() == [NEG] * 17


@pytest.mark.parametrize("mode", ["gen", "step"])
def test_record_placement(mode):
    B, V, N, cap = 4, 1003, 3, 5
    x = torch.randn(B, V).to(BF).cuda()
    chosen = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device="cuda")
    st = K.LogitState(B, "cuda", rec_cap=cap, top_n=N)
    for t in (st.lp, st.top_lp):
        t.fill_(777.0)
    st.top_ids.fill_(-5)
    done = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device="cuda")
    if mode == "gen":
        idx = [2, 1, cap, 0]                              # row 1 is done, row 2 is at the capacity
        ctx = K.LogitCtx(st, gen=torch.tensor(idx, dtype=torch.int32, device="cuda"), done=done)
        written = {(0, 2), (3, 0)}
    else:
        ctx = K.LogitCtx(st, step=torch.tensor([4], dtype=torch.int32, device="cuda"), done=done)
        written = {(0, 4), (2, 4), (3, 4)}
    K.token_logprobs(x, chosen, ctx, N)
    lp, ids = st.lp.cpu(), st.top_ids.cpu()
    for b in range(B):
        for r in range(cap):
            if (b, r) in written:
                assert lp[b, r] <= 0 and ids[b, r].min() >= 0 and bool((st.top_lp[b, r] <= 0).all())
            else:
                assert lp[b, r] == 777.0 and ids[b, r].tolist() == [-5] * N and st.top_lp[b, r].tolist() == [777.0] * N
    if mode == "step":                                    # a step counter at the capacity: nothing at all
        st.lp.fill_(777.0)
        K.token_logprobs(x, chosen, K.LogitCtx(st, step=torch.tensor([cap], dtype=torch.int32, device="cuda")), N)
        assert bool((st.lp == 777.0).all())


# ----------------------------------------------------------------------------- engines, graph on

@pytest.fixture(scope="module")
def stack():
    cfg = get_config("tiny")
    model = DecoderModel(DecoderWeights.random(cfg, "cuda", seed=3))
    kv = PagedKVCache(cfg.layers, 96, cfg.kv_heads, cfg.head_dim, "cuda")
    return LLMEngine(model, kv, max_prefill_tokens=128, use_graph=True)


PROMPTS = [[1, 5, 9, 11, 13, 200], [1, 7, 7, 300, 12], [1, 44, 45, 46, 47, 48, 49]]


def _check_records(toks, recs, n):
    assert len(recs) == len(toks)
    for t, (lp, top) in zip(toks, recs):
        assert len(top) == n and lp <= 0 and all(a[1] >= b[1] for a, b in zip(top, top[1:])) and top[0][1] <= 0
    return [(t, lp, top[0]) for t, (lp, top) in zip(toks, recs)]


def test_continuous_engine_graph(stack):
    eng = stack
    n_new = 14
    plain = ContinuousEngine(eng, max_slots=4, max_new_cap=16, max_prompt=64, steps_per_sync=3)
    base = [plain.submit(p, n_new) for p in PROMPTS]
    plain.run()
    plain.close()
    ce = ContinuousEngine(eng, max_slots=4, max_new_cap=16, max_prompt=64, steps_per_sync=3, processors=True,
                          logprobs=4)
    assert ce.use_graph
    a = ce.submit(PROMPTS[0], n_new, logprobs=4)                                   # neutral
    b = ce.submit(PROMPTS[1], n_new, frequency_penalty=100.0, logprobs=4)
    c = ce.submit(PROMPTS[2], n_new, logit_bias={77: 100.0}, logprobs=2)
    ce.run()
    assert ce.graphs, "the step was not captured"
    assert a.tokens == base[0].tokens
    assert len(b.tokens) == n_new and len(set(b.tokens)) == n_new      # the replays read the live gen / tokens
    assert not set(b.tokens) & set(PROMPTS[1])                         # ... and the slot's own prompt tail
    assert c.tokens == [77] * n_new
    for t, lp, top1 in _check_records(a.tokens, a.logprobs, 4):
        assert top1[0] == t and top1[1] == lp                          # greedy, neutral: chosen is top-1
    _check_records(b.tokens, b.logprobs, 4)
    for t, lp, top1 in _check_records(c.tokens, c.logprobs, 2):
        assert lp <= top1[1]                                           # records are of the raw logits
    # the freed slots taken again (same prompts, so the same slots): plain requests inherit neither
    # the parameters nor the tail of the penalised and the biased request that held them
    again = [ce.submit(p, n_new, logprobs=1 if i == 0 else None) for i, p in enumerate(PROMPTS)]
    ce.run()
    assert [r.tokens for r in again] == [r.tokens for r in base]
    assert again[1].logprobs is None and [len(r[1]) for r in again[0].logprobs] == [1] * n_new
    ce.close()


def test_static_engine_graph(stack):
    eng = stack
    n_new = 12
    plain = eng.generate(PROMPTS, n_new, ignore_eos=True)
    assert eng.last_used_graph and plain.logprobs is None
    pen = eng.generate(PROMPTS, n_new, ignore_eos=True, frequency_penalty=100.0, logprobs=3)
    assert eng.last_used_graph
    for p, t, recs in zip(PROMPTS, pen.tokens, pen.logprobs):
        assert len(t) == n_new and len(set(t)) == n_new and not set(t) & set(p)
        _check_records(t, recs, 3)
    forced = eng.generate(PROMPTS, n_new, ignore_eos=True, logit_bias={77: 100.0})
    assert forced.tokens == [[77] * n_new] * 3
    same = eng.generate(PROMPTS, n_new, ignore_eos=True, logprobs=2)
    assert same.tokens == plain.tokens
    for t, recs in zip(same.tokens, same.logprobs):
        for tok, lp, top1 in _check_records(t, recs, 2):
            assert top1 == (tok, lp)
