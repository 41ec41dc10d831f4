#!/usr/bin/env python3
"""What per-request sampler settings cost and buy (ROOFLINE.md, README "Sampler fields").

``kernel``: device time per launch of ``sample_rows`` against the two kernels it shares its code
with, at one decode step's shape (``--rows`` x ``--vocab`` bf16 logits), all in this process:
all-greedy rows against ``cfc_sample``, and rows with top_k 40 / top_p 0.95 / min_p 0.05 against
``cfc_sample_truncated``.  Every timing is of ``--iters`` launches replayed from one captured graph
(the way the decode step runs them), between device events, best of ``--reps`` alternating rounds.

``server``: ``--clients`` concurrent requests with as many distinct seeds through one
``BatchScheduler``, with ``per_request_sampling`` off (one slot engine per configuration, four at
the most, the rest through blocking ``generate`` calls) and on (one engine).  Two waves per
scheduler, the second with fresh seeds as an OpenAI client sends them; wall time of each wave.
One JSON line per mode.
"""
import argparse
import concurrent.futures as cf
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernel(a):
    from copilot_for_consensus_amd.ops import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this is a device measurement")
    B, V = a.rows, a.vocab
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, V, generator=g) * 2).to(torch.bfloat16).cuda()
    out = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    trunc = K.SamplingParams(0.7, 40, 0.95, 0.05)
    rows_g, rows_t = K.SamplerRows(B, "cuda"), K.SamplerRows(B, "cuda")
    rows_t.set_rows(range(B), [trunc] * B, range(B))
    cases = {"sample_greedy": lambda: K.sample(x, out, 0.0, 0, step),
             "sample_rows_greedy": lambda: K.sample_rows(x, out, rows_g, B),
             "sample_truncated": lambda: K.sample(x, out, trunc, 1, step),
             "sample_rows_truncated": lambda: K.sample_rows(x, out, rows_t, B)}
    graphs = {}
    s = torch.cuda.Stream()
    for name, fn in cases.items():
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            for _ in range(a.iters):
                fn()
        graphs[name] = gr
    best = {n: float("inf") for n in cases}
    for _ in range(a.reps):
        for name, gr in graphs.items():
            gr.replay()                     # warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1) * 1e3 / a.iters)
    res = {"metric": "sampler kernels, us per launch (graph replay)", "rows": B, "vocab": V, "iters": a.iters,
           **{n: round(v, 2) for n, v in best.items()},
           "rows_minus_sample_greedy_us": round(best["sample_rows_greedy"] - best["sample_greedy"], 2),
           "rows_minus_sample_truncated_us": round(best["sample_rows_truncated"] - best["sample_truncated"], 2)}
    print(json.dumps(res), flush=True)


def server(a):
    from copilot_for_consensus_amd.serving import build_from_config
    from copilot_for_consensus_amd.serving.llm_server import GenRequest
    res = {"metric": "concurrent seeded requests through one scheduler, wall s per wave", "model": a.model,
           "clients": a.clients, "prompt": a.prompt, "new": a.new}
    for on in (False, True):
        app, s = build_from_config({"model": a.model, "device": "cuda", "max_new_tokens": a.new, "max_batch": 16,
                                    "kv_cache_tokens": 32 * (a.prompt + a.new) + 4096, "per_request_sampling": on},
                                   max_prompt=a.prompt + 64, max_new_cap=a.new)
        sched = app.state.scheduler
        rng = random.Random(0)
        V = s.cfg.vocab_size
        # warm the libraries and the prefill outside the scheduler (no slot engine is built for it)
        s.engine.generate([[s.cfg.bos_id] + [rng.randrange(3, V) for _ in range(a.prompt - 1)]], 4, ignore_eos=True)
        waves = []
        for wave in range(2):
            reqs = [GenRequest([s.cfg.bos_id] + [rng.randrange(3, V) for _ in range(a.prompt - 1)], a.new, 0.7, 40, 0.95,
                               0.05, seed=1000 * wave + i + 1, ignore_eos=True) for i in range(a.clients)]
            t0 = time.perf_counter()
            with cf.ThreadPoolExecutor(a.clients) as pool:
                done = list(pool.map(sched.submit, reqs))
            waves.append(round(time.perf_counter() - t0, 3))
            assert all(len(r.tokens) == a.new for r in done)
        res["on" if on else "off"] = {"wave_s": waves, "engines": len(sched.engines), "batches": sched.batches,
                                      "max_batch_seen": sched.max_seen_batch}
        sched.close()
        for ce in sched.engines.values():
            ce.close()
        del app, s, sched
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "server"])
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    a = ap.parse_args()
    kernel(a) if a.mode == "kernel" else server(a)


if __name__ == "__main__":
    main()
