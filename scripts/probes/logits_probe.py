#!/usr/bin/env python3
"""Logit-processor / token-logprob probe (csrc/kernels/logits.hip): times the two kernels beside
sample_kernel and sample_topk_kernel in one process at decode shapes.  Each timing is a hipGraph
of `--calls` launches replayed `--reps` times between device events (no host launch gaps), once on
one logits buffer (warm: the step's case, the lm_head GEMM has just written the row) and once
rotating over enough buffers to exceed the 256 MiB Infinity Cache (cold).

    python scripts/probes/logits_probe.py [--batches 1 8 64 128] [--vocabs 32000 128256]

Prints one JSON line per (B, V) with microseconds per launch.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from copilot_for_consensus_amd.ops import kernels as K  # noqa: E402


def timed(fn, ncopy, calls, reps):
    """us per launch of fn(i) (i picks the buffer), graph-replayed."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(ncopy):
            fn(i)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for i in range(calls):
            fn(i % ncopy)
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return round(1e3 * a.elapsed_time(b) / (reps * calls), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8, 64, 128])
    ap.add_argument("--vocabs", nargs="+", type=int, default=[32000, 128256])
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    for V in a.vocabs:
        for B in a.batches:
            nbytes = B * V * 2
            cold = min(a.calls, max(2, (320 << 20) // nbytes + 1))
            bufs = [(torch.randn(B, V, generator=g) * 3).to(torch.bfloat16).to(dev) for _ in range(min(cold, 4))]
            bufs += [bufs[i % 4].clone() for i in range(cold - len(bufs))]
            pbufs = [b.clone() for b in bufs]
            out = torch.zeros(B, dtype=torch.int32, device=dev)
            step = torch.ones(1, dtype=torch.int32, device=dev)
            cap = 1100
            tokens = torch.randint(0, 2000, (B, cap), generator=g).to(torch.int32).to(dev)
            row = {"B": B, "V": V, "row_bytes": V * 2, "cold_buffers": cold}

            def state(last_n, nbias, rec=False, top=0):
                st = K.LogitState(B, dev, rec_cap=4 if rec else 0, top_n=top)
                bias = {int(i): 1.0 for i in torch.randperm(V, generator=g)[:nbias]}
                p = K.LogitParams.make(1.1, last_n, 0.1, 0.1, bias, vocab=V)
                st.set_rows(range(B), [p] * B, [list(range(1, 1200))] * B)
                return st

            kernels = {
                "sample_greedy": lambda i: K.sample(bufs[i], out, 0.0, 0, step),
                "sample_temp": lambda i: K.sample(bufs[i], out, 0.7, 0, step),
                "sample_topk40": lambda i: K.sample(bufs[i], out, K.SamplingParams(0.7, 40, 0.95, 0.05), 0, step),
            }
            for name, (n, nb) in {"proc_w64": (64, 0), "proc_w64_bias512": (64, 512), "proc_w1024": (-1, 0),
                                  "proc_w1024_bias512": (-1, 512)}.items():
                ctx = K.LogitCtx(state(n, nb), tokens=tokens, gen=torch.full((B,), 1000, dtype=torch.int32, device=dev))
                # in place, so on copies: the rows the samplers and the logprobs read stay as drawn
                kernels[name] = lambda i, ctx=ctx: K.logit_processors(pbufs[i], ctx)
            for name, top in {"logprobs_n0": 0, "logprobs_n1": 1, "logprobs_n20": 20}.items():
                ctx = K.LogitCtx(state(0, 0, True, top), step=step)
                kernels[name] = lambda i, ctx=ctx, top=top: K.token_logprobs(bufs[i], out, ctx, top)
            for name, fn in kernels.items():
                row[name] = {"warm_us": timed(fn, 1, a.calls, a.reps), "cold_us": timed(fn, cold, a.calls, a.reps)}
            print(json.dumps(row), flush=True)
            del bufs, pbufs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
