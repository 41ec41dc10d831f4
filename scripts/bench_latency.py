#!/usr/bin/env python3
"""Single-stream latency benchmark: one request at a time, the operating point of every decode speed
the reference publishes (Ollama / llama.cpp, BASELINE.md: Mistral 150-200 tok/s on an RTX 4090,
Llama 2 13B 20-25 tok/s and TTFT ~2 s on an RX 6700 XT, ...).

For each model: random-init bf16 weights of that architecture, a synthetic prompt of ``--prompt``
tokens, greedy decode of ``--new`` tokens with the hipGraph decode step.  Reports TTFT (prefill of
the prompt + first token) and decode tokens/s (tokens after the first / decode wall time), median
over ``--reps`` runs.  The prefix cache is off so every run prefills the whole prompt.

    python scripts/bench_latency.py --models mistral-7b llama-2-7b llama-2-13b --prompt 512 2500

``--batch B`` decodes B such requests together (one engine call; decode tokens/s is then the sum
over the batch); with quantized weights ``--ab-qgemm`` runs every point twice in the same process,
on the quantized decode GEMM and with ``CFC_DECODE_QGEMM=0`` (the bf16 copies above B = 4).

    python scripts/bench_latency.py --models mistral-7b --weights q4_k_m --batch 8 --ab-qgemm

``--gguf-resident quant`` keeps the quantized weights resident in their blocks only
(DecoderWeights.to_quant_only: the bf16 consumers read a scratch unpacked from the blocks);
``both`` runs every point on two weight sets of the same blocks in the same process, one resident
each way, and every row carries resident_bytes() and torch.cuda.max_memory_allocated() (the
process's peak since the weights were built: with ``both`` it covers the two weight sets, so run
one residency per process to compare peaks).

    python scripts/bench_latency.py --models mistral-7b --weights q4_k_m --batch 8 --gguf-resident both
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights, get_config  # noqa: E402
from copilot_for_consensus_amd.runtime.engine import LLMEngine  # noqa: E402
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache, blocks_needed  # noqa: E402

# Published single-stream decode speeds (tok/s) for the same architecture, best hardware quoted
# (BASELINE.md).  Quantised (Q4_K_M / Q8_0) on the reference side; bf16 here.
PUBLISHED = {
    "mistral-7b": {"tok_s": 200.0, "hw": "RTX 4090, Ollama (docs/operations/ollama-gpu-setup.md:150)"},
    "llama-2-7b": {"tok_s": 80.0, "hw": "RTX 3060, Ollama (docs/operations/ollama-gpu-setup.md:152)"},
    "llama-2-13b": {"tok_s": 25.0, "ttft_s": 2.0, "hw": "RX 6700 XT, llama.cpp Q4_K_M (docs/operations/llm-gpu-setup.md:476)"},
}


def run_model(name, prompt_lens, new, reps, seed, weights="bf16", batch=1, ab_qgemm=False, resident="bf16"):
    cfg = get_config(name)
    dev = torch.device("cuda")
    wbytes = cfg.num_params() * 2
    if resident != "bf16" and weights == "bf16":
        raise SystemExit("--gguf-resident quant / both needs --weights q4_k_m or q8_0")

    def make_weights(quant_only):
        w = DecoderWeights.random(cfg, dev, seed=seed)
        if weights != "bf16":
            # ggml-quantized projections (llama.cpp's Q4_K_M type recipe, or all Q8_0), random blocks:
            # decode streams them (csrc/kernels/quant.hip); prefill keeps the bf16 copies unless the
            # weights are resident in their blocks only (then it reads the unpack scratch)
            from copilot_for_consensus_amd.ops.kernels import attach_random_quant
            attach_random_quant(w, weights, seed)
        return w.to_quant_only() if quant_only else w

    # (weights, CFC_DECODE_QGEMM flag or None) per engine
    runs = [(make_weights(r == "quant"), None) for r in (("bf16", "quant") if resident == "both" else (resident,))]
    w = runs[0][0]
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()      # the peak from here on: resident weights + KV + activations
    if weights != "bf16":
        wbytes = sum(q.nbytes for layer in w.qlayers for q in layer.values()) + w.q_lm_head.nbytes
    if ab_qgemm and weights != "bf16":
        runs = [(rw, flag) for rw, _ in runs for flag in (("1",) if rw.quant_only else ("1", "0"))]
    engines = []
    for w, flag in runs:
        saved = os.environ.get("CFC_DECODE_QGEMM")
        if flag is not None:
            os.environ["CFC_DECODE_QGEMM"] = flag
        try:
            model = DecoderModel(w)
        finally:
            if flag is not None:
                os.environ.pop("CFC_DECODE_QGEMM")
                if saved is not None:
                    os.environ["CFC_DECODE_QGEMM"] = saved
        if weights != "bf16":
            assert model.decode_qgemv
        kv = PagedKVCache(cfg.layers, batch * blocks_needed(max(prompt_lens) + new) + 8, cfg.kv_heads, cfg.head_dim,
                          dev)
        engines.append(LLMEngine(model, kv, max_prefill_tokens=16384, prefix_cache=False))
    g = torch.Generator().manual_seed(seed)
    rows = []
    for plen in prompt_lens:
        prompts = [[cfg.bos_id] + torch.randint(3, cfg.vocab_size, (plen - 1,), generator=g).tolist()
                   for _ in range(batch)]
        for eng in engines:
            eng.generate(prompts, max_new_tokens=new, ignore_eos=True)      # capture the graph, warm GEMMs
        stats = [([], []) for _ in engines]
        for _ in range(reps):
            for eng, (ttft, tps) in zip(engines, stats):      # the engines alternate rep by rep
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = eng.generate(prompts, max_new_tokens=new, ignore_eos=True)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                ttft.append(res.ttft_s)
                tps.append(sum(len(t) - 1 for t in res.tokens) / max(wall - res.ttft_s, 1e-9))
        for eng, (ttft, tps) in zip(engines, stats):
            row = {"model": name, "prompt_tokens": plen, "new_tokens": new, "ttft_s": round(statistics.median(ttft), 4),
                   "decode_tok_s": round(statistics.median(tps), 1),
                   "ms_per_token": round(1000.0 / statistics.median(tps), 3),
                   "weights": weights, "weight_gb": round(wbytes / 1e9, 2)}
            if batch > 1:
                row["batch"] = batch
                row["decode_path"] = eng.model.decode_path(batch)
            row["decode_qgemm"] = bool(eng.model.decode_qgemm)
            if weights != "bf16":
                row["gguf_resident"] = "quant" if eng.model.w.quant_only else "bf16"
                row["resident_bytes"] = eng.model.w.resident_bytes()
                row["max_memory_allocated"] = torch.cuda.max_memory_allocated()
            # HBM bytes one decode step must read: all weights + the KV of the context so far
            kv_bytes = 2 * cfg.layers * cfg.kv_heads * cfg.head_dim * 2 * (plen + new / 2)
            # (a batch shares the weight read: steps/s = tok/s / batch, every request's KV is read each step)
            row["achieved_TB_s"] = round((wbytes + batch * kv_bytes) * statistics.median(tps) / batch / 1e12, 2)
            pub = PUBLISHED.get(name)
            if pub:
                row["published_tok_s"] = pub["tok_s"]
                row["published_hw"] = pub["hw"]
                row["vs_published"] = round(row["decode_tok_s"] / pub["tok_s"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
    del engines, eng, kv, model, runs, w
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["mistral-7b", "llama-2-7b", "llama-2-13b"])
    ap.add_argument("--prompt", nargs="+", type=int, default=[512, 2500])
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", choices=["bf16", "q4_k_m", "q8_0"], default="bf16",
                    help="decode weight format (q4_k_m / q8_0: ggml blocks streamed by the quantized GEMV)")
    ap.add_argument("--batch", type=int, default=1, help="requests decoded together (decode tok/s: their sum)")
    ap.add_argument("--ab-qgemm", action="store_true",
                    help="quantized weights: every point also with CFC_DECODE_QGEMM=0, the two alternating")
    ap.add_argument("--gguf-resident", choices=["bf16", "quant", "both"], default="bf16",
                    help="quantized weights: keep the bf16 copies (bf16), the ggml blocks only (quant), or run "
                         "every point on one weight set of each kind (both)")
    a = ap.parse_args()
    for name in a.models:
        run_model(name, a.prompt, a.new, a.reps, a.seed, a.weights, a.batch, a.ab_qgemm, a.gguf_resident)


if __name__ == "__main__":
    main()
