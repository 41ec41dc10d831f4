#!/usr/bin/env python3
"""Headline benchmark: end-to-end threads summarized / s (+ p50 summary latency), Mistral-7B.

BASELINE.json metric: "end-to-end threads summarized/sec + p50 summary latency, Mistral-7B TP=1/8".
One step = one batch of mailing-list threads per GPU taken through the whole pipeline of the
reference (ingest bytes -> parse mbox -> thread -> chunk -> embed (HIP encoder) -> index (HIP kNN)
-> orchestrator top-k context selection -> prompt -> Mistral-7B prefill + 512-token greedy decode
(hand-written HIP kernels only -- MFMA prefill / decode GEMMs, flash prefill, paged decode
attention; hipGraph decode) -> summary + citations).  Synthetic .mbox data and
random-init bf16 weights (no network).  Data parallel over ranks (one process per GPU, RCCL
barrier/all-reduce for timing): weak scaling, per-GPU work fixed.

    python bench.py [--gpus N --steps K --warmup W]
    torchrun --nproc-per-node N bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the result line.  ``--full`` adds what
is measured outside the timed window (the latency points under Poisson arrivals, the light-load
point through the services, the topic-search latency); ``--dump-outputs DIR`` writes what the last
timed step generated as ``DIR/<name>.npy``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

# before torch loads: c10d logs every timed-out TCPStore wait of the DP control plane's idle
# threads (--pipeline node) as a warning
os.environ.setdefault("TORCH_CPP_LOG_LEVEL", "ERROR")

# Reference operating point derived in BASELINE.md: best published number (RTX 4090, 150-200
# tok/s Ollama decode) => ~3-4 s per thread => 0.25-0.33 threads/s.  We divide by the MOST
# favourable-to-the-reference value (1/3 thread/s); the AMD RX 6700 XT point is 0.07-0.09.
BASELINE_THREADS_PER_S = 1.0 / 3.0


def metric_name(model: str) -> str:
    """BASELINE.json's metric string, with the decoder actually run (``--model``) in it."""
    words = model.split("-")
    pretty = "-".join(w.capitalize() if not w[:1].isdigit() else w.upper() for w in words)
    return f"end-to-end threads summarized/sec + p50 summary latency, {pretty} TP=1/8"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--encoder", default="minilm-l6")
    ap.add_argument("--threads-per-gpu", type=int, default=128, help="threads summarized per engine (GPU, or TP group) per step")
    ap.add_argument("--max-new", type=int, default=512, help="generated tokens per summary (llama.cpp n_predict)")
    ap.add_argument("--tp", type=int, default=1)
    ap.add_argument("--prefill-tokens", type=int, default=16384)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="KV-cache storage; fp8 (e4m3fn) is an opt-in precision trade-off, not the headline")
    ap.add_argument("--weights", choices=["bf16", "fp8"], default="bf16",
                    help="decoder projections; fp8 = opt-in W8A8 e4m3fn (precision trade-off, not the headline)")
    ap.add_argument("--llm-only", action="store_true", help="skip the CPU/encoder/kNN stages (diagnostic)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kv-max-prompt", type=int, default=4096,
                    help="prompt tokens per thread the paged KV pool is sized for (x threads x 1.1)")
    ap.add_argument("--index-prefill", type=int, default=1_000_000,
                    help="background vectors resident in the HBM kNN index besides the run's own chunks")
    ap.add_argument("--no-overlap", action="store_true", help="run pipeline stages strictly sequentially")
    ap.add_argument("--overlap-prefill", choices=["on", "off"], default=os.environ.get("CFC_OVERLAP_PREFILL", "off"),
                    help="prefill batch i+1 on half the CUs beside batch i's decode (runtime/cu_partition.py)")
    ap.add_argument("--latency-rate", type=float, default=8.0,
                    help="latency half of the metric: Poisson arrivals per second per GPU served by the continuous "
                         "engine after the timed throughput steps (0 = skip)")
    ap.add_argument("--latency-steps", type=int, default=2, help="batches of threads the latency probe replays")
    ap.add_argument("--latency-low-rate", type=float, default=0.5,
                    help="a second latency point at a light load (the reference's one-thread-at-a-time regime): "
                         "Poisson arrivals per second per GPU (0 = skip)")
    ap.add_argument("--latency-low-threads", type=int, default=12, help="threads the light-load probe serves")
    ap.add_argument("--service-latency-rate", type=float, default=0.5,
                    help="the light-load point through the real services (pipeline/node_bench.py: archive submit "
                         "-> report stored), Poisson arrivals per second per GPU (0 = skip; TP=1 only)")
    ap.add_argument("--service-latency-threads", type=int, default=12)
    ap.add_argument("--search-queries", type=int, default=64,
                    help="topic searches timed after the throughput steps (GET /api/reports/search through "
                         "ReportingService: HIP encoder + HIP kNN top-150 over the resident index; 0 = skip)")
    ap.add_argument("--pipeline", choices=["bench", "node"], default="bench",
                    help="bench: the stage code with a static LLM batch (headline); node: the real services "
                         "(Node, in-proc bus, continuous summarization engine), pipeline/node_bench.py")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the probes that take runs of their own: --latency-rate, "
                         "--latency-low-rate, --service-latency-rate and --search-queries (all off without it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one generated (token ids and prompt lengths "
                         "per thread) as DIR/<name>.npy, float32; same arguments -> same inputs from run to run")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.pipeline == "node":
        ap.error("--dump-outputs reads the engine of --pipeline bench; the node pipeline stores reports instead")
    if not args.full:
        # a plain run does only what the headline figure needs
        args.latency_rate = args.latency_low_rate = args.service_latency_rate = 0.0
        args.search_queries = 0
    return args


def dump_outputs(out_dir, res, rank, world):
    """--dump-outputs: the arrays the last timed step's ``LLMEngine.generate`` returned -- the
    generated token ids of every thread (one row each, -1 behind a shorter row) and the prompt
    lengths -- as float32 (ids stay below 2**24, so they are exact)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    tag = f".rank{rank}" if world > 1 else ""
    tokens = np.full((len(res.tokens), max((len(t) for t in res.tokens), default=0)), -1.0, dtype=np.float32)
    for i, t in enumerate(res.tokens):
        tokens[i, :len(t)] = t
    np.save(os.path.join(out_dir, f"generated_tokens{tag}.npy"), tokens)
    np.save(os.path.join(out_dir, f"prompt_lens{tag}.npy"), np.asarray(res.prompt_lens, dtype=np.float32))


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        print(f"[bench] warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    from copilot_for_consensus_amd.parallel import init_distributed, make_groups
    from copilot_for_consensus_amd.pipeline.bench_pipeline import BenchPipeline

    env = init_distributed()
    dev = env.device
    # TP groups of args.tp consecutive ranks (one engine per group), DP across groups
    groups = make_groups(env, args.tp)
    if args.pipeline == "node":
        return _main_node(args, env, groups)
    pipe = BenchPipeline(model=args.model, encoder=args.encoder, device=dev, threads_per_step=args.threads_per_gpu,
                         max_new_tokens=args.max_new, tp=args.tp, prefill_tokens=args.prefill_tokens, kv_dtype=args.kv_dtype,
                         weight_dtype=args.weights,
                         llm_only=args.llm_only, use_graph=not args.no_graph,
                         seed=args.seed + 7919 * groups.dp_rank, groups=groups if args.tp > 1 else None,
                         index_prefill=args.index_prefill, kv_max_prompt=args.kv_max_prompt,
                         # DP: the TP leaders' RAG indexes form one sharded index (vectors of a thread on
                         # the GPU that owns it; insert + relevance exchanged over RCCL each batch)
                         index_group=groups.dp_group if groups.dp_size > 1 and not args.llm_only else None,
                         overlap_prefill=args.overlap_prefill == "on" and not args.no_overlap)
    last_generation = []
    if args.dump_outputs:
        # every schedule ends a batch in LLMEngine.finish (generate calls it too): keep its last result
        finish = pipe.engine.finish

        def keep_last(*a, **kw):
            last_generation[:] = [finish(*a, **kw)]
            return last_generation[0]
        pipe.engine.finish = keep_last

    # the latency half runs at every TP degree (the TP followers replay the continuous engine's steps)
    probe_steps = list(range(args.warmup + args.steps, args.warmup + args.steps + args.latency_steps)) \
        if args.latency_rate > 0 and not args.llm_only else []
    low_steps = [args.warmup + args.steps + args.latency_steps] if probe_steps and args.latency_low_rate > 0 else []
    pipe.prepare_sources(list(range(args.warmup + args.steps)) + probe_steps + low_steps)

    def barrier():
        if world > 1:
            dist.barrier()
        if dev.type == "cuda":   # CPU rehearsal (tests/test_bench_contract_cpu.py) has no device to sync
            torch.cuda.synchronize(dev)

    def progress(kind):
        # one stderr line per finished step on rank 0 (a long timed loop stays visibly alive);
        # stdout carries only the final JSON line
        def report(i, r):
            if rank == 0:
                print(f"[bench] {kind} {i}: {r.summary()}", file=sys.stderr, flush=True)
        return report

    overlap_prefill = pipe.overlap_prefill

    def run(steps, kind):
        if pipe.overlap_prefill:
            return pipe.run_steps_overlapped(steps, on_step=progress(kind))
        return pipe.run_steps(steps, overlap=not args.no_overlap, on_step=progress(kind))
    run(list(range(args.warmup)), "warmup")

    barrier()
    t0 = time.perf_counter()
    results = run(list(range(args.warmup, args.warmup + args.steps)), "step")
    barrier()
    elapsed = time.perf_counter() - t0

    # one report per DP replica: TP followers ran the same threads as their leader
    lead = groups.tp_rank == 0
    if args.dump_outputs and lead and last_generation:
        dump_outputs(args.dump_outputs, last_generation[0], rank, world)
    threads_local = sum(r.threads for r in results) if lead else 0
    lat_local = [x for r in results for x in r.latencies_s] if lead else []
    gen_tokens_local = sum(r.generated_tokens for r in results) if lead else 0
    prompt_tokens_local = sum(r.prompt_tokens for r in results) if lead else 0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        c = torch.tensor([threads_local, gen_tokens_local, prompt_tokens_local], dtype=torch.float64, device=dev)
        dist.all_reduce(c)
        threads, gen_tokens, prompt_tokens = (float(x) for x in c.tolist())
        lats = [None] * world
        dist.all_gather_object(lats, lat_local)
        lat_all = [x for part in lats for x in part]
    else:
        threads, gen_tokens, prompt_tokens, lat_all = threads_local, gen_tokens_local, prompt_tokens_local, lat_local

    value = threads / elapsed
    p50 = statistics.median(lat_all) if lat_all else None

    def probe_point(steps, rate, seed, max_threads=None):
        """One latency point: every DP replica's continuous engine under Poisson arrivals; the TP
        followers' empty dicts are dropped before the aggregate."""
        barrier()
        probe = pipe.latency_probe(steps, rate, seed=seed, max_threads=max_threads)
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, probe)
            probe = [p for p in parts if p]
        else:
            probe = [probe]
        agg = dict(probe[0])
        agg.update(threads=sum(p["threads"] for p in probe),
                   p50_s=round(statistics.median([p["p50_s"] for p in probe]), 3),
                   p95_s=round(max(p["p95_s"] for p in probe), 3),
                   throughput_threads_per_s=round(sum(p["throughput_threads_per_s"] for p in probe), 3))
        return agg
    # after the timed window: the reference's one live vector query, the reporting topic search
    # (embed + kNN top-150 over the resident index + enrichment), on an otherwise idle GPU
    search = None
    if args.search_queries > 0 and not args.llm_only:
        barrier()
        sp = pipe.search_probe(args.search_queries, limit=50, seed=args.seed + 31 * groups.dp_rank)
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, sp)
            parts = [p for p in parts if p]
        else:
            parts = [sp] if sp else []
        if parts:
            search = dict(parts[0])
            search.update(queries=sum(p["queries"] for p in parts),
                          reports_per_query=round(statistics.mean(p["reports_per_query"] for p in parts), 1),
                          p50_ms=round(statistics.median([p["p50_ms"] for p in parts]), 2),
                          p95_ms=round(max(p["p95_ms"] for p in parts), 2), max_ms=round(max(p["max_ms"] for p in parts), 2))
    # after the timed window: the same GPUs at a load below saturation (Poisson arrivals), then a
    # light load -- a few threads far apart, the regime of the reference's published 3-4 s per thread
    latency = probe_point(probe_steps, args.latency_rate, args.seed + 104729 * groups.dp_rank) if probe_steps else None
    latency_low = (probe_point(low_steps, args.latency_low_rate, args.seed + 7919 + 104729 * groups.dp_rank,
                               max_threads=args.latency_low_threads) if low_steps else None)
    service_light = None
    if args.service_latency_rate > 0 and args.tp == 1 and not args.llm_only:
        # the light-load point again, through the deployment's services on this GPU (a node beside
        # the bench pipeline's model: its own encoder, index and decoder), admitting each thread on
        # arrival as a lightly loaded summarization service does
        from copilot_for_consensus_amd.pipeline.node_bench import NodeBench
        # the bench pipeline is finished: free its model, KV pool and index before the node builds
        # its own, so the peak is one stack per rank (two ranks sharing one GPU fit too)
        del pipe
        import gc
        gc.collect()
        if dev.type == "cuda":
            torch.cuda.empty_cache()
        barrier()
        nb = NodeBench(model=args.model, encoder=args.encoder, device=dev, threads_per_step=args.threads_per_gpu,
                       max_new_tokens=args.max_new, seed=args.seed + 7919 * groups.dp_rank,
                       index_prefill=args.index_prefill, min_admit=1, admit_wait_ms=50)
        try:
            sp = nb.light_load_probe(args.service_latency_rate, args.service_latency_threads,
                                     seed=args.seed + 271 * groups.dp_rank)
        finally:
            nb.close()
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, sp)
        else:
            parts = [sp]
        service_light = dict(parts[0])
        service_light.update(threads=sum(p["threads"] for p in parts),
                             p50_s=round(statistics.median([p["p50_s"] for p in parts]), 3),
                             p95_s=round(max(p["p95_s"] for p in parts), 3))
    if rank == 0:
        out = {
            "metric": metric_name(args.model),
            "value": round(value, 4),
            "unit": "threads/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000 * elapsed / args.steps, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / BASELINE_THREADS_PER_S, 2),
            "dtype": "bf16" if args.weights == "bf16" else "fp8_e4m3fn W8A8 (opt-in, reduced precision)",
            "data": "synthetic .mbox threads, random-init weights",
            "config": {
                "model": args.model,
                "encoder": args.encoder,
                "global_batch": args.threads_per_gpu * groups.dp_size,
                "seq_len": round(prompt_tokens / max(threads, 1)),
                "max_new_tokens": args.max_new,
                "kv_cache": "bf16" if args.kv_dtype == "bf16" else "fp8_e4m3fn (opt-in, reduced-precision KV)",
                "parallelism": f"dp{groups.dp_size}" + (f"xtp{args.tp}" if args.tp > 1 else ""),
                # "index": the chunk vectors go into the HBM kNN index; "centroid-select": the
                # orchestrator scores each thread's own rows against their centroid (the reference's
                # ThreadChunksSource reads a thread's chunks, orchestrator/app/context_sources.py:40);
                # the HIP kNN query path is timed separately in search_latency
                "pipeline": ("llm-only" if args.llm_only
                             else "parse+chunk+embed+index+centroid-select+prefill+decode"),
                "index": (f"sharded over {groups.dp_size} GPUs by thread (RCCL all_to_all insert + relevance)"
                          if groups.dp_size > 1 and not args.llm_only else "one HBM index per GPU"),
                "schedule": ("prefill of batch i+1 on half the CUs beside batch i's decode" if overlap_prefill
                             else "prefill then decode per batch (next batch's preparation overlapped)"),
            },
            "p50_summary_latency_s": round(p50, 3) if p50 is not None else None,
            "p50_summary_latency_regime": ("saturated: every thread of a timed batch, from its batch's "
                                           "preparation start to its last token (see latency_mode* for "
                                           "stated arrival rates below saturation)"),
            # latency half of the metric at a stated arrival rate below saturation (continuous engine)
            "latency_mode": latency,
            "latency_mode_light": latency_low,
            # the same light load through the real services (archive submit -> report stored)
            "latency_service_light": service_light,
            # GET /api/reports/search (topic search: HIP encoder + HIP kNN + enrichment) vs the P95 0.5 s SLO
            "search_latency": search,
            "generated_tokens_per_s": round(gen_tokens / elapsed, 1),
            "prompt_tokens_per_s": round(prompt_tokens / elapsed, 1),
            "baseline_threads_per_s": round(BASELINE_THREADS_PER_S, 4),
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def _main_node(args, env, groups):
    """--pipeline node: the same metric through the deployment's services.  One rank: a whole node
    on the GPU.  Under torchrun: the topology ``services.main node`` deploys -- rank 0 runs the
    services with the DP facades, every rank a DPNodeWorker (its own encoder, HBM index shard and
    continuous LLM engine); a step is one archive of threads-per-gpu x world threads."""
    import torch
    import torch.distributed as dist

    from copilot_for_consensus_amd.pipeline.node_bench import NodeBench
    if args.tp > 1:
        raise SystemExit("--pipeline node runs one model per rank (DP over ranks)")
    world, rank, dev = env.world, env.rank, env.device
    dp = None
    cpu = None
    if world > 1:
        # host-side barriers / gathers on their own gloo group: the DP workers' serve threads keep
        # using the GPU (and the job's store) while the main thread waits here
        cpu = dist.new_group(backend="gloo")
        dp = {"store": dist.distributed_c10d._get_default_store(), "rank": rank, "world": world}
    nb = NodeBench(model=args.model, encoder=args.encoder, device=dev, threads_per_step=args.threads_per_gpu,
                   max_new_tokens=args.max_new, seed=args.seed, index_prefill=args.index_prefill, dp=dp)
    if rank == 0:
        nb.prepare_sources(list(range(args.warmup + args.steps)))

    def report(kind):
        def f(i, r):
            if rank == 0:
                print(f"[bench-node] {kind} {i}: {r.summary()}", file=sys.stderr, flush=True)
        return f

    def barrier():
        if world > 1:
            dist.barrier(group=cpu)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    barrier()                                   # every rank's models and index built
    if args.warmup and rank == 0:
        nb.run_steps(list(range(args.warmup)), on_step=report("warmup"))
    barrier()
    t0 = time.perf_counter()
    results = nb.run_steps(list(range(args.warmup, args.warmup + args.steps)), on_step=report("step")) \
        if rank == 0 else []
    barrier()
    elapsed = time.perf_counter() - t0
    threads = sum(r.threads for r in results)
    gen = sum(r.generated_tokens for r in results)
    prompt = sum(r.prompt_tokens for r in results)
    lats = [x for r in results for x in r.latencies_s]
    # the light-load point through the same topology (rank 0's services, every rank's worker serving
    # its owned threads): one-thread archives at a Poisson rate, archive submit -> report stored
    service_light = None
    if args.service_latency_rate > 0:
        barrier()
        if rank == 0:
            service_light = nb.light_load_probe(args.service_latency_rate, args.service_latency_threads,
                                                seed=args.seed + 271)
        barrier()
    per_rank = [nb.dp_stats()]
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, nb.dp_stats(), group=cpu)
    nb.close()
    if rank == 0:
        value = threads / elapsed
        print(json.dumps({
            "metric": metric_name(args.model),
            "value": round(value, 4), "unit": "threads/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": round(value / BASELINE_THREADS_PER_S, 2), "dtype": "bf16",
            "data": "synthetic .mbox threads, random-init weights",
            "config": {"model": args.model, "encoder": args.encoder, "global_batch": args.threads_per_gpu * world,
                       "seq_len": round(prompt / max(threads, 1)), "max_new_tokens": args.max_new, "kv_cache": "bf16",
                       "parallelism": f"dp{world}",
                       "pipeline": "node: ingestion+parse+chunk+embed+index+select+continuous prefill/decode+report",
                       "topology": ("services.main node: rank-0 services + a DPNodeWorker per rank (encoder, HBM "
                                    "index shard, continuous engine) over the TCPStore control plane"
                                    if world > 1 else "one node on the GPU")},
            "p50_summary_latency_s": round(statistics.median(lats), 3) if lats else None,
            "p50_summary_latency_regime": "archive submit -> report stored, paced source (<= 2 steps in flight)",
            "per_rank": per_rank if world > 1 else None,
            "latency_service_light": service_light,
            "dp_wait": os.environ.get("CFC_DP_WAIT", "block") if world > 1 else None,
            "generated_tokens_per_s": round(gen / elapsed, 1), "prompt_tokens_per_s": round(prompt / elapsed, 1),
            "baseline_threads_per_s": round(BASELINE_THREADS_PER_S, 4)}), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
