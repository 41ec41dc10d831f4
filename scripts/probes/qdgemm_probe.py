#!/usr/bin/env python3
"""Quantized decode GEMM probe (csrc/kernels/qdgemm.hip): times Mistral-7B's decode projections
with llama.cpp's Q4_K_M types at M = 8 .. 128 against the bf16 decode GEMM (K.dgemm) on the packed
bf16 weight of the same shape -- same process, the two alternating, weights rotated over > 600 MB
so every call streams from HBM (QWeight.random: needs no file).  One JSON line per (projection, M):

    q_us / bf16_us            the GEMM launches alone (gate + up: two qdgemm launches / one dgemm)
    q_TBs                     quantized bytes over q_us
    q_step_us / bf16_step_us  as the decoder runs the projection, with the reduce that consumes the
                              slabs (residual + RMSNorm for o / down, SwiGLU for gate + up)

    python scripts/probes/qdgemm_probe.py [--out profiles/qdgemm_probe.jsonl] [--sweep]

--sweep times every (rows per workgroup, split) the kernel takes instead (the fit of
K.qdgemm_config's rates) and writes one line per configuration.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from copilot_for_consensus_amd.ops import kernels as K  # noqa: E402
from copilot_for_consensus_amd.runtime import gguf as G  # noqa: E402

H, FFN, KV, VOCAB = 4096, 14336, 1024, 32000
# (name, [(ggml type, N)], K, consumer)
PROJ = [("q", [(12, H)], H, None), ("k", [(12, KV)], H, None), ("v_q4k", [(12, KV)], H, None),
        ("v_q6k", [(14, KV)], H, None), ("qkv_q4k", [(12, H), (12, KV), (12, KV)], H, None),
        ("qkv_q6k", [(12, H), (12, KV), (14, KV)], H, None), ("o", [(12, H)], H, "norm"),
        ("gate_up", [(12, FFN), (12, FFN)], H, "swiglu"), ("down_q4k", [(12, H)], FFN, "norm"),
        ("down_q6k", [(14, H)], FFN, "norm"), ("lm_head", [(14, VOCAB)], H, "bf16")]
ROTATE_BYTES = 600 << 20


def timed(fns, iters, reps):
    """Median us per call of each fn in ``fns``: ``iters`` calls of each captured in one hipGraph (the
    decode step runs captured too, and an eager loop of ~30-us kernels times the host), the graphs
    replayed alternately, ``reps`` times each."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(s):
        for f in fns:
            for i in range(3):
                f(i)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for i in range(iters):
                    f(i)
            graphs.append(g)
        ts = [[] for _ in fns]
        for g in graphs:
            g.replay()
        s.synchronize()
        for r in range(reps):
            for k, g in enumerate(graphs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                g.replay()
                e1.record(s)
                s.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    torch.cuda.current_stream().wait_stream(s)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/qdgemm_probe.jsonl")
    ap.add_argument("--ms", nargs="+", type=int, default=[8, 16, 32, 64, 128])
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qdgemm_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev = "cuda"
    out = open(a.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()

    for name, parts, Kd, consumer in PROJ:
        if a.only and name not in a.only:
            continue
        N = sum(n for _, n in parts)
        qbytes = sum(n * Kd // G.BLOCK[t][0] * G.BLOCK[t][1] for t, n in parts)
        ncopy = min(256, max(3, ROTATE_BYTES // qbytes + 1))
        base = [K.QWeight.random(t, n, Kd, dev) for t, n in parts]
        qws = [[dataclasses.replace(q, buf=q.buf.clone()) for q in base] for _ in range(ncopy)]
        nbf = min(256, max(3, ROTATE_BYTES // (N * Kd * 2) + 1))
        wbf = torch.randn(N, Kd, device=dev).bfloat16() * 0.02
        for M in a.ms:
            pk = K.pack_dgemm_weight(wbf, swiglu=consumer == "swiglu", m=M)
            pks = [K.PackedWeight(pk.data.clone(), pk.N, pk.K, pk.bn) for _ in range(nbf)]
            x = torch.randn(M, Kd, device=dev).bfloat16()
            res = torch.randn(M, N, device=dev).bfloat16() if consumer == "norm" else None
            nw = torch.ones(N, device=dev).bfloat16() if consumer == "norm" else None
            bn, split = K.qdgemm_config(M, parts[0][1], Kd, parts[0][0])   # per launch, as the decoder asks
            dbn, dsplit = K.dgemm_config(M, N, Kd, swiglu=consumer == "swiglu", bn=pk.bn)

            def q_gemm(i, bn=bn, split=split):
                ws = qws[i % ncopy]
                if consumer == "bf16":
                    return K.qdgemm(x, ws[0], "bf16", bn=bn)
                if consumer == "swiglu":
                    buf = K._workspace(dev, split * M * N)[:split * M * N].view(split, M, N)
                    K.qdgemm(x, ws[0], "part", out=buf, interleave="gate", bn=bn)
                    return K.qdgemm(x, ws[1], "part", out=buf, interleave="up", bn=bn)
                buf = K._workspace(dev, split * M * N)[:split * M * N].view(split, M, N)
                col = 0
                for w in ws:
                    K.qdgemm(x, w, "part", out=buf, col0=col, bn=bn)
                    col += w.N
                return buf

            def q_step(i):
                y = q_gemm(i)
                if consumer == "norm":
                    return K.splitk_residual_rmsnorm(y, res, nw, 1e-5)
                if consumer == "swiglu":
                    return K.splitk_reduce(y, swiglu=True)
                return y

            def bf_gemm(i):
                w = pks[i % nbf]
                if consumer == "swiglu":
                    return K.dgemm(x, w, "swiglu", bn=dbn)
                if consumer == "bf16" or dsplit == 1:
                    return K.dgemm(x, w, "bf16", bn=dbn)
                return K.dgemm(x, w, "part", dsplit, bn=dbn)

            def bf_step(i):
                w = pks[i % nbf]
                if consumer == "norm":
                    return K.dgemm_residual_rmsnorm(x, w, res, nw, 1e-5)
                if consumer == "swiglu":
                    return K.dgemm_swiglu(x, w)
                return bf_gemm(i) if consumer is None else K.dgemm_linear(x, w)

            if a.sweep:
                nb = Kd // 256
                for b in K.QDGEMM_BNS:
                    if b < 8 * -(-M // 16):
                        continue
                    for s in sorted({1, 2, 3, 4, 7, 8, 14, 16, 28, 56} & set(range(1, nb + 1))):
                        if consumer == "bf16" and s > 1:
                            continue
                        if (-(-N // b)) * s > 8192:
                            continue
                        us, = timed([lambda i, b=b, s=s: q_gemm(i, b, s)], a.iters, 3)
                        emit({"proj": name, "M": M, "N": N, "K": Kd, "bn": b, "split": s, "q_us": round(us, 2),
                              "q_TBs": round(qbytes / us / 1e6, 3), "picked": (b, s) == (bn, split)})
                continue
            q_us, bf_us, qs_us, bfs_us = timed([q_gemm, bf_gemm, q_step, bf_step], a.iters, a.reps)
            emit({"proj": name, "M": M, "N": N, "K": Kd, "q_MB": round(qbytes / 1e6, 2),
                  "bf16_MB": round(N * Kd * 2 / 1e6, 2), "q_cfg": [bn, split], "bf16_cfg": [dbn, dsplit],
                  "q_us": round(q_us, 2), "q_TBs": round(qbytes / q_us / 1e6, 3), "bf16_us": round(bf_us, 2),
                  "bf16_TBs": round(N * Kd * 2 / bf_us / 1e6, 3), "q_step_us": round(qs_us, 2),
                  "bf16_step_us": round(bfs_us, 2), "ratio_step": round(bfs_us / qs_us, 3)})
            del pks, pk
        del qws, base, wbf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
