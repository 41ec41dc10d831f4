#!/usr/bin/env python3
"""FP8 decode GEMM probe (csrc/kernels/f8dgemm.hip): times Mistral-7B's four decode projections at
M = 8 .. 128 three ways in one process, the three alternating, weights rotated over > 600 MB so
every call streams from HBM:

    f8     K.f8dgemm on the packed FP8 weight            (+ the kernels the f8gemm family runs with it)
    lib    K.linear_fp8 (torch._scaled_mm, hipBLASLt)    (+ the kernels the library FP8 loop runs with it)
    bf16   K.dgemm on the packed bf16 weight             (+ its reduce, as the dgemm family runs it)

One JSON line per (projection, M): *_us the GEMM launch alone on an already quantised input,
*_step_us the projection as the decoder runs it (o: quantise the attention output, GEMM, reduce +
residual + RMSNorm (+ quantise); gate_up: GEMM, SwiGLU (+ quantise); down: GEMM, reduce + residual
+ RMSNorm (+ quantise); qkv: the GEMM, whose slabs the RoPE kernel reads).

    python scripts/probes/f8dgemm_probe.py [--out profiles/f8dgemm_probe.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from copilot_for_consensus_amd.ops import kernels as K  # noqa: E402
from qdgemm_probe import ROTATE_BYTES, timed  # noqa: E402  (same directory: hipGraph-captured, alternating, medians)

H, FFN, KV = 4096, 14336, 1024
PROJ = [("qkv", H + 2 * KV, H), ("o", H, H), ("gate_up", 2 * FFN, H), ("down", H, FFN)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/f8dgemm_probe.jsonl")
    ap.add_argument("--ms", nargs="+", type=int, default=[8, 16, 32, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f8dgemm_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev, out = "cuda", open(a.out, "w")
    for name, N, Kd in PROJ:
        wbf = torch.randn(N, Kd, device=dev).bfloat16() * 0.02
        w8, sw = K.quant_fp8_weight(wbf)
        n8, nbf = ROTATE_BYTES // (N * Kd) + 1, ROTATE_BYTES // (N * Kd * 2) + 1
        rows = [w8.clone() for _ in range(n8)]
        for M in a.ms:
            p8 = K.pack_f8dgemm_weight(w8, sw, m=M)
            p8s = [K.PackedWeightF8(p8.data.clone(), p8.scale, N, Kd, p8.bn) for _ in range(n8)]
            pk = K.pack_dgemm_weight(wbf, swiglu=name == "gate_up", m=M)
            pks = [K.PackedWeight(pk.data.clone(), N, Kd, pk.bn) for _ in range(nbf)]
            x = torch.randn(M, Kd, device=dev).bfloat16()
            xq = K.quant_fp8_rows(x)
            res, nw = torch.randn(M, N, device=dev).bfloat16(), torch.ones(N, device=dev).bfloat16()
            split = K.f8dgemm_config(M, N, Kd, p8.bn)[1]
            dbn, dsplit = K.dgemm_config(M, N, Kd, swiglu=name == "gate_up", bn=pk.bn)

            def f8(i):
                return K.f8dgemm(*xq, p8s[i % n8], "bf16") if name == "gate_up" else K.f8dgemm(*xq, p8s[i % n8], "part", split)

            def lib(i):
                return K.linear_fp8(xq, rows[i % n8], sw)

            def bf(i):
                epi = "swiglu" if name == "gate_up" else "bf16" if dsplit == 1 else "part"
                return K.dgemm(x, pks[i % nbf], epi, 1 if epi != "part" else dsplit, bn=dbn)

            def f8_step(i):
                if name == "qkv":
                    return f8(i)
                if name == "gate_up":
                    return K.silu_mul_fp8(f8(i), interleaved=True)
                q = K.quant_fp8_rows(x) if name == "o" else xq
                return K.splitk_residual_rmsnorm_fp8(K.f8dgemm(*q, p8s[i % n8], "part", split), res, nw, 1e-5)

            def lib_step(i):
                if name == "qkv":
                    return lib(i)
                if name == "gate_up":
                    return K.silu_mul_fp8(lib(i), interleaved=True)
                return K.rmsnorm_fp8(K.linear_fp8(x if name == "o" else xq, rows[i % n8], sw), nw, 1e-5, residual=res)

            def bf_step(i):
                if name == "qkv":
                    return bf(i)
                if name == "gate_up":
                    return K.dgemm_swiglu(x, pks[i % nbf])
                return K.dgemm_residual_rmsnorm(x, pks[i % nbf], res, nw, 1e-5)

            t = timed([f8, lib, bf, f8_step, lib_step, bf_step], a.iters, a.reps)
            row = {"proj": name, "M": M, "N": N, "K": Kd, "f8_cfg": [p8.bn, split], "bf16_cfg": [dbn, dsplit],
                   "f8_us": round(t[0], 2), "lib_us": round(t[1], 2), "bf16_us": round(t[2], 2),
                   "f8_TBs": round(N * Kd / t[0] / 1e6, 3), "lib_TBs": round(N * Kd / t[1] / 1e6, 3),
                   "bf16_TBs": round(2 * N * Kd / t[2] / 1e6, 3), "f8_step_us": round(t[3], 2),
                   "lib_step_us": round(t[4], 2), "bf16_step_us": round(t[5], 2)}
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
            del p8s, pks
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
