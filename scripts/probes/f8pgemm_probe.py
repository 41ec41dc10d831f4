#!/usr/bin/env python3
"""FP8 prefill GEMM probe (csrc/kernels/f8pgemm.hip): times Mistral-7B's four projections at
M = 16384, 2048 and 512 two ways in one process, on the same quantised operands, the two
alternating:

    f8p    K.f8pgemm on the packed FP8 weight (the decode GEMM's copy)
    lib    K.linear_fp8 (torch._scaled_mm, hipBLASLt) on the row-major FP8 weight

One JSON line per (projection, M): median us per call of each (hipGraph-captured, qdgemm_probe's
timed), the rate of each in TF/s (2 M N K flop), f8p_over_lib = f8p time / library time (below 1: the
kernel wins) and the largest difference of the two bf16 outputs relative to the largest output.

    python scripts/probes/f8pgemm_probe.py [--out profiles/f8pgemm_probe.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from copilot_for_consensus_amd.ops import kernels as K  # noqa: E402
from qdgemm_probe import timed  # noqa: E402  (same directory: hipGraph-captured, alternating, medians)

H, FFN, KV = 4096, 14336, 1024
PROJ = [("qkv", H + 2 * KV, H), ("o", H, H), ("gate_up", 2 * FFN, H), ("down", H, FFN)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/f8pgemm_probe.jsonl")
    ap.add_argument("--ms", nargs="+", type=int, default=[16384, 2048, 512])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f8pgemm_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev, out = "cuda", open(a.out, "w")
    for name, N, Kd in PROJ:
        w8, sw = K.quant_fp8_weight(torch.randn(N, Kd, device=dev).bfloat16() * 0.02)
        pw = K.pack_f8dgemm_weight(w8, sw)
        for M in a.ms:
            xq = K.quant_fp8_rows(torch.randn(M, Kd, device=dev).bfloat16())
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

            def f8p(i):
                return K.f8pgemm(*xq, pw, out=y)

            def lib(i):
                return K.linear_fp8(xq, w8, sw)

            diff = float((f8p(0).float() - lib(0).float()).abs().max() / lib(0).float().abs().max())
            t = timed([f8p, lib], a.iters, a.reps)
            row = {"proj": name, "M": M, "N": N, "K": Kd, "bn": pw.bn, "f8p_us": round(t[0], 2),
                   "lib_us": round(t[1], 2), "f8p_TFs": round(2 * M * N * Kd / t[0] / 1e6, 1),
                   "lib_TFs": round(2 * M * N * Kd / t[1] / 1e6, 1), "f8p_over_lib": round(t[0] / t[1], 3),
                   "max_diff_rel": diff}
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
        del w8, pw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
