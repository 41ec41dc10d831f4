#!/usr/bin/env python3
"""MXFP4 prefill GEMM probe (csrc/kernels/mx4pgemm.hip): times Mistral-7B's four projections at
M = 16384, 2048, 512 and 256 three ways in one process, the three alternating:

    mx4p    K.mx4pgemm on the packed MXFP4 weight (the decode GEMM's copy)
    slices  K.linear_mxfp4(..., tiled=False) on the same pair: 128-row slices of the decode kernel
    f8p     K.f8pgemm on an FP8 quantisation of the same bf16 weight

One JSON line per (projection, M): median us per call of each (hipGraph-captured, qdgemm_probe's
timed), mx4p's rate in TF/s (2 M N K flop), mx4p_over_slices and mx4p_over_f8p (below 1: the kernel
wins) and the largest difference of mx4p and slices relative to the largest output.

    python scripts/probes/mx4pgemm_probe.py [--out profiles/mx4pgemm_probe.jsonl]
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
    ap.add_argument("--out", default="profiles/mx4pgemm_probe.jsonl")
    ap.add_argument("--ms", nargs="+", type=int, default=[16384, 2048, 512, 256])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx4pgemm_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev, out = "cuda", open(a.out, "w")
    for name, N, Kd in PROJ:
        w = torch.randn(N, Kd, device=dev).bfloat16() * 0.02
        pw = K.pack_mx4dgemm_weight(*K.quant_mxfp4_weight(w))
        p8 = K.pack_f8dgemm_weight(*K.quant_fp8_weight(w))
        del w
        for M in a.ms:
            xq = K.quant_fp8_rows(torch.randn(M, Kd, device=dev).bfloat16())
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

            def mx4p(i):
                return K.mx4pgemm(*xq, pw, out=y)

            def slices(i):
                return K.linear_mxfp4(xq, pw, tiled=False)

            def f8p(i):
                return K.f8pgemm(*xq, p8, out=y)

            ref = slices(0).float()
            diff = float((mx4p(0).float() - ref).abs().max() / ref.abs().max())
            t = timed([mx4p, slices, f8p], a.iters, a.reps)
            row = {"proj": name, "M": M, "N": N, "K": Kd, "bn": pw.bn, "mx4p_us": round(t[0], 2),
                   "slices_us": round(t[1], 2), "f8p_us": round(t[2], 2),
                   "mx4p_TFs": round(2 * M * N * Kd / t[0] / 1e6, 1), "mx4p_over_slices": round(t[0] / t[1], 3),
                   "mx4p_over_f8p": round(t[0] / t[2], 3), "max_diff_rel": diff}
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
        del pw, p8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
