#!/usr/bin/env python3
"""Unpack probe (csrc/kernels/qunpack.hip): times the unpack of every projection shape of
Mistral-7B and Llama-3-70B from Q4_K / Q6_K / Q8_0 planes into the decode GEMM's packed bf16
layout -- as DecoderModel._scratch_weight runs it: q, k, v in three launches, gate and up in two,
into ONE destination -- against a device-to-device copy of the same destination bytes in the same
process, the two alternating.  The sources (quantized planes, and the copy's bf16 source) rotate
over > 600 MB so every call streams from HBM (QWeight.random: needs no file).  One JSON line per
(model, projection, type):

    unpack_us, dst_TBs     the unpack launches and the destination bytes over their time
    copy_us, copy_TBs      torch's d2d copy of as many bytes into the same destination
    vs_copy                copy_us / unpack_us (1.0 = the unpack writes as fast as a copy)

    python scripts/probes/qunpack_probe.py [--out profiles/qunpack_probe.jsonl] [--splits 1 2 4 8 16]

--splits times the kernel's K split (parts per 16-row tile) instead of its own pick.
"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from copilot_for_consensus_amd.ops import kernels as K  # noqa: E402
from copilot_for_consensus_amd.runtime import gguf as G  # noqa: E402
from qdgemm_probe import ROTATE_BYTES, timed  # noqa: E402

# hidden, ffn, q rows, kv rows
MODELS = {"mistral-7b": (4096, 14336, 4096, 1024), "llama-3-70b": (8192, 28672, 8192, 1024)}
TYPES = {"q4_k": 12, "q6_k": 14, "q8_0": 8}


def projections(h, ffn, qs, ks):
    """(name, [(rows, row0 or interleave)], N_total, K, swiglu)"""
    return [("qkv", [(qs, 0), (ks, qs), (ks, qs + ks)], qs + 2 * ks, h, False), ("o", [(h, 0)], h, qs, False),
            ("gate_up", [(ffn, "gate"), (ffn, "up")], 2 * ffn, h, True), ("down", [(h, 0)], h, ffn, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/qunpack_probe.jsonl")
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--types", nargs="+", default=list(TYPES))
    ap.add_argument("--splits", nargs="+", type=int, default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qunpack_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev = "cuda"
    out = open(a.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()

    for model in a.models:
        for name, parts, N, Kd, swiglu in projections(*MODELS[model]):
            bn = K.dgemm_config(128, N, Kd, swiglu=swiglu)[0]        # pack_decode()'s tile width
            dst = K.PackedWeight(torch.empty(N * Kd, dtype=torch.bfloat16, device=dev), N, Kd, bn)
            dbytes = N * Kd * 2
            nsrc = max(2, ROTATE_BYTES // dbytes + 1)
            srcs = [torch.randn(N * Kd // 2, device=dev).view(torch.bfloat16) for _ in range(nsrc)]
            for tname in a.types:
                t = TYPES[tname]
                qbytes = N * Kd // G.BLOCK[t][0] * G.BLOCK[t][1]
                ncopy = min(64, max(2, ROTATE_BYTES // qbytes + 1))
                base = [K.QWeight.random(t, n, Kd, dev) for n, _ in parts]
                qws = [[dataclasses.replace(q, buf=q.buf.clone()) for q in base] for _ in range(ncopy)]

                def unpack(i, split=0):
                    for q, (_, where) in zip(qws[i % ncopy], parts):
                        if isinstance(where, str):
                            K.qunpack(q, dst, interleave=where, split=split)
                        else:
                            K.qunpack(q, dst, row0=where, split=split)

                def copy(i):
                    dst.data.copy_(srcs[i % nsrc])

                row = {"model": model, "proj": name, "type": tname, "N": N, "K": Kd, "bn": bn,
                       "q_MB": round(qbytes / 1e6, 2), "dst_MB": round(dbytes / 1e6, 2)}
                if a.splits:
                    for s in a.splits:
                        if s > Kd // 256:
                            continue
                        us, = timed([lambda i, s=s: unpack(i, s)], a.iters, 3)
                        emit(dict(row, split=s, unpack_us=round(us, 2), dst_TBs=round(dbytes / us / 1e6, 3)))
                else:
                    u_us, c_us = timed([unpack, copy], a.iters, a.reps)
                    emit(dict(row, unpack_us=round(u_us, 2), dst_TBs=round(dbytes / u_us / 1e6, 3),
                              copy_us=round(c_us, 2), copy_TBs=round(dbytes / c_us / 1e6, 3),
                              vs_copy=round(c_us / u_us, 3)))
                del qws, base
            del srcs, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
