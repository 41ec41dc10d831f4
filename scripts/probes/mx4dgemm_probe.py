#!/usr/bin/env python3
"""MXFP4 decode GEMM probe (csrc/kernels/mx4dgemm.hip): times Mistral-7B's four decode projections at
M = 1, 16, 64, 128 three ways in one process, the three alternating, weights rotated over > 600 MB
so every call streams from HBM:

    mx4    K.mx4dgemm on the packed MXFP4 weight   (17/32 byte per weight)
    f8     K.f8dgemm on the packed FP8 weight      (1 byte)
    bf16   K.dgemm on the packed bf16 weight       (2 bytes)

each at the (bn, split) its cost model picks, the GEMM launch alone on an already quantised input
(fp32 slabs, or bf16 at split 1).  With --sweep the MXFP4 kernel is also timed at every bn it is
built for and the splits in --splits; "tried" lists [bn, split, us] of each.  One JSON line per
(projection, M): *_us medians over hipGraph replays, *_TBs the weight bytes of that format over
that time.

    python scripts/probes/mx4dgemm_probe.py [--sweep] [--out profiles/mx4dgemm_probe.jsonl]
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
    ap.add_argument("--out", default="profiles/mx4dgemm_probe.jsonl")
    ap.add_argument("--ms", nargs="+", type=int, default=[1, 16, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--splits", nargs="+", type=int, default=[1, 2, 4, 8])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx4dgemm_probe needs the GPU")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    dev, out = "cuda", open(a.out, "w")
    for name, N, Kd in PROJ:
        wbf = torch.randn(N, Kd, device=dev).bfloat16() * 0.02
        w8, sw = K.quant_fp8_weight(wbf)
        codes, scales = K.quant_mxfp4_weight(wbf)
        wbytes = {"mx4": N * Kd * K.MX4_BYTES_PER_WEIGHT, "f8": N * Kd, "bf16": 2 * N * Kd}
        copies = {k: int(ROTATE_BYTES // v) + 1 for k, v in wbytes.items()}

        def mx4_copies(bn):
            p = K.pack_mx4dgemm_weight(codes, scales, bn=bn)
            return [K.PackedWeightMX4(p.data.clone(), N, Kd, bn) for _ in range(copies["mx4"])]

        for M in a.ms:
            x = torch.randn(M, Kd, device=dev).bfloat16()
            xq = K.quant_fp8_rows(x)
            mbn, msplit = K.mx4dgemm_config(M, N, Kd)
            p4s = mx4_copies(mbn)
            p8 = K.pack_f8dgemm_weight(w8, sw, m=M)
            p8s = [K.PackedWeightF8(p8.data.clone(), p8.scale, N, Kd, p8.bn) for _ in range(copies["f8"])]
            fsplit = K.f8dgemm_config(M, N, Kd, p8.bn)[1]
            pk = K.pack_dgemm_weight(wbf, m=M)
            pks = [K.PackedWeight(pk.data.clone(), N, Kd, pk.bn) for _ in range(copies["bf16"])]
            dbn, dsplit = K.dgemm_config(M, N, Kd, bn=pk.bn)

            def mx4_at(ws, split):
                return lambda i: (K.mx4dgemm(*xq, ws[i % len(ws)], "bf16") if split == 1
                                  else K.mx4dgemm(*xq, ws[i % len(ws)], "part", split))

            def f8(i):
                return K.f8dgemm(*xq, p8s[i % len(p8s)], "bf16") if fsplit == 1 else K.f8dgemm(*xq, p8s[i % len(p8s)], "part", fsplit)

            def bf(i):
                return K.dgemm(x, pks[i % len(pks)], "bf16" if dsplit == 1 else "part", dsplit, bn=dbn)

            t = timed([mx4_at(p4s, msplit), f8, bf], a.iters, a.reps)
            row = {"proj": name, "M": M, "N": N, "K": Kd, "mx4_cfg": [mbn, msplit], "f8_cfg": [p8.bn, fsplit],
                   "bf16_cfg": [dbn, dsplit], "mx4_us": round(t[0], 2), "f8_us": round(t[1], 2), "bf16_us": round(t[2], 2),
                   "mx4_TBs": round(wbytes["mx4"] / t[0] / 1e6, 3), "f8_TBs": round(wbytes["f8"] / t[1] / 1e6, 3),
                   "bf16_TBs": round(wbytes["bf16"] / t[2] / 1e6, 3)}
            del p8s, pks
            if a.sweep:
                row["tried"] = []
                for bn in K.MX4DGEMM_BNS:
                    ws = p4s if bn == mbn else mx4_copies(bn)
                    splits = [s for s in a.splits if s <= Kd // 128]
                    for s, us in zip(splits, timed([mx4_at(ws, s) for s in splits], a.iters, a.reps)):
                        row["tried"].append([bn, s, round(us, 2)])
                    del ws
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
            del p4s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
