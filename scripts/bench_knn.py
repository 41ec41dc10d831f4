#!/usr/bin/env python3
"""BASELINE config 5 (retrieval half): a 100M x 384 bf16 cosine index resident in one MI355X's HBM
(77 GB of 288 GB), exact top-k by the fused MFMA scan + radix-select kernel (knn_topk_kernel: the
[nq, N] scores never reach HBM).  ``--ivf NLIST NPROBE``: the same index as IVF-flat over
clustered data (a Gaussian mixture, so lists mean something), k-means on a bf16 sample, one
fused launch per query batch; reports build time, ms per batch and recall@10 against the flat
scan.  ``--many``: batches of 17-128 queries through the many-query kernel, timed beside the loop of
16-query scans and the library GEMM + top-k (rows appended to ``--out``, default profiles/knn_many.jsonl).
``--vector-dtype both``: the int8 scalar-quantised flat index beside the bf16 one over the same clustered
rows (time, resident bytes, recall@10 of int8 against bf16; default ``--out`` profiles/knn_int8.jsonl).

The vectors are generated on the GPU (random, L2-normalised) straight into the index storage;
queries are batches of <= 16 (the scan kernel's query tile).  Reports scan bandwidth, query
latency and queries/s for top-k = 10 and 150 (the reporting service's limit*3, main.py:205)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from copilot_for_consensus_amd.vectorstore import HipFlatIndex  # noqa: E402


def bench_many(idx, n, dim, queries, out, iters=5):
    """``--many``: batches of 17-128 queries three ways in one process, alternating per iteration:
    the loop of 16-query fused scans, the library GEMM + K.topk over the [nq, N] score matrix, and
    the many-query kernel (K.knn_topk with the whole batch).  Median ms of ``iters`` device-event
    timings each; index_TBs = index bytes / time (what a single pass would stream)."""
    from copilot_for_consensus_amd.ops import kernels as K
    X = idx._X[:n]

    def loop16(Q, k):
        return [K.knn_topk(idx._X, Q[s:s + 16], k, N=n) for s in range(0, Q.shape[0], 16)]

    def gemm(Q, k):
        return K.topk((Q @ X.T).float().contiguous(), k)

    def many(Q, k):
        return K.knn_topk(idx._X, Q, k, N=n)

    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    paths = {"loop16": loop16, "gemm_topk": gemm, "many": many}
    with open(out, "a") as fh:
        for k in (10, 150):
            for nq in (17, 32, 64, 128):
                Q = queries(nq).bfloat16().contiguous()
                use = {name: f for name, f in paths.items() if name != "gemm_topk" or nq * n * 6 < 120e9}
                ms = {name: [] for name in use}
                for it in range(iters + 1):                  # iteration 0 warms every path up
                    for name, f in use.items():
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        f(Q, k)
                        b.record()
                        b.synchronize()
                        if it:
                            ms[name].append(a.elapsed_time(b))
                ref_i = torch.cat([i for _, i in loop16(Q, k)]).sort(1).values
                row = {"n": n, "dim": dim, "nq": nq, "k": k,
                       "same_ids_as_loop16": float((many(Q, k)[1].sort(1).values == ref_i).float().mean())}
                for name, t in ms.items():
                    med = sorted(t)[len(t) // 2]
                    row[name + "_ms"] = round(med, 3)
                    row[name + "_spread_ms"] = [round(min(t), 3), round(max(t), 3)]
                    row[name + "_index_TBs"] = round(n * dim * 2 / med / 1e9, 2)
                print(json.dumps(row), flush=True)
                fh.write(json.dumps(row) + "\n")
                fh.flush()


def bench_dtypes(n, dim, clusters, dtypes, out, iters=7):
    """``--vector-dtype``: the flat scan of an int8 index (knn8.hip) beside the bf16 one over the SAME
    rows (a Gaussian mixture, quantised from the bf16 rows) in one process, alternating per iteration.
    Median ms of ``iters`` device-event timings of idx.search (query preparation, scan and merge);
    index_TBs = the index's resident vector bytes / time; recall@10 of int8 against the bf16 result."""
    g = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.nn.functional.normalize(torch.randn(clusters, dim, device="cuda", generator=g), dim=1)
    idx = {d: HipFlatIndex(dim, device="cuda", capacity=n, vector_dtype=d) for d in dtypes}
    for s in range(0, n, 1 << 22):
        e = min(n, s + (1 << 22))
        v = centers[torch.randint(0, clusters, (e - s,), device="cuda", generator=g)] \
            + 0.02 * torch.randn(e - s, dim, device="cuda", generator=g)
        for ix in idx.values():
            rows, n2, sc = ix._prepare(v)
            ix._X[s:e], ix._norm2[s:e] = rows, n2
            if sc is not None:
                ix._scale[s:e] = sc
        del v
    for ix in idx.values():
        ix._alive[:n] = True
        ix._n = n
    nbytes = {d: n * dim * (1 if d == "int8" else 2) + (n * 4 if d == "int8" else 0) for d in dtypes}

    def queries(nq):
        c = centers[torch.randint(0, clusters, (nq,), device="cuda", generator=g)]
        return c + 0.02 * torch.randn(nq, dim, device="cuda", generator=g)

    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "a") as fh:
        for nq, k in ((1, 10), (1, 150), (16, 10), (16, 150)):
            Q = queries(nq)
            ms = {d: [] for d in dtypes}
            for it in range(iters + 2):                      # iterations 0 and 1 warm both paths up
                for d, ix in idx.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ix.search(Q, k)
                    b.record()
                    b.synchronize()
                    if it > 1:
                        ms[d].append(a.elapsed_time(b))
            row = {"n": n, "dim": dim, "nq": nq, "k": k}
            for d, t in ms.items():
                med = sorted(t)[len(t) // 2]
                row[d + "_ms"] = round(med, 3)
                row[d + "_spread_ms"] = [round(min(t), 3), round(max(t), 3)]
                row[d + "_index_TBs"] = round(nbytes[d] / med / 1e9, 2)
                row[d + "_resident_bytes"] = nbytes[d]
            print(json.dumps(row), flush=True)
            fh.write(json.dumps(row) + "\n")
            fh.flush()
        if len(dtypes) == 2:
            Q = queries(64)
            hits = 0
            for s in range(0, 64, 16):
                i8 = idx["int8"].search(Q[s:s + 16], 10)[1].cpu().tolist()
                ib = idx["bf16"].search(Q[s:s + 16], 10)[1].cpu().tolist()
                hits += sum(len(set(x) & set(y)) for x, y in zip(i8, ib))
            row = {"n": n, "dim": dim, "int8_recall_at_10_vs_bf16": round(hits / 640, 4)}
            print(json.dumps(row), flush=True)
            fh.write(json.dumps(row) + "\n")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--vector-dtype", choices=("bf16", "int8", "both"), default=None,
                    help="time the flat scan of an int8 index, a bf16 one, or both over the same clustered rows")
    ap.add_argument("n", nargs="?", type=float, default=100_000_000)
    ap.add_argument("--many", action="store_true", help="time batches of 17-128 queries three ways")
    ap.add_argument("--out", default="profiles/knn_many.jsonl", help="jsonl the --many rows are appended to")
    ap.add_argument("--ivf", type=int, nargs=2, metavar=("NLIST", "NPROBE"), default=None)
    ap.add_argument("--clusters", type=int, default=20000)
    args = ap.parse_args()
    n = int(args.n)
    dim = 384
    if args.vector_dtype:
        dtypes = ("bf16", "int8") if args.vector_dtype == "both" else (args.vector_dtype,)
        out = args.out if args.out != ap.get_default("out") else "profiles/knn_int8.jsonl"
        return bench_dtypes(n, dim, args.clusters, dtypes, out)
    if args.ivf:
        from copilot_for_consensus_amd.vectorstore import HipIVFIndex
        idx = HipIVFIndex(dim, "cosine", nlist=args.ivf[0], nprobe=args.ivf[1], device="cuda", capacity=n)
    else:
        idx = HipFlatIndex(dim, device="cuda", capacity=n)
    chunk = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.nn.functional.normalize(torch.randn(args.clusters, dim, device="cuda", generator=g), dim=1) \
        if args.ivf else None
    t = time.perf_counter()
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        v = torch.randn(e - s, dim, device="cuda", generator=g)
        if centers is not None:   # Gaussian mixture: a center + noise of ~0.35 of its norm
            v = centers[torch.randint(0, args.clusters, (e - s,), device="cuda", generator=g)] + 0.02 * v
        idx._X[s:e] = torch.nn.functional.normalize(v, dim=1).bfloat16()
        del v
    idx._norm2[:n] = 1.0
    idx._alive[:n] = True
    idx._n = n
    idx._ids = [None] * 0          # device-side search() only; ids are not materialised at this scale
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t
    res = {"vectors": n, "dim": dim, "index_bytes": n * dim * 2, "fill_s": round(build_s, 2)}
    if args.ivf:
        idx._ids = [None] * n          # regroup permutes ids: placeholders at this scale
        idx._meta = [None] * n
        t = time.perf_counter()
        idx.train(iters=8)
        torch.cuda.synchronize()
        res.update(ivf_nlist=idx.nlist, ivf_nprobe=idx.nprobe, ivf_train_s=round(time.perf_counter() - t, 2),
                   ivf_max_chunks=idx._maxc)
        print(f"ivf: nlist={idx.nlist} trained+regrouped in {res['ivf_train_s']} s", flush=True)

    def queries(nq):
        if centers is None:
            return torch.nn.functional.normalize(torch.randn(nq, dim, device="cuda", generator=g), dim=1)
        c = centers[torch.randint(0, args.clusters, (nq,), device="cuda", generator=g)]
        return torch.nn.functional.normalize(c + 0.02 * torch.randn(nq, dim, device="cuda", generator=g), dim=1)
    if args.many:
        return bench_many(idx, n, dim, queries, args.out)
    for nq, k in ((1, 10), (1, 150), (16, 10), (16, 150)):
        Q = queries(nq)
        for _ in range(2):
            idx.search(Q, k)
        torch.cuda.synchronize()
        it = 5
        t = time.perf_counter()
        for _ in range(it):
            v, i = idx.search(Q, k)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / it
        res[f"nq{nq}_k{k}"] = {"ms": round(dt * 1e3, 2), "qps": round(nq / dt, 1),
                               "scan_TBs": round(n * dim * 2 / dt / 1e12, 2)}
        print(f"nq={nq} k={k}: {dt*1e3:.2f} ms/batch, {nq/dt:.1f} qps, {n*dim*2/dt/1e12:.2f} TB/s", flush=True)
    if args.ivf:   # recall@10 of the IVF search against the exact flat scan of the same rows
        Q = queries(64)
        hits = 0
        for s in range(0, 64, 16):
            _, i_ivf = idx.search(Q[s:s + 16], 10)
            _, i_flat = HipFlatIndex.search(idx, Q[s:s + 16], 10, rows=(0, n))
            hits += sum(len(set(a) & set(b)) for a, b in zip(i_ivf.cpu().tolist(), i_flat.cpu().tolist()))
        res["ivf_recall_at_10"] = round(hits / 640, 4)
        print(f"ivf recall@10 vs flat: {res['ivf_recall_at_10']}", flush=True)
        out = "gpurun_out/bench_ivf.json"
    else:
        out = "gpurun_out/bench_knn.json"
    # exactness spot check on a slice against a plain fp32 matmul
    Q = torch.nn.functional.normalize(torch.randn(4, dim, device="cuda", generator=g), dim=1)
    m = min(n, 1 << 22)
    v, i = HipFlatIndex.search(idx, Q, 10, rows=(0, m))
    ref = torch.topk(Q @ idx._X[:m].float().T, 10, dim=1)
    res["exact_top10_overlap"] = float((i.cpu().sort(1).values == ref.indices.cpu().sort(1).values).float().mean())
    print(json.dumps(res), flush=True)
    os.makedirs("gpurun_out", exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
