// ggml-quantized planes -> the decode GEMM's fragment-packed bf16 layout, on gfx950.  A GGUF model
// kept resident in its quantized blocks only (DecoderWeights quant_only) re-fills one per-model bf16
// scratch from the blocks just before a consumer that has no quantized kernel reads it: the prefill
// GEMM (pgemm.hip) and decode batches past the quantized decode GEMM (dgemm.hip).
//
// Source: one QWeight [N, K] of type Q4_K / Q6_K / Q8_0 in the planar layouts of quant.hip
// (ops/kernels.py:_planar).  Destination: [N_total / bn][K / 32][bn / 16][64][8] bf16
// (ops/reference.py:pack_dgemm_weight): every 16-row x 32-k fragment is 1 KB, lane 16 q + r of it
// the 16 bytes of row r, k 8 q .. 8 q + 7.  The weight's row 0 lands at destination row row0 (q, k, v
// of different ggml types fill one qkv buffer in three launches); il 1 / 2 puts row j at
// 16 (j / 8) + j % 8 (+ 8 for up): gate and up fill one 8-row interleaved buffer in two launches.
//
// Mapping.  A wave owns 16 source rows and a range of 256-weight blocks and reads them exactly as
// qdgemm.hip does (QBlk, qblk.h): lane (i = lane & 15, g = lane >> 4) holds chunks 2g, 2g + 1 of
// row n0 + i, so the 64 lanes read whole 128-B lines of the nibble plane.  frag<S, J>() is the 8
// bf16 of k = 256 b + 64 g + 32 S + 8 J .. + 7: the 16-byte piece at lane position 16 J + i of the
// 32-k fragment 8 b + 2 g + S.  One store instruction (fixed S, J) therefore writes, per k group g,
// the 16 rows' pieces side by side -- four 256-byte runs (two whole 128-B lines each) in four
// fragments; with gate / up interleaving the 16 rows split into two 8-row halves of two 16-row
// groups, eight 128-byte runs (one whole line each).  After the eight stores of a block the wave has
// written eight complete 1-KB fragments.  Every run is line-aligned (row0 % 16 == 0), so no line is
// written partially; an LDS exchange that would let a wave store whole fragments was NOT built, so
// no number compares the two.
//
// Measured on one MI355X (scripts/probes/qunpack_probe.py, profiles/qunpack_probe.jsonl,
// ROOFLINE.md) against a device-to-device copy of the same destination bytes, Mistral-7B and
// Llama-3-70B projection shapes: Q4_K 0.87-1.35x the copy's speed (2.2-3.5 TB/s of destination
// bytes), Q6_K 0.79-1.17x, Q8_0 0.62-1.0x; the 33-50 MB shapes are the slow end.  One K part per
// row tile leaves the 256-tile shapes at 0.8-1.5 TB/s, 4-16 parts are within 10 % of each other
// (profiles/qunpack_splits.jsonl): the entry point splits K for ~8192 waves.
//
// Values: qd_deq8's fp32 fmaf and one RNE rounding -- the bits of dequant_bf16 (the products d.sc.q
// and dmin.m are exact in fp32, so the fused and the separate multiply / subtract agree).
#include "qblk.h"

namespace {

template <int T, int S, int J>
__device__ __forceinline__ void qu_store(const QBlk<T>& w, uint4* frag0, size_t fs) {
  frag0[(size_t)S * fs + 16 * J] = w.template frag<S, J>();
}

// grid.x: groups of four 16-row tiles (one per wave); grid.y: K parts in whole blocks.
template <int T>
__global__ void __launch_bounds__(256) qunpack_kernel(const uint8_t* __restrict__ W, size_t o1, size_t o2, size_t o3,
                                                      int N, int K, int split, int il, int row0, int bn,
                                                      uint16_t* __restrict__ dst) {
  const size_t off[3] = {o1, o2, o3};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = (blockIdx.x * 4 + w) * 16;
  if (n0 >= N) return;   // no barrier below
  const int nb = K / 256, p = blockIdx.y;
  const int b0 = p * nb / split, b1 = (p + 1) * nb / split;   // split <= nb: never empty
  const int j = n0 + i;
  const int R = row0 + (il == 0 ? j : 16 * (j >> 3) + (j & 7) + (il == 2 ? 8 : 0));
  const int tile = R / bn, wr = (R - tile * bn) >> 4, r = R & 15;
  const size_t fs = (size_t)(bn / 16) * 64;   // uint4 between consecutive 32-k fragments of a row group
  // lane position r of fragment (tile, kk = 0, wr); fragment kk is kk * fs further
  uint4* d = reinterpret_cast<uint4*>(dst) + ((size_t)tile * (K / 32) * (bn / 16) + wr) * 64 + r;

  QBlk<T> cur, nxt;
  cur.load(W, off, j, b0, g, K);
  for (int b = b0; b < b1; ++b) {
    nxt.load(W, off, j, min(b + 1, b1 - 1), g, K);
    cur.prep(g);
    uint4* f = d + (size_t)(8 * b + 2 * g) * fs;
    qu_store<T, 0, 0>(cur, f, fs);
    qu_store<T, 0, 1>(cur, f, fs);
    qu_store<T, 0, 2>(cur, f, fs);
    qu_store<T, 0, 3>(cur, f, fs);
    qu_store<T, 1, 0>(cur, f, fs);
    qu_store<T, 1, 1>(cur, f, fs);
    qu_store<T, 1, 2>(cur, f, fs);
    qu_store<T, 1, 3>(cur, f, fs);
    cur = nxt;
  }
}

template <int T>
int qu_launch(const uint8_t* w, size_t o1, size_t o2, size_t o3, int N, int K, int split, int il, int row0, int bn,
              uint16_t* dst, hipStream_t st) {
  const dim3 grid((N / 16 + 3) / 4, split);
  qunpack_kernel<T><<<grid, 256, 0, st>>>(w, o1, o2, o3, N, K, split, il, row0, bn, dst);
  return CFC_CHECK_LAUNCH();
}

}  // namespace

// dst rows [row0, row0 + N) (il 0) or the gate (il 1) / up (il 2) rows of [row0, row0 + 2 N) of a
// packed bf16 weight [N_total, K] for bn-row workgroups <- dequant(w), w a Q4_K / Q6_K / Q8_0 tensor
// [N, K] in the planar layouts (plane 0 at w, planes 1..3 at w + o1 / o2 / o3).
//   N % 16 == 0, K % 256 == 0, bn 128 / 112 / 96 / 64, N_total % bn == 0, row0 % 16 == 0
//   split: K parts per 16-row tile, 1 .. K / 256; 0 = enough parts for ~8 waves per SIMD
// Returns a negative code (nothing launched) for anything else.
CFC_API int cfc_qunpack(const void* w, int type, int N, int K, long long o1, long long o2, long long o3, void* dst,
                        int N_total, int row0, int bn, int il, int split, hipStream_t stream) {
  if (N <= 0 || N % 16 || K <= 0 || K % 256 || !w || !dst || ((uintptr_t)dst & 15)) return -1;
  if (bn != 128 && bn != 112 && bn != 96 && bn != 64) return -5;
  if (il < 0 || il > 2 || N_total <= 0 || N_total % bn || row0 < 0 || row0 % 16) return -3;
  if ((long long)row0 + (il ? 2LL * N : (long long)N) > N_total) return -6;
  const int nb = K / 256, tiles = N / 16;
  if (split < 0 || split > nb) return -3;
  if (split == 0) {
    split = (8192 + tiles - 1) / tiles;
    if (split > nb) split = nb;
  }
  uint16_t* d = (uint16_t*)dst;
  const uint8_t* s = (const uint8_t*)w;
  switch (type) {
    case QT_Q4K: return qu_launch<QT_Q4K>(s, o1, o2, o3, N, K, split, il, row0, bn, d, stream);
    case QT_Q6K: return qu_launch<QT_Q6K>(s, o1, o2, o3, N, K, split, il, row0, bn, d, stream);
    case QT_Q8_0: return qu_launch<QT_Q8_0>(s, o1, o2, o3, N, K, split, il, row0, bn, d, stream);
    default: return -4;
  }
}
