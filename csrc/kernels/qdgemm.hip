// Batched decode GEMM straight from ggml-quantized blocks on gfx950: Y[M, N] = X[M, K] . dequant(W)^T,
// 1 <= M <= 128 rows of bf16 X, W a Q4_K / Q6_K / Q8_0 tensor in the planar GPU layouts of quant.hip
// (ops/kernels.py:_planar; the one resident quantized copy, shared with the M <= 4 quantized GEMV).
// A decode projection at these M is a weight stream: the quantized planes are 3.6x (Q4_K) / 2.4x
// (Q6_K) fewer bytes than the bf16 copy the decode GEMM (dgemm.hip) streams.
//
// Work split.  A workgroup of BN / 16 waves owns BN rows of W and one K part (grid.y = split, in
// whole 256-weight blocks, parts may differ by one block); wave w owns the 16 rows n0 + 16 w .. + 15
// for ALL ceil(M / 16) row tiles of X.  Per 256-weight block a lane (row i = lane & 15, k group
// g = lane >> 4) loads the bytes of chunks 2g and 2g + 1 of its row -- 32 contiguous nibble bytes
// (Q4_K / Q6_K) or 64 int8 (Q8_0), so the 64 lanes read 16 full 128-B (256-B) lines of the nibble
// plane -- plus the row's block header / scales, and builds eight MFMA A fragments of 8 weights
// from them in registers: fragment (s, j) holds weights 32 (2g + s) + 8j .. + 7 of the block (low
// nibbles of bytes 0-7, 8-15, then the high nibbles: every byte is loaded once and used twice).  The
// reduction over k is order-free, so MFMA (s, j) simply pairs those with the X fragment of the same
// k: X[m][256 b + 64 g + 32 s + 8 j .. + 7], 16 contiguous bytes of the block's X tile in LDS
// (row stride 528 B: the 16 rows of a ds_read_b128 land on 64 distinct banks).  X tiles are double
// buffered (global -> registers during the MFMAs of the previous block, one barrier per block); W
// for block b + 1 is in flight while block b is computed.
//
// MFMA 16x16x32 bf16, fp32 accumulate, A = W fragment, B = X fragment: a lane ends up with X row
// 16 t + (lane & 15) at the four consecutive W rows n0 + 16 w + 4 (lane >> 4) + r -- one 16-byte
// (fp32 slab) or 8-byte (bf16) store per row tile.
//
// Numeric scheme: (a) at every M.  Every weight is dequantized to the bf16 value dequant_bf16
// produces (fp32 d.sc.q - dmin.m, one RNE rounding to bf16) and multiplied on the MFMA, so a
// projection computes what the dequantized bf16 model computes up to fp32 summation order.  The
// VALU cost is constant in M: hipcc emits ~3.5 instructions per weight (nibble mask,
// v_cvt_f32_ubyte, half a v_pk_fma_f32, half a v_cvt_pk_bf16_f32).  Scheme (b) -- MFMA over the
// exact integer codes with d.sc / dmin.m applied to the accumulator per sub-block -- needs every MFMA
// to stay inside one 32-weight sub-block (each nibble byte loaded by two lanes, or a cross-lane
// exchange) and an accumulator fix-up that grows with M; it was NOT built, so no probe number
// compares the two and the choice of (a) is by construction cost, not by measurement.
//
// Measured on one MI355X (scripts/probes/qdgemm_probe.py, profiles/qdgemm_probe.jsonl and
// qdgemm_sweep.jsonl, ROOFLINE.md), Mistral-7B shapes: the kernel is bound by these instructions,
// not by HBM -- ~1.0 us per wave and 16 x 256 block for the dequantization plus ~0.34 us per 16
// rows of X (8 MFMAs + 8 ds_read_b128), i.e. 2-3 TB/s of quantized bytes at M <= 16 and ~1 TB/s at
// M = 128.  Against the bf16 decode GEMM the projections of one layer sum to 1.04x / 1.01x faster
// at M = 8 / 16 and 0.83x / 0.70x / 0.60x at M = 32 / 64 / 128, which is why the decoder sends only
// batches up to 16 rows here by default (ops/kernels.py: QDGEMM_DEFAULT_MAX_M).
//
// Outputs: fp32 split-K slabs [split][M][ldo] into a column range (q / k / v of different ggml
// types fill one buffer), optionally with gate / up rows interleaved 8 by 8 (W row j -> column
// 16 (j / 8) + j % 8, + 8 for up: interleave_gate_up's order, read by splitk_reduce's SwiGLU), or
// bf16 [M][ldo] at split 1.  Plain stores, no atomics: bit-reproducible from replay to replay.
#include "qblk.h"   // QBlk: a lane's share of one 256-weight block, shared with qunpack.hip

namespace {

enum { QD_PART = 0, QD_BF16 = 1 };
constexpr int QD_XROW = 33;   // uint4 per X row in LDS: 32 (256 bf16) + 1 pad

__device__ __forceinline__ f32x4_t qd_mfma(uint4 a, uint4 b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                 c, 0, 0, 0);
}

template <int T, int MT, int S, int J>
__device__ __forceinline__ void qd_step(const QBlk<T>& w, const uint4* xb, f32x4_t (&acc)[MT]) {
  const uint4 a = w.template frag<S, J>();
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = qd_mfma(a, xb[t * 16 * QD_XROW + 4 * S + J], acc[t]);
}

// MT: 16-row tiles of X (M <= 16 MT); NW: waves = 16-row tiles of W per workgroup.
template <int T, int MT, int NW>
__global__ void __launch_bounds__(NW * 64) qdgemm_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                         size_t o1, size_t o2, size_t o3, int M, int N, int K,
                                                         int split, int epi, int il, float* __restrict__ yf,
                                                         uint16_t* __restrict__ yb, long long slab, int ldo) {
  extern __shared__ uint4 xs[];
  constexpr int NT = NW * 64, XT = MT * 16 * QD_XROW;   // threads; uint4 per X buffer
  constexpr int CNT = MT * 16 * 32 / NT;                 // X uint4 per thread and block (MT * 8 / NW)
  static_assert(CNT * NT == MT * 16 * 32, "X tile must divide over the threads");
  const size_t off[3] = {o1, o2, o3};
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int nb = K / 256, p = blockIdx.y;
  const int b0 = p * nb / split, b1 = (p + 1) * nb / split;   // split <= nb <= K / 256: no overflow
  const int n0 = (blockIdx.x * NW + w) * 16;
  const bool live = n0 < N;
  const int row = min(n0, N - 16) + i;   // idle waves of the last workgroup stream a real tile (no branch)

  // X tile of block b: thread's e-th uint4 is row e / 32 (clamped to M - 1: rows past M are never
  // stored), 16-byte column e % 32
  int xg[CNT], xl[CNT];
#pragma unroll
  for (int e = 0; e < CNT; ++e) {
    const int idx = e * NT + tid, r = idx >> 5, c = idx & 31;
    xg[e] = min(r, M - 1) * (K / 8) + c;
    xl[e] = r * QD_XROW + c;
  }
  const uint4* X4 = reinterpret_cast<const uint4*>(X);
  uint4 xr[CNT];
  QBlk<T> cur, nxt;
  cur.load(W, off, row, b0, g, K);
#pragma unroll
  for (int e = 0; e < CNT; ++e) xr[e] = X4[xg[e] + 32 * b0];
#pragma unroll
  for (int e = 0; e < CNT; ++e) xs[xl[e]] = xr[e];
  __syncthreads();

  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int b = b0; b < b1; ++b) {
    const int bnx = min(b + 1, b1 - 1);
    nxt.load(W, off, row, bnx, g, K);
#pragma unroll
    for (int e = 0; e < CNT; ++e) xr[e] = X4[xg[e] + 32 * bnx];
    cur.prep(g);
    const uint4* xb = xs + ((b - b0) & 1) * XT + i * QD_XROW + 8 * g;
    qd_step<T, MT, 0, 0>(cur, xb, acc);
    qd_step<T, MT, 0, 1>(cur, xb, acc);
    qd_step<T, MT, 0, 2>(cur, xb, acc);
    qd_step<T, MT, 0, 3>(cur, xb, acc);
    qd_step<T, MT, 1, 0>(cur, xb, acc);
    qd_step<T, MT, 1, 1>(cur, xb, acc);
    qd_step<T, MT, 1, 2>(cur, xb, acc);
    qd_step<T, MT, 1, 3>(cur, xb, acc);
    // the other buffer's last readers finished before the previous iteration's barrier
    uint4* xw = xs + (((b - b0) + 1) & 1) * XT;
#pragma unroll
    for (int e = 0; e < CNT; ++e) xw[xl[e]] = xr[e];
    __syncthreads();
    cur = nxt;
  }
  if (!live) return;
  const int n = n0 + 4 * g;   // this lane's four consecutive W rows
  const int col = il == 0 ? n : 16 * (n >> 3) + (n & 7) + (il == 2 ? 8 : 0);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + i;
    if (m >= M) continue;
    if (epi == QD_PART)
      *reinterpret_cast<float4*>(yf + (size_t)p * slab + (size_t)m * ldo + col) =
          make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    else
      *reinterpret_cast<uint2*>(yb + (size_t)m * ldo + col) =
          make_uint2(pack2bf(acc[t][0], acc[t][1]), pack2bf(acc[t][2], acc[t][3]));
  }
}

struct QdArgs {
  const uint16_t* x;
  const uint8_t* w;
  size_t o1, o2, o3;
  int M, N, K, split, epi, il;
  float* yf;
  uint16_t* yb;
  long long slab;
  int ldo;
  hipStream_t st;
};

template <int T, int MT, int NW>
int qd_launch(const QdArgs& a) {
  const size_t lds = (size_t)2 * MT * 16 * QD_XROW * sizeof(uint4);
  const dim3 grid((a.N + NW * 16 - 1) / (NW * 16), a.split);
  qdgemm_kernel<T, MT, NW><<<grid, NW * 64, lds, a.st>>>(a.x, a.w, a.o1, a.o2, a.o3, a.M, a.N, a.K, a.split, a.epi,
                                                         a.il, a.yf, a.yb, a.slab, a.ldo);
  return CFC_CHECK_LAUNCH();
}

template <int T, int MT>
int qd_rows(const QdArgs& a, int bn) {
  // a thread stages MT * 8 / NW 16-byte pieces of X per block in registers: at most 16 (bn >= 8 MT)
  switch (bn) {
    case 16:
      if constexpr (MT <= 2) return qd_launch<T, MT, 1>(a);
      return -5;
    case 32:
      if constexpr (MT <= 4) return qd_launch<T, MT, 2>(a);
      return -5;
    case 64: return qd_launch<T, MT, 4>(a);
    case 128: return qd_launch<T, MT, 8>(a);
    default: return -5;
  }
}

template <int T>
int qd_tiles(const QdArgs& a, int bn) {
  if (a.M <= 16) return qd_rows<T, 1>(a, bn);
  if (a.M <= 32) return qd_rows<T, 2>(a, bn);
  if (a.M <= 64) return qd_rows<T, 4>(a, bn);
  return qd_rows<T, 8>(a, bn);
}

}  // namespace

// Y[M, N] = X[M, K] . W^T for ggml-quantized W in the planar GPU layouts of quant.hip, 1 <= M <= 128,
// N % 16 == 0, K % 256 == 0, type 12 / 14 / 8 (Q4_K / Q6_K / Q8_0).
//   w: the tensor's buffer (plane 0 at w, planes 1..3 at w + o1 / o2 / o3)
//   bn: W rows per workgroup (16 / 32 / 64 / 128, at least 8 per 16 rows of X); split: K parts, 1 .. K / 256
//   epi 0: fp32 slabs, part p's row m at yf + p * slab + m * ldo; epi 1 (split 1): bf16 rows at yb + m * ldo
//   il 0: W row j -> column j; 1 / 2: gate / up rows of an 8-row interleaved pair (column
//   16 (j / 8) + j % 8, + 8 for up).  yf / yb point at the first column of the range (16-B / 8-B aligned).
// Returns a negative code (nothing launched) for anything else.
CFC_API int cfc_qdgemm(const void* x, int M, int N, int K, int type, const void* w, long long o1, long long o2,
                       long long o3, int epi, int split, int bn, int il, float* yf, void* yb, long long slab, int ldo,
                       hipStream_t stream) {
  if (M < 1 || M > 128 || N <= 0 || N % 16 || K <= 0 || K % 256 || !w || !x) return -1;
  if (split < 1 || split > K / 256 || il < 0 || il > 2) return -3;
  if (epi == QD_PART ? !yf : (epi != QD_BF16 || !yb || split != 1)) return -2;
  if (ldo % 4 || slab % 4 || slab < 0 || ldo < (il ? 2 * N : N)) return -6;
  if (epi == QD_PART ? ((uintptr_t)yf & 15) : ((uintptr_t)yb & 7)) return -6;
  const QdArgs a{(const uint16_t*)x, (const uint8_t*)w, (size_t)o1, (size_t)o2, (size_t)o3, M, N, K, split, epi, il,
                 yf, (uint16_t*)yb, slab, ldo, stream};
  switch (type) {
    case QT_Q4K: return qd_tiles<QT_Q4K>(a, bn);
    case QT_Q6K: return qd_tiles<QT_Q6K>(a, bn);
    case QT_Q8_0: return qd_tiles<QT_Q8_0>(a, bn);
    default: return -4;
  }
}
