// Int8 scalar-quantised flat index: the row quantiser and the fused scan + top-k on the int8 MFMA
// (v_mfma_i32_16x16x64_i8).  The counterpart of Qdrant's scalar int8 quantisation and FAISS
// IndexScalarQuantizer QT_8bit, with one fp32 scale per row: a row is code[dim] int8 + scale, and
// decodes to code * scale.  Half the bytes per row of the bf16 index (knn.hip), so half the HBM
// traffic of a scan that is bound by it.
//
//   * cfc_quant_i8_rows: bf16 rows -> codes, scale, decoded squared norm, one wave per row.
//   * cfc_knn8_topk: rows [row_lo, N) against <= 16 int8 queries; k <= 256 candidates per query
//     and span leave the CUs ([nq][spans][k], merged by cfc_topk_pass).  The i32 dot product is
//     exact (dim <= 1024: |dot| < 2^24, so its fp32 image is exact too); the score is
//     (float(dot) * qscale[q]) * xscale[row], or -(xnorm2 + qnorm2 - 2 score) with norms.
#include "common.h"
#include "knn_select.h"

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ i32x4_t as_i32x4(uint4 v) { return __builtin_bit_cast(i32x4_t, v); }

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------ quantiser
// One wave per row, the row in registers: lane l holds the 16-element pieces l + 64 j (two 16-byte
// loads each), so one pass over HBM serves the amax reduce, the quantisation, the integer sum of
// squares and the 16-byte code stores.  NJ = 1 covers dim <= 1024, NJ = 4 dim <= 4096.
template <int NJ>
__global__ void __launch_bounds__(256) quant_i8_rows_kernel(int8_t* __restrict__ codes, float* __restrict__ scale,
                                                            float* __restrict__ norm2,
                                                            const uint16_t* __restrict__ x, int rows, int dim,
                                                            int normalize) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                       // wave-uniform
  const int npiece = dim / 16;
  const uint16_t* xr = x + (size_t)row * dim;
  float v[NJ][16];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = lane + 64 * j;
    if (p < npiece) {
      unpack8(*reinterpret_cast<const uint4*>(xr + 16 * p), v[j]);
      unpack8(*reinterpret_cast<const uint4*>(xr + 16 * p + 8), v[j] + 8);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[j][e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(v[j][e]));
  }
  amax = wave_max(amax);
  const float inv = amax > 0.f ? 127.f / amax : 0.f;
  int ss = 0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = lane + 64 * j;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = (int)fminf(fmaxf(rintf(v[j][e] * inv), -127.f), 127.f);   // rint: ties to even
      ss += c * c;
      w[e >> 2] |= (uint32_t)(c & 0xff) << (8 * (e & 3));
    }
    if (p < npiece) *reinterpret_cast<uint4*>(codes + (size_t)row * dim + 16 * p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  ss = wave_sum_i32(ss);                          // <= 4096 * 127^2 < 2^31
  if (lane == 0) {
    const float S = (float)ss;
    const float sc = amax > 0.f ? (normalize ? 1.f / sqrtf(S) : amax / 127.f) : 0.f;
    scale[row] = sc;
    norm2[row] = amax > 0.f ? (normalize ? 1.f : S * sc * sc) : 0.f;
  }
}

// ------------------------------------------------------------------ scan + top-k
// One kernel for every (nq <= 16, k <= 256).  grid = spans, one 4-wave workgroup walks one span of
// rows in rounds of K8_ROUND(KC) = 64 G rows (G = k8_groups(KC) 16-row groups per wave per round).
//
//   * The query B fragments (16 bytes per lane per 64-wide k-step: lane (col, g) holds bytes
//     64 c + 16 g .. + 15 of query col) stay in registers for the whole span: 4 KC VGPRs, 24 at dim
//     384.  A fragments come straight from HBM with the same byte offsets of row r0 + col, so
//     whatever k-order the instruction gives a lane's 16 bytes, A and B agree on it.  A wave issues
//     every load of its G groups (16 G KC bytes per lane: 1.5 KB at dim 384, 6 KB per wave) plus
//     the groups' row scales before the first MFMA.
//   * Accumulator element i of lane (col, g) is row 4 g + i of the group against query col.  Every
//     row gets the contract score (two fp32 multiplies; with norms the L2 form, the row norm loaded
//     with the scale), as an order-preserving u32 key.  A key above the query's running
//     threshold takes a slot (LDS atomic) in the query's candidate buffer: cap entries of (u32 key,
//     u16 row-in-span).  Only such a row's alive byte is read: after the first rounds of a span a
//     few rows per round pass, so the alive array costs next to nothing instead of 1 B per 384.
//   * No [nq][rows] score tile in LDS and no select per round.  A round ends in ONE barrier; the
//     lane whose slot crosses cap - ROUND raises a flag (two flags, by round parity, so a wave that
//     is already appending the next round's rows cannot change what a slower wave reads), and only
//     then the waves cut the over-full buffers to their exact top k with ks_cut, raise the
//     thresholds to the k-th key and meet at a second barrier.  A round adds at most ROUND entries
//     to a buffer and a cut leaves k <= cap - ROUND, so a slot is always free: no candidate is
//     dropped whatever the order of the data.  Keys equal to the threshold after a cut are
//     skipped: k keys >= it are held, so the result is exact up to tie order.
//   * LDS: nq x cap x 6 B + 192 B, cap = k + ROUND rounded up to 64 (<= 512): 16 queries, k = 10,
//     dim 384: 30 KB; k = 256: 48 KB; 1 query: <= 3 KB.  VGPRs: A 16 G KC / 4 = 96 at dim 384 / 768,
//     64 at 1024, + 4 KC for B + 8 G scale / norm; the compiler reports 186 at dim 384 (no scratch):
//     2 waves per SIMD, so 2 workgroups per CU with 48 KB of index loads in flight, and the LDS
//     never limits.  The CU's other workgroup covers the drain at a round's barrier.
//   * Clocks per 16-row group at dim 384 (6 KB = 600 clk of a CU's 10 B/clk HBM share): 6 MFMAs x
//     8 passes x 4 clk = 192 clk on one of four SIMDs; keys + compares for 4 scores per lane ~ 40
//     VALU clk.  The stream bounds it: measured 100M x 384 in 6.4 ms = 6.05 TB/s for 1 and for 16
//     queries at k = 10, the rate of the 1-query bf16 scan (profiles/ROOFLINE.md).
//   * Span (k8_plan): rows / 2048 so that >= 4 workgroups per CU exist from 1M rows up, at least
//     max(1024, 32 k) rows so that the k candidates a span emits stay under ~3 % of its rows, at
//     most 65536 (row-in-span is u16).  At 1M rows, k <= 32: 1024 workgroups; k = 256: 128.
constexpr int K8_MAXSPAN = 65536;
constexpr int k8_groups(int kc) { return kc <= 6 ? 4 : kc <= 8 ? 3 : kc <= 12 ? 2 : 1; }
constexpr int k8_round(int kc) { return 64 * k8_groups(kc); }

__device__ __forceinline__ uint32_t k8_cut(uint32_t* bk, uint16_t* br, int cnt, int kk, int cap) {
  switch (cap >> 6) {
    case 1: return ks_cut<1>(bk, br, cnt, kk);
    case 2: return ks_cut<2>(bk, br, cnt, kk);
    case 3: return ks_cut<3>(bk, br, cnt, kk);
    case 4: return ks_cut<4>(bk, br, cnt, kk);
    case 5: return ks_cut<5>(bk, br, cnt, kk);
    case 6: return ks_cut<6>(bk, br, cnt, kk);
    case 7: return ks_cut<7>(bk, br, cnt, kk);
    default: return ks_cut<8>(bk, br, cnt, kk);   // k8_plan: cap <= 512
  }
}

template <int KC>  // KC = dim / 64 MFMA k-steps
__global__ void __launch_bounds__(256) knn8_topk_kernel(const int8_t* __restrict__ X, const float* __restrict__ xscale,
                                                        const int8_t* __restrict__ Q, const float* __restrict__ qscale,
                                                        int N, int nq, const float* __restrict__ xnorm2,
                                                        const float* __restrict__ qnorm2,
                                                        const uint8_t* __restrict__ alive, int k, int row_lo, int span,
                                                        int cap, float* __restrict__ out_v, int64_t* __restrict__ out_i) {
  constexpr int D = KC * 64, G = k8_groups(KC), ROUND = k8_round(KC);
  extern __shared__ __attribute__((aligned(16))) char k8_smem[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(k8_smem);            // [16]
  uint32_t* thr = cnt + 16;                                         // [16]
  uint32_t* flag = thr + 16;                                        // [2] (+ padding to 192 B)
  uint32_t* bk = cnt + 48;                                          // [nq][cap]
  uint16_t* br = reinterpret_cast<uint16_t*>(bk + nq * cap);        // [nq][cap]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int lo = row_lo + blockIdx.x * span, hi = min(N, lo + span);
  const bool qv = col < nq;
  if (threadIdx.x < 48) cnt[threadIdx.x] = 0u;                      // counts, thresholds, flags

  i32x4_t qf[KC];
  {
    const int8_t* qr = Q + (size_t)(qv ? col : 0) * D + 16 * g;
#pragma unroll
    for (int c = 0; c < KC; ++c)
      qf[c] = as_i32x4(qv ? *reinterpret_cast<const uint4*>(qr + 64 * c) : make_uint4(0, 0, 0, 0));
  }
  const float qs = qv ? qscale[col] : 0.f;
  const float qn = (qnorm2 && qv) ? qnorm2[col] : 0.f;
  const int limit = cap - ROUND;                                    // >= k
  __syncthreads();

  const int nrounds = (hi - lo + ROUND - 1) / ROUND;
  for (int r = 0; r < nrounds; ++r) {
    const uint32_t th = qv ? thr[col] : 0xffffffffu;
    const int base = lo + r * ROUND + w * (16 * G);                 // this wave's G groups
    uint4 a[G][KC];
    float xs[G][4], xn[G][4];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      // rows past the span's end re-read row hi - 1 (never scored): no read goes past N
      const int8_t* xr = X + (size_t)min(base + 16 * j + col, hi - 1) * D + 16 * g;
#pragma unroll
      for (int c = 0; c < KC; ++c) a[j][c] = *reinterpret_cast<const uint4*>(xr + 64 * c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = min(base + 16 * j + 4 * g + i, hi - 1);
        xs[j][i] = xscale[row];
        xn[j][i] = xnorm2 ? xnorm2[row] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      i32x4_t acc = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < KC; ++c) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(as_i32x4(a[j][c]), qf[c], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = base + 16 * j + 4 * g + i;
        float v = ((float)acc[i] * qs) * xs[j][i];
        if (xnorm2) v = -(xn[j][i] + qn - 2.f * v);
        const uint32_t key = f2key(v);
        if (row < hi && key > th && (!alive || alive[row])) {       // th = ~0 for the padding columns
          const uint32_t slot = atomicAdd(&cnt[col], 1u);
          if (slot < (uint32_t)cap) {                               // always: see the header
            bk[col * cap + slot] = key;
            br[col * cap + slot] = (uint16_t)(row - lo);
          }
          if (slot == (uint32_t)limit) flag[r & 1] = 1u;            // this buffer may not hold another round
        }
      }
    }
    __syncthreads();                                                // the round's appends are visible
    if (flag[r & 1]) {                                              // workgroup-uniform
      for (int qi = w; qi < nq; qi += 4) {
        const int n = min(__builtin_amdgcn_readfirstlane((int)cnt[qi]), cap);
        if (n > limit) {
          const uint32_t t = k8_cut(bk + qi * cap, br + qi * cap, n, k, cap);
          if (lane == 0) { thr[qi] = t; cnt[qi] = (uint32_t)k; }
        }
      }
      __syncthreads();                                              // cuts done, thresholds visible
      if (threadIdx.x == 0) flag[r & 1] = 0u;                       // next written two rounds on
    }
  }
  for (int qi = w; qi < nq; qi += 4) {
    uint32_t* qk = bk + qi * cap;
    uint16_t* qr = br + qi * cap;
    int n = min(__builtin_amdgcn_readfirstlane((int)cnt[qi]), cap);
    if (n > k) {
      k8_cut(qk, qr, n, k, cap);
      n = k;
    }
    const size_t o = ((size_t)qi * gridDim.x + blockIdx.x) * k;
    for (int s = lane; s < k; s += 64) {
      out_v[o + s] = s < n ? key2f(qk[s]) : -INFINITY;
      out_i[o + s] = s < n ? (int64_t)lo + qr[s] : -1;
    }
  }
}

struct K8Plan { int span, cap, nspans; };

// Span, candidate slots per query and spans of knn8_topk_kernel (its header has the reasoning).
bool k8_plan(int nq, int k, int dim, long rows, K8Plan* p) {
  const int kc = dim / 64;
  if (dim % 64 != 0 || (kc != 2 && kc != 4 && kc != 6 && kc != 8 && kc != 12 && kc != 16)) return false;
  if (nq < 1 || nq > 16 || k < 1 || k > 256 || rows < 1) return false;
  long span = (rows + 2047) / 2048;
  const long lo = 32L * k > 1024 ? 32L * k : 1024;
  span = span < lo ? lo : span > K8_MAXSPAN ? K8_MAXSPAN : span;
  span = (span + 63) / 64 * 64;
  const int cap = (k + k8_round(kc) + 63) / 64 * 64;
  *p = K8Plan{(int)span, cap, (int)((rows + span - 1) / span)};
  return true;
}

}  // namespace

// x bf16 [rows][dim] -> codes int8 [rows][dim], scale [rows], norm2 [rows] (of the decoded row).
// code = clamp(rint(x * (127 / amax)), -127, 127); normalize = 0: scale = amax / 127; normalize = 1
// (cosine): scale = 1 / sqrt(sum code^2), the decoded row has unit length.  A zero row: all zeros.
CFC_API int cfc_quant_i8_rows(void* codes, float* scale, float* norm2, const void* x, int rows, int dim, int normalize,
                              hipStream_t stream) {
  if (dim < 16 || dim % 16 != 0 || dim > 4096 || rows < 0) return -1;
  if (rows == 0) return 0;
  const int blocks = (rows + 3) / 4;
  if (dim <= 1024)
    quant_i8_rows_kernel<1><<<blocks, 256, 0, stream>>>((int8_t*)codes, scale, norm2, (const uint16_t*)x, rows, dim,
                                                        normalize);
  else
    quant_i8_rows_kernel<4><<<blocks, 256, 0, stream>>>((int8_t*)codes, scale, norm2, (const uint16_t*)x, rows, dim,
                                                        normalize);
  return CFC_CHECK_LAUNCH();
}

// Plan of cfc_knn8_topk: out = {span rows, candidate slots per query, spans}.
CFC_API int cfc_knn8_plan(int nq, int k, int dim, int64_t rows, int* out) {
  K8Plan p;
  if (!k8_plan(nq, k, dim, (long)rows, &p)) return -1;
  out[0] = p.span; out[1] = p.cap; out[2] = p.nspans;
  return 0;
}

// Int8 flat index, rows [row_lo, N), nq <= 16, k <= 256, dim in {128, 256, 384, 512, 768, 1024}.
// Candidates out [nq][spans][k] (spans from cfc_knn8_plan(nq, k, dim, N - row_lo); unsorted, -inf /
// -1 padding; merge with cfc_topk_pass).  Dead rows (alive == 0) are never candidates.
CFC_API int cfc_knn8_topk(const void* X8, const float* xscale, const void* Q8, const float* qscale, int N, int row_lo,
                          int nq, int dim, const float* xnorm2, const float* qnorm2, const uint8_t* alive, int k,
                          float* out_v, int64_t* out_i, hipStream_t stream) {
  K8Plan p;
  if (row_lo < 0 || N <= row_lo || !k8_plan(nq, k, dim, (long)N - row_lo, &p)) return -1;
  const size_t lds = 192 + (size_t)nq * p.cap * 6;
#define K8(KC) \
  case KC: \
    knn8_topk_kernel<KC><<<p.nspans, 256, lds, stream>>>((const int8_t*)X8, xscale, (const int8_t*)Q8, qscale, N, nq, \
                                                         xnorm2, qnorm2, alive, k, row_lo, p.span, p.cap, out_v, out_i); \
    return CFC_CHECK_LAUNCH();
  switch (dim / 64) {
    K8(2) K8(4) K8(6) K8(8) K8(12) K8(16)
    default: return -2;
  }
#undef K8
}
