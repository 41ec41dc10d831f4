// Top-k selection helpers shared by the bf16 (knn.hip) and int8 (knn8.hip) index scans: the
// order-preserving float <-> u32 key, and the wave-level cut of a candidate buffer to its exact top k.
#pragma once
#include "common.h"

__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// keys held NJ per lane (entry lane + 64 j; 0 = empty): the exact kk-th largest
template <int NJ>
__device__ __forceinline__ uint32_t ks_kth(const uint32_t* key, int kk) {
  uint32_t thr = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t cand = thr | (1u << b);
    int c = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) c += __popcll(__ballot(key[j] >= cand));
    if (c >= kk) thr = cand;                 // wave-uniform decision
  }
  return thr;
}

// Cut a query's buffer (kk < cnt <= 64 NJ entries; rows as RT) to its exact top kk, in place
// (wave-level; every entry is in registers before the first write).  Returns the kk-th largest
// key (the new threshold).
template <int NJ, typename RT>
__device__ __forceinline__ uint32_t ks_cut(uint32_t* bk, RT* br, int cnt, int kk) {
  const int lane = threadIdx.x & 63;
  uint32_t key[NJ];
  RT row[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = lane + 64 * j;
    key[j] = i < cnt ? bk[i] : 0u;
    row[j] = i < cnt ? br[i] : (RT)0;
  }
  const uint32_t thr = ks_kth<NJ>(key, kk);
  int gt = 0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) gt += __popcll(__ballot(key[j] > thr));
  const uint32_t need = (uint32_t)(kk - gt);
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint32_t base_gt = 0, base_eq = 0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const bool g = key[j] > thr, e = key[j] == thr && key[j] != 0u;
    const uint64_t bg = __ballot(g), be = __ballot(e);
    int slot = -1;
    if (g) slot = (int)(base_gt + __popcll(bg & below));
    else if (e) {
      const uint32_t q = base_eq + __popcll(be & below);
      if (q < need) slot = gt + (int)q;
    }
    if (slot >= 0) { bk[slot] = key[j]; br[slot] = row[j]; }
    base_gt += __popcll(bg);
    base_eq += __popcll(be);
  }
  return thr;
}
