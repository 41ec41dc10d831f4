// Logit processors and token log-probabilities of the decode step (the sampler's neighbours):
//   * logit_processors_kernel: logit_bias, then repeat / frequency / presence penalties over the
//     row's window of history, in llama.cpp's order, in place on the bf16 logits;
//   * token_logprobs_kernel: log_softmax of the raw logits at the chosen token and at the N most
//     probable ones, written to a per-row record.
// Both run one workgroup per row inside the captured step: no host sync, no allocation, and no
// state of their own -- the history is read where the engines already keep it (tokens[b, :count]
// with count from the static engine's step counter or the continuous engine's gen[b]), so the
// capture warm-up has nothing extra to save and restore.
#include "common.h"

namespace {

constexpr int PEN_WINDOW_CAP = 1024;   // history tokens a row's penalties can look back over
constexpr int BIAS_CAP = 512;          // logit_bias entries per row
constexpr int TOPLP_CAP = 20;          // top log-probabilities per record
constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_CAND = 1024;          // candidate list of the top-N ranking

// ---------------------------------------------------------------------------------------------
// Processors.  One 1024-thread workgroup per row: thread i owns window position i and bias entry
// i.  A token is written by exactly one thread -- a bias entry's thread (it also applies the
// token's penalty), or the thread of the token's first occurrence in the window when it has no
// bias -- and a thread reads only the logit it writes, so there is no ordering between writers.
// Only touched logits are read or written: the cost does not depend on V.
__global__ void __launch_bounds__(1024) logit_processors_kernel(
    uint16_t* __restrict__ logits, int V, const int32_t* __restrict__ tokens, int tok_stride,
    const int32_t* __restrict__ step_ptr, const int32_t* __restrict__ gen, const int32_t* __restrict__ done,
    const int32_t* __restrict__ prompt_tail, const int32_t* __restrict__ tail_len, int wmax,
    const int32_t* __restrict__ last_n, const float* __restrict__ repeat, const float* __restrict__ frequency,
    const float* __restrict__ presence, const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_vals,
    const int32_t* __restrict__ n_bias) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (done && done[b]) return;
  __shared__ __attribute__((aligned(16))) int32_t wtok[PEN_WINDOW_CAP];
  __shared__ int32_t bid[BIAS_CAP];
  const float rep = repeat[b], freq = frequency[b], pres = presence[b];
  const int nb = max(0, min(n_bias[b], BIAS_CAP));
  const bool pen = !(rep == 1.f && freq == 0.f && pres == 0.f);
  // window = the last w tokens of prompt_tail[:tl] ++ tokens[:count]
  int w = 0, tl = 0, hist_len = 0;
  if (pen) {
    int n = last_n[b];
    if (n < 0 || n > wmax) n = wmax;
    tl = max(0, min(tail_len[b], wmax));
    int count = gen ? gen[b] : (step_ptr ? *step_ptr : 0);
    count = tokens ? max(0, min(count, tok_stride)) : 0;
    hist_len = tl + count;
    w = min(n, hist_len);
  }
  if (w == 0 && nb == 0) return;       // neutral row: every bit stays
  uint16_t* lr = logits + (size_t)b * V;
  const int w4 = (w + 3) & ~3;
  if (tid < w4) {
    int t = -1;
    if (tid < w) {
      const int p = hist_len - w + tid;
      t = p < tl ? prompt_tail[(size_t)b * wmax + p] : tokens[(size_t)b * tok_stride + (p - tl)];
      if ((unsigned)t >= (unsigned)V) t = -1;      // never index outside the row
    }
    wtok[tid] = t;
  }
  if (tid < nb) {
    const int id = bias_ids[(size_t)b * BIAS_CAP + tid];
    bid[tid] = (unsigned)id < (unsigned)V ? id : -1;
  }
  __syncthreads();
  auto window_count = [&](int t, int before, bool& first) -> int {
    int c = 0;
    first = true;
    for (int j = 0; j < w4; j += 4) {
      const int4 q = *reinterpret_cast<const int4*>(&wtok[j]);
      const int e0 = q.x == t, e1 = q.y == t, e2 = q.z == t, e3 = q.w == t;
      c += e0 + e1 + e2 + e3;
      if ((e0 && j < before) || (e1 && j + 1 < before) || (e2 && j + 2 < before) || (e3 && j + 3 < before))
        first = false;
    }
    return c;
  };
  auto penalise = [&](float x, int c) -> float {
    x = x <= 0.f ? x * rep : x / rep;
    return x - ((float)c * freq + pres);
  };
  if (tid < nb && bid[tid] >= 0) {                 // bias, then the same token's penalty
    const int id = bid[tid];
    const float bv = bias_vals[(size_t)b * BIAS_CAP + tid];
    float x = bf2f(lr[id]);
    x = bv == -INFINITY ? -INFINITY : x + bv;
    bool first;
    const int c = w > 0 ? window_count(id, 0, first) : 0;
    if (c > 0) x = penalise(x, c);
    lr[id] = f2bf(x);
  }
  if (tid < w && wtok[tid] >= 0) {                 // penalty of a token without a bias entry
    const int t = wtok[tid];
    bool first;
    const int c = window_count(t, tid, first);
    if (first) {
      bool biased = false;
      for (int j = 0; j < nb; ++j) biased |= bid[j] == t;
      if (!biased) lr[t] = f2bf(penalise(bf2f(lr[t]), c));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Log-probabilities.

// NaN ranks as -inf, as in the samplers
__device__ __forceinline__ uint16_t lp_clean(uint16_t u) { return (u & 0x7fffu) > 0x7f80u ? (uint16_t)0xff80u : u; }

// order-preserving 16-bit image of a bf16 (larger value = larger key)
__device__ __forceinline__ uint32_t key16(uint16_t u) {
  return (u & 0x8000u) ? (~(uint32_t)u & 0xffffu) : ((uint32_t)u | 0x8000u);
}

// f(clean bf16 bits, index) over one row: a scalar head up to the first 16-byte boundary, 16-byte
// vectors (four independent loads in flight per thread, as sample_kernel), then a scalar tail --
// rows of a vocabulary that is no multiple of 8 start at any 2-byte offset.
template <typename F>
__device__ __forceinline__ void lp_for_row(const uint16_t* __restrict__ lr, int V, F&& f) {
  const int tid = threadIdx.x;
  const int head = min(V, (int)((16u - ((uintptr_t)lr & 15u)) & 15u) >> 1);
  const int nvec = (V - head) >> 3;
  if (tid < head) f(lp_clean(lr[tid]), tid);
  const uint4* vp = reinterpret_cast<const uint4*>(lr + head);
  for (int c0 = tid; c0 < nvec; c0 += 4 * LP_THREADS) {
    uint4 raw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * LP_THREADS;
      raw[u] = c < nvec ? vp[c] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * LP_THREADS;
      if (c >= nvec) break;
      const uint32_t wds[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(lp_clean((uint16_t)(wds[j] & 0xffffu)), head + c * 8 + 2 * j);
        f(lp_clean((uint16_t)(wds[j] >> 16)), head + c * 8 + 2 * j + 1);
      }
    }
  }
  for (int i = head + nvec * 8 + tid; i < V; i += LP_THREADS) f(lp_clean(lr[i]), i);
}

// Key of the K-th largest of a set of 16-bit keys: two passes of a 256-bin LDS histogram.
// ROW: the set is the whole row; otherwise every thread contributes `own`.
template <bool ROW>
__device__ uint32_t select16(const uint16_t* __restrict__ lr, int V, uint32_t own, int K, uint32_t* hist,
                             uint32_t* s_pair) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, mask = 0, remaining = (uint32_t)K;
  for (int shift = 8; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    if (ROW) {
      for (int i = tid; i < V; i += LP_THREADS) {
        const uint32_t k = key16(lp_clean(lr[i]));
        if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 0xFF], 1u);
      }
    } else if ((own & mask) == prefix) {
      atomicAdd(&hist[(own >> shift) & 0xFF], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (cum + hist[bin] >= remaining) break;
        cum += hist[bin];
      }
      s_pair[0] = prefix | ((uint32_t)bin << shift);
      s_pair[1] = remaining - cum;
    }
    __syncthreads();
    prefix = s_pair[0];
    remaining = s_pair[1];
    mask |= 0xFFu << shift;
    __syncthreads();
  }
  return prefix;
}

// (max, sum of exp(x - max)) pairs merge
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == -INFINITY) return;         // both empty
  s = s * __expf(m - nm) + os * __expf(om - nm);
  m = nm;
}

// One 1024-thread workgroup per row.
//   pass 1 (one memory round trip, as sample_kernel): running max and sum of exponentials per
//           thread, merged over the block -> log Z; every thread also keeps the key of its own
//           largest logit.
//   top-N:  the K-th largest of the 1024 thread maxima is a lower bound T of the row's K-th largest
//           (K distinct elements reach it), so the candidates are the elements >= T: pass 2 gathers
//           them into LDS and they are ranked by (value desc, index asc), the order of
//           sample_topk_kernel.  Rows where that list would overflow (long runs of ties at T, or
//           one thread holding many of the largest) take that kernel's scheme instead: radix
//           select of the exact K-th key over the row, gather of the keys above it, and the ties
//           at it by ascending index with per-wave ballots.
__global__ void __launch_bounds__(LP_THREADS) token_logprobs_kernel(
    const uint16_t* __restrict__ logits, const int32_t* __restrict__ chosen, int V, int N,
    const int32_t* __restrict__ step_ptr, const int32_t* __restrict__ gen, const int32_t* __restrict__ done, int cap,
    float* __restrict__ out_lp, int32_t* __restrict__ out_ids, float* __restrict__ out_top) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (done && done[row]) return;
  const int rec = gen ? gen[row] : (step_ptr ? *step_ptr : 0);
  if (rec < 0 || rec >= cap) return;
  const uint16_t* lr = logits + (size_t)row * V;
  __shared__ float red_m[LP_WAVES], red_s[LP_WAVES];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_pair[2];
  __shared__ int s_n, s_gt;
  __shared__ float cv[LP_CAND];
  __shared__ int ci[LP_CAND];
  __shared__ int tie_i[LP_WAVES][TOPLP_CAP];
  __shared__ int tie_n[LP_WAVES];
  __shared__ float sv[TOPLP_CAP];
  __shared__ int si[TOPLP_CAP];

  float m = -INFINITY, s = 0.f;
  uint32_t tkey = 0;                   // below every real key: a thread that saw no element
  lp_for_row(lr, V, [&](uint16_t u, int) {
    const float x = bf2f(u);
    tkey = max(tkey, key16(u));
    if (x != -INFINITY) {
      const float d = x - m, e = __expf(-fabsf(d));
      s = d > 0.f ? s * e + 1.f : s + e;
      m = fmaxf(m, x);
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane == 0) { red_m[wid] = m; red_s[wid] = s; }
  if (tid == 0) { s_n = 0; s_gt = 0; }
  __syncthreads();
  m = red_m[0]; s = red_s[0];
  for (int i = 1; i < LP_WAVES; ++i) lse_merge(m, s, red_m[i], red_s[i]);
  const float logz = m + logf(s);      // the same value in every thread

  const size_t r = (size_t)row * cap + rec;
  if (tid == 0) {
    const int c = chosen[row];
    out_lp[r] = (unsigned)c < (unsigned)V ? bf2f(lp_clean(lr[c])) - logz : -INFINITY;
  }
  if (N <= 0) return;
  const int K = min(N, V);
  int32_t* oi = out_ids + r * N;
  float* ot = out_top + r * N;
  if (tid >= K && tid < N) { oi[tid] = -1; ot[tid] = -INFINITY; }   // V < N: the rest stays empty

  uint32_t T = select16<false>(nullptr, 0, tkey, K, hist, s_pair);
  int gt = 0;
  lp_for_row(lr, V, [&](uint16_t u, int idx) {
    const uint32_t k = key16(u);
    if (k >= T) {
      gt += k > T;
      const int slot = atomicAdd(&s_n, 1);
      if (slot < LP_CAND) { cv[slot] = bf2f(u); ci[slot] = idx; }
    }
  });
  if (gt) atomicAdd(&s_gt, gt);
  __syncthreads();
  int n = s_n;
  if (n > LP_CAND) {                   // block-uniform
    if (s_gt > LP_CAND - K) T = select16<true>(lr, V, 0, K, hist, s_pair);   // now fewer than K lie above T
    __syncthreads();
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < V; i += LP_THREADS) {
      const uint16_t u = lp_clean(lr[i]);
      if (key16(u) > T) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < LP_CAND) { cv[slot] = bf2f(u); ci[slot] = i; }
      }
    }
    {  // the K lowest-index ties at T: each wave scans its 1/16 of the row in index order
      const int lo = (int)(((int64_t)V * wid) / LP_WAVES), hi = (int)(((int64_t)V * (wid + 1)) / LP_WAVES);
      int found = 0;
      for (int base = lo; base < hi && found < K; base += 64) {
        const int i = base + lane;
        const bool tie = i < hi && key16(lp_clean(lr[i])) == T;
        const unsigned long long bm = __ballot(tie);
        if (tie) {
          const int pos = found + __popcll(bm & ((1ull << lane) - 1ull));
          if (pos < K) tie_i[wid][pos] = i;
        }
        found += __popcll(bm);
      }
      if (lane == 0) tie_n[wid] = min(found, K);
    }
    __syncthreads();
    if (tid == 0) {
      int n0 = min(s_n, LP_CAND - K), added = 0;
      for (int w = 0; w < LP_WAVES && added < K; ++w)
        for (int j = 0; j < tie_n[w] && added < K; ++j, ++added) {
          ci[n0] = tie_i[w][j];
          cv[n0] = bf2f(lp_clean(lr[tie_i[w][j]]));
          ++n0;
        }
      s_n = n0;
    }
    __syncthreads();
    n = s_n;
  }
  // rank = position in (value desc, index asc)
  if (tid < n) {
    const float v = cv[tid];
    const int id = ci[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (cv[j] > v) || (cv[j] == v && ci[j] < id);
    if (rank < K) { sv[rank] = v; si[rank] = id; }
  }
  __syncthreads();
  if (tid < K) { oi[tid] = si[tid]; ot[tid] = sv[tid] - logz; }
}

}  // namespace

CFC_API int cfc_logit_window_cap() { return PEN_WINDOW_CAP; }
CFC_API int cfc_logit_bias_cap() { return BIAS_CAP; }
CFC_API int cfc_top_logprobs_cap() { return TOPLP_CAP; }

// logits [B, V] bf16, rewritten in place.  History of row b = prompt_tail[b, :tail_len[b]] ++
// tokens[b, :count], count = gen[b] (continuous engine) or *step_ptr (static engine); both null (or
// tokens null): nothing generated yet -- the prefill's first token.  prompt_tail is [B, wmax],
// bias_ids / bias_vals are [B, 512].
CFC_API int cfc_logit_processors(void* logits, int B, int V, const int32_t* tokens, int tok_stride,
                                 const int32_t* step_ptr, const int32_t* gen, const int32_t* done,
                                 const int32_t* prompt_tail, const int32_t* tail_len, int wmax, const int32_t* last_n,
                                 const float* repeat, const float* frequency, const float* presence,
                                 const int32_t* bias_ids, const float* bias_vals, const int32_t* n_bias,
                                 hipStream_t stream) {
  if (B == 0) return 0;
  if (B < 0 || V <= 0 || wmax < 1 || wmax > PEN_WINDOW_CAP || tok_stride < 0 || (step_ptr && gen)) return -1;
  if (!logits || !prompt_tail || !tail_len || !last_n || !repeat || !frequency || !presence || !bias_ids ||
      !bias_vals || !n_bias)
    return -1;
  logit_processors_kernel<<<B, 1024, 0, stream>>>((uint16_t*)logits, V, tokens, tok_stride, step_ptr, gen, done,
                                                  prompt_tail, tail_len, wmax, last_n, repeat, frequency, presence,
                                                  bias_ids, bias_vals, n_bias);
  return CFC_CHECK_LAUNCH();
}

// Record of row b goes to index gen[b] / *step_ptr (both null: 0) of out_lp [B, cap], out_ids and
// out_top [B, cap, N]; rows with done[b] != 0 or an index outside [0, cap) write nothing.
CFC_API int cfc_token_logprobs(const void* logits, const int32_t* chosen, int B, int V, int N,
                               const int32_t* step_ptr, const int32_t* gen, const int32_t* done, int cap,
                               float* out_lp, int32_t* out_ids, float* out_top, hipStream_t stream) {
  if (B == 0) return 0;
  if (B < 0 || V <= 0 || N < 0 || N > TOPLP_CAP || cap < 1 || (step_ptr && gen)) return -1;
  if (!logits || !chosen || !out_lp || (N > 0 && (!out_ids || !out_top))) return -1;
  token_logprobs_kernel<<<B, LP_THREADS, 0, stream>>>((const uint16_t*)logits, chosen, V, N, step_ptr, gen, done,
                                                      cap, out_lp, out_ids, out_top);
  return CFC_CHECK_LAUNCH();
}
