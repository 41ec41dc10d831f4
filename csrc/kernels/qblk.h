// One lane's view of a 256-weight block of a ggml-quantized row in the planar GPU layouts of
// quant.hip (ops/kernels.py:_planar), shared by the quantized decode GEMM (qdgemm.hip) and the
// unpack into the decode GEMM's packed bf16 layout (qunpack.hip).  Every weight becomes the bf16
// value dequant_bf16 produces: fp32 d.sc.q - dmin.m (one fmaf; the products are exact), one RNE
// rounding to bf16.
#pragma once
#include "common.h"

namespace {

enum { QT_Q4K = 12, QT_Q6K = 14, QT_Q8_0 = 8 };

typedef unsigned int qd_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 qd_stream(const void* p) {   // once-read weights: nontemporal
  const qd_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const qd_u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float qd_h2f(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
__device__ __forceinline__ uint32_t qd_byte(uint32_t v, int k) { return (v >> (8 * k)) & 0xffu; }

// get_scale_min_k4 on the 12 scale bytes held in three dwords (quant.hip: scale_min_k4r)
__device__ __forceinline__ void qd_scale_min(int j, uint32_t s0, uint32_t s1, uint32_t s2, int& d, int& m) {
  if (j < 4) {
    d = qd_byte(s0, j) & 63;
    m = qd_byte(s1, j) & 63;
  } else {
    const int k = j - 4;
    d = (qd_byte(s2, k) & 0xF) | ((qd_byte(s0, k) >> 6) << 4);
    m = (qd_byte(s2, k) >> 4) | ((qd_byte(s1, k) >> 6) << 4);
  }
}

// the 8 byte values of dwords a, b (weights 0-3, 4-7) -> 8 bf16 of s * byte + c (fp32 fma, RNE)
__device__ __forceinline__ uint4 qd_deq8(uint32_t a, uint32_t b, float s, float c) {
  uint4 r;
  r.x = cvt_pk_bf16_f32(fmaf(s, (float)(a & 0xffu), c), fmaf(s, (float)((a >> 8) & 0xffu), c));
  r.y = cvt_pk_bf16_f32(fmaf(s, (float)((a >> 16) & 0xffu), c), fmaf(s, (float)(a >> 24), c));
  r.z = cvt_pk_bf16_f32(fmaf(s, (float)(b & 0xffu), c), fmaf(s, (float)((b >> 8) & 0xffu), c));
  r.w = cvt_pk_bf16_f32(fmaf(s, (float)((b >> 16) & 0xffu), c), fmaf(s, (float)(b >> 24), c));
  return r;
}

// One lane's share of one 256-weight block of its row: chunks 2g and 2g + 1.  load() issues the
// global loads, prep() turns the header into per-chunk fp32 scale / offset, frag<S, J>() builds the
// 8 bf16 of weights 32 (2g + S) + 8 J .. + 7.
template <int T>
struct QBlk;

template <>
struct QBlk<QT_Q4K> {
  uint4 nib[2], hdr;
  float sc[2], of[2];
  __device__ __forceinline__ void load(const uint8_t* base, const size_t* off, int row, int b, int g, int K) {
    const uint8_t* p = base + (size_t)row * (K / 2) + 128 * b + 32 * g;
    nib[0] = qd_stream(p);
    nib[1] = qd_stream(p + 16);
    hdr = *reinterpret_cast<const uint4*>(base + off[0] + (size_t)row * (K / 16) + 16 * b);
  }
  __device__ __forceinline__ void prep(int g) {
    const float d = qd_h2f(hdr.x & 0xffffu), dm = qd_h2f(hdr.x >> 16);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int q, m;
      qd_scale_min(2 * g + s, hdr.y, hdr.z, hdr.w, q, m);
      sc[s] = d * (float)q;
      of[s] = -(dm * (float)m);
    }
  }
  template <int S, int J>
  __device__ __forceinline__ uint4 frag() const {
    uint32_t a = (J & 1) ? nib[S].z : nib[S].x, b = (J & 1) ? nib[S].w : nib[S].y;
    if (J >= 2) { a >>= 4; b >>= 4; }
    return qd_deq8(a & 0x0F0F0F0Fu, b & 0x0F0F0F0Fu, sc[S], of[S]);
  }
};

template <>
struct QBlk<QT_Q6K> {
  uint4 nib[2], hi;
  uint32_t sc4, dd;
  float sc[4];
  __device__ __forceinline__ void load(const uint8_t* base, const size_t* off, int row, int b, int g, int K) {
    const uint8_t* p = base + (size_t)row * (K / 2) + 128 * b + 32 * g;
    nib[0] = qd_stream(p);
    nib[1] = qd_stream(p + 16);
    hi = qd_stream(base + off[0] + (size_t)row * (K / 4) + 64 * b + 16 * g);
    sc4 = *reinterpret_cast<const uint32_t*>(base + off[1] + (size_t)row * (K / 16) + 16 * b + 4 * g);
    dd = *reinterpret_cast<const uint16_t*>(base + off[2] + (size_t)row * (K / 128) + 2 * b);
  }
  __device__ __forceinline__ void prep(int) {
    const float d = qd_h2f(dd);
#pragma unroll
    for (int k = 0; k < 4; ++k) sc[k] = d * (float)(int8_t)qd_byte(sc4, k);
  }
  template <int S, int J>
  __device__ __forceinline__ uint4 frag() const {
    // weights 8 J .. 8 J + 7 of chunk S: nibble dwords f = 2 (J & 1), + 1 (low nibbles for J < 2),
    // top bits from HI dword J >> 1 of the chunk at bit 2 f
    constexpr int F = 2 * (J & 1);
    uint32_t a = F ? nib[S].z : nib[S].x, b = F ? nib[S].w : nib[S].y;
    if (J >= 2) { a >>= 4; b >>= 4; }
    const uint32_t h = S ? (J >= 2 ? hi.w : hi.z) : (J >= 2 ? hi.y : hi.x);
    a = (a & 0x0F0F0F0Fu) | (((h >> (2 * F)) & 0x03030303u) << 4);
    b = (b & 0x0F0F0F0Fu) | (((h >> (2 * F + 2)) & 0x03030303u) << 4);
    const float s = sc[2 * S + (J >> 1)];
    return qd_deq8(a, b, s, -32.f * s);   // d sc (q - 32), one rounding
  }
};

template <>
struct QBlk<QT_Q8_0> {
  uint4 q[4];
  uint32_t d2;
  float sc[2];
  __device__ __forceinline__ void load(const uint8_t* base, const size_t* off, int row, int b, int g, int K) {
    const uint8_t* p = base + (size_t)row * K + 256 * b + 64 * g;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qd_stream(p + 16 * k);
    d2 = *reinterpret_cast<const uint32_t*>(base + off[0] + (size_t)row * (K / 16) + 16 * b + 4 * g);
  }
  __device__ __forceinline__ void prep(int) {
    sc[0] = qd_h2f(d2 & 0xffffu);
    sc[1] = qd_h2f(d2 >> 16);
  }
  template <int S, int J>
  __device__ __forceinline__ uint4 frag() const {
    const uint4 v = q[2 * S + (J >> 1)];
    const uint32_t a = ((J & 1) ? v.z : v.x) ^ 0x80808080u, b = ((J & 1) ? v.w : v.y) ^ 0x80808080u;
    return qd_deq8(a, b, sc[S], -128.f * sc[S]);   // int8 q = u - 128: d (u - 128), one rounding
  }
};

}  // namespace
