// W8A8 FP8 prefill GEMM for gfx950 at any M >= 1 (built for M in the hundreds to tens of thousands):
//   Y[M, N] (bf16) = diag(sx) . (X8[M, K] . W8[N, K]^T) . diag(sw)
// X8 row-major OCP e4m3fn with sx fp32 per row (what rmsnorm_fp8 / silu_mul_fp8 / quant_fp8_rows
// emit); W8 in the FP8 decode GEMM's fragment-packed layout (cfc_f8dgemm_pack, any of its bn) with
// sw fp32 per W row.  It reads the weight copy f8dgemm.hip reads, so W8A8 prefill and decode share
// one FP8 copy of the projections and no library GEMM is left on the FP8 decoder's path.
//
// This is pgemm.hip's ping-pong kernel ("pp", pgemm_pp_kernel, packed W) with one-byte elements:
// at BK = 128 k the byte geometry of that kernel carries over unchanged, and so does its schedule.
//
// Work split.  256 x 256 output tile per workgroup of 8 waves (launch bound 1: one workgroup per
// CU); wave (grp, wc) owns output rows 128 grp .. + 128, columns 64 wc .. + 64: acc[8][4] of f32x4,
// 128 accumulator VGPRs.  blockIdx -> tile as in pgemm: bijective XCD remap, then groups of 8
// M-tiles sweep the N-tiles, so the workgroups resident on one XCD share X rows and W rows in its
// L2.  The waves are two groups of four (0-3, 4-7: one of each on every SIMD) running one barrier
// apart, so on each SIMD one wave's MFMA segment covers its partner's load segment.
//
// K-tile = 128 k = 4 half-tiles of 128 rows x 128 B = 16 KB: X0 = tile rows {0-63, 128-191},
// X1 = {64-127, 192-255}, W0 = W rows 0-127, W1 = 128-255; two K-tile buffers = 128 KB of LDS.  Every
// wave issues two 1-KB LDS-DMA pieces per half.  K-tile kt runs as segment A (X0 and both W halves:
// the wave's first 64 rows) and segment B (X1: its last 64 rows, the W fragments kept in
// registers), 16 MFMAs each; segment A issues tile kt+1's X1, segment B tile kt+2's {X0, W0, W1},
// each into a half whose last reader retired its ds_reads before the barrier in front of the issue;
// the counted vmcnt(8) of both segments leaves 4 half-tiles of DMA in flight per wave and retires
// exactly what the next segment reads.  K / 128 of 1 or 2 is shorter than the prologue: the
// prologue issues only the tiles that exist and its wait and the tail waits count what was issued.
//
// Instruction: v_mfma_f32_16x16x128_f8f6f4 (f8_mfma, common.h), W fragment as A, X fragment as B,
// so a lane's accumulator holds 4 CONSECUTIVE output columns of one row.  Per K-tile a wave issues
// 32 of them where "pp" issues 64 of 16x16x32 bf16, over the same staged bytes and the same 16
// ds_read_b128 per segment A (8 per segment B).  IF the FP8 instruction has twice the bf16
// instruction's flop rate, MFMA time per K-tile equals "pp"'s and the balance of DMA, LDS reads and
// matrix pipe is "pp"'s at twice the flops: reasoned, not measured -- what the probe measured is in
// profiles/ROOFLINE.md, "FP8 prefill GEMM".
//
// X image: 128-B rows, chunk c (16 B) of image row r at r * 128 + ((c ^ (r & 7)) << 4), the swizzle
// applied through the DMA's source address; image row r of half h is tile row (r >> 6) * 128 +
// 64 h + (r & 63).  A fragment is two ds_read_b128: lane (row l & 15, group g = l >> 4) reads chunk
// g, then chunk 4 + g.  Bank argument: f8dgemm.hip's header (the same image, the same read) --
// every one of the 16 chunk slots of a 256-B bank row is read by exactly 4 of the 64 lanes, the four
// passes a 1-KB read needs anyway; reasoned, not measured.  Rows past M read row M - 1.
//
// W: the 16-row x 128-k fragment of row group G = n / 16 and k block kb is 2 KB contiguous at
// (((G / nw) * (K / 128) + kb) * nw + G % nw) * 2048 with nw = bn / 16: two 1-KB pieces, lane l of
// piece h holding W[16 G + (l & 15)][128 kb + 64 h + 16 (l >> 4) .. + 15].  A W half is 8 fragments =
// 16 pieces, two per wave (pieces w and w + 8: fragment piece >> 1, half piece & 1); G / nw and
// G % nw are taken per piece, so a 256-row tile may straddle the bn-row groups of the packed layout
// (bn = 96, 112) and any bn the decode kernel chose serves.  Piece p lands at p * 1024 of the half,
// i.e. fragment f's piece h at f * 2048 + h * 1024, and its ds_read_b128 at + 16 l is conflict
// free.  Row groups past N read group N / 16 - 1; nothing past M or N is stored.
//
// Which k sits where: lane group g, byte i of a lane's 32 bytes carries k = 64 (i / 16) + 16 g +
// i % 16 of the block in the W fragment (the pack kernel) and in the X fragment (chunk 4 h + g of
// the row is bytes 64 h + 16 g .. + 15); the reduction over k is order-free (f8dgemm.hip).
//
// Epilogue: acc * (sx[m] * sw[n]) in f8dgemm.hip's expression order, rounded to bf16, one 8-byte
// store per lane and accumulator; sx and sw are loaded after the K loop, not held across it.  No
// SwiGLU epilogue: the down projection's input needs a per-row amax over the whole FFN width, so
// silu_mul_fp8 follows the bf16 output.  No LDS-staged 16-byte stores ("pps"): not measured here.
//
// Bounds: M >= 1, N % 64 == 0, K % 128 == 0, ldo % 4 == 0, X and padded-W byte spans < 4 GiB
// (32-bit DMA offsets).  Not built (follow-ups): a persistent variant like "ppp", fp32 partials for
// tensor parallel, a second tile shape for short M.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void f8p_lds_t;

constexpr int F8P_BM = 256, F8P_BN = 256, F8P_BK = 128;
constexpr int F8P_GROUP_M = 8;
constexpr int F8P_HALF = 128 * 128;        // bytes of one half-tile (128 rows x 128 k)
constexpr int F8P_BUF = 4 * F8P_HALF;      // X0 X1 W0 W1

// One 1-KB LDS-DMA piece from sbase + voff (per lane): lane l's 16 bytes land at lds_addr + 16 l
// (pgemm.hip's pg_glds16: inline asm so that the compiler orders nothing behind it; M0 saved and
// restored in the statement)
__device__ __forceinline__ void f8p_glds16(uint32_t voff, const void* sbase, uint32_t lds_addr) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory");
}

__device__ __forceinline__ void f8p_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <int N>
__device__ __forceinline__ void f8p_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}

__global__ void __launch_bounds__(512, 1)
    f8pgemm_kernel(const uint8_t* __restrict__ X, const float* __restrict__ sx, const uint8_t* __restrict__ W,
                   const float* __restrict__ sw, uint16_t* __restrict__ out, int M, int N, int K, int ldo, int tiles_m,
                   int tiles_n, int wnw) {
  __shared__ __attribute__((aligned(16))) char smem[2 * F8P_BUF];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = w >> 2, wc = w & 3;

  // ---- tile of this workgroup: XCD-local id, then GROUP_M-row groups sweeping the N tiles
  const int nwg = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int per_group = F8P_GROUP_M * tiles_n;
  const int first_m = (id / per_group) * F8P_GROUP_M;
  const int gsz = min(tiles_m - first_m, F8P_GROUP_M);
  const int in_group = id % per_group;
  const int m0 = (first_m + in_group % gsz) * F8P_BM;
  const int n0 = (in_group / gsz) * F8P_BN;
  const int nk = K / F8P_BK;

  // ---- DMA sources (byte offsets).  X: pieces w and w + 8 of half h = image rows 8 p .. 8 p + 7
  // (lane: row lane >> 3, chunk lane & 7 through the swizzle).  W half h, pieces w and w + 8: piece p
  // is half p & 1 of the fragment of row group n0 / 16 + 8 h + (p >> 1), k block 0
  uint32_t vx[2][2], vw[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = w + 8 * i;
      const int r = 8 * p + (lane >> 3);
      const int trow = (r >> 6) * 128 + 64 * h + (r & 63);
      const int c = (lane & 7) ^ (r & 7);
      vx[h][i] = (uint32_t)min(m0 + trow, M - 1) * (uint32_t)K + 16u * c;
      const int G = min(n0 / 16 + 8 * h + (p >> 1), N / 16 - 1);
      vw[h][i] = (uint32_t)((G / wnw) * nk * wnw + G % wnw) * 2048u + (p & 1) * 1024u + 16u * lane;
    }
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(f8p_lds_t*)smem + w * 1024);
  const size_t wstep = (size_t)wnw * 2048;   // one k block of every row group of a bn-row group
  auto issue_x = [&](int kt, int h) {
    const uint8_t* src = X + (size_t)kt * F8P_BK;
    const uint32_t la = lds0 + (kt & 1) * F8P_BUF + h * F8P_HALF;
    f8p_glds16(vx[h][0], src, la);
    f8p_glds16(vx[h][1], src, la + 8192);
  };
  auto issue_w = [&](int kt, int h) {
    const uint8_t* src = W + (size_t)kt * wstep;
    const uint32_t la = lds0 + (kt & 1) * F8P_BUF + (2 + h) * F8P_HALF;
    f8p_glds16(vw[h][0], src, la);
    f8p_glds16(vw[h][1], src, la + 8192);
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // fragment reads.  X: image row 64 grp + 16 i + (lane & 15) of the half, chunk 4 hh + (lane >> 4)
  // through the swizzle (row & 7 == lane & 7).  W n-tile T = 4 wc + j lies in half T >> 3.
  const int xrd = (64 * grp + (lane & 15)) * 128;
  const int swz = lane & 7;
  auto rd_x = [&](int buf, int h, int i, int hh) {
    return *reinterpret_cast<const uint4*>(smem + buf + h * F8P_HALF + xrd + i * 16 * 128 +
                                           (((4 * hh + (lane >> 4)) ^ swz) << 4));
  };
  auto rd_w = [&](int buf, int j, int hh) {
    const int T = 4 * wc + j;
    return *reinterpret_cast<const uint4*>(smem + buf + (2 + (T >> 3)) * F8P_HALF + (T & 7) * 2048 + hh * 1024 +
                                           16 * lane);
  };

  // ---- prologue: tile 0 whole, tile 1's {X0, W0, W1}; tile 0's X0 / W0 / W1 landed in every wave
  issue_x(0, 0);
  issue_w(0, 0);
  issue_w(0, 1);
  issue_x(0, 1);
  if (nk > 1) {
    issue_x(1, 0);
    issue_w(1, 0);
    issue_w(1, 1);
    f8p_wait_barrier<8>();
  } else {
    f8p_wait_barrier<2>();
  }
  if (grp == 1) f8p_barrier();   // the stagger: group 1 runs one barrier behind group 0

  uint4 wf[4][2], xf[4][2];
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = (kt & 1) * F8P_BUF;
    // ======== segment A: load part (tile kt+1's X1 into the other buffer; fragments)
    if (kt + 1 < nk) issue_x(kt + 1, 1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) wf[j][hh] = rd_w(buf, j, hh);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) xf[i][hh] = rd_x(buf, 0, i, hh);
    // retire tile kt's X1 (segment B reads it) and this wave's ds_reads
    if (kt + 1 < nk) f8p_wait_barrier<8>();
    else f8p_wait_barrier<0>();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f8_mfma(wf[j][0], wf[j][1], xf[i][0], xf[i][1], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    f8p_barrier();
    // ======== segment B: load part (tile kt+2's X0 / W0 / W1 into this buffer's free halves)
    if (kt + 2 < nk) {
      issue_x(kt + 2, 0);
      issue_w(kt + 2, 0);
      issue_w(kt + 2, 1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) xf[i][hh] = rd_x(buf, 1, i, hh);
    // retire tile kt+1's X0 / W0 / W1 (next segment A reads them)
    if (kt + 2 < nk) f8p_wait_barrier<8>();
    else if (kt + 1 < nk) f8p_wait_barrier<2>();
    else f8p_wait_barrier<0>();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[4 + i][j] = f8_mfma(wf[j][0], wf[j][1], xf[i][0], xf[i][1], acc[4 + i][j]);
    __builtin_amdgcn_sched_barrier(0);
    f8p_barrier();
  }

  // ---- epilogue: lane holds rows m = mw + 16 i + (lane & 15) (segment A's m-tiles i < 4 = tile rows
  // 128 grp + 16 i, segment B's = 128 grp + 64 + 16 (i - 4)), columns nq + 16 j .. + 3
  const int mw = m0 + grp * 128 + (lane & 15);
  const int nq = n0 + wc * 64 + 4 * (lane >> 4);
  float4 swv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    swv[j] = nq + 16 * j < N ? *reinterpret_cast<const float4*>(sw + nq + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
  float sxv[8];   // all eight in flight at once (rows past M: row M - 1's, unused)
#pragma unroll
  for (int i = 0; i < 8; ++i) sxv[i] = sx[min(mw + 16 * i, M - 1)];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = mw + 16 * i;
    if (m < M) {
      const float s = sxv[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = nq + 16 * j;
        if (n < N)
          *reinterpret_cast<uint2*>(out + (size_t)m * ldo + n) =
              make_uint2(pack2bf(acc[i][j][0] * (s * swv[j].x), acc[i][j][1] * (s * swv[j].y)),
                         pack2bf(acc[i][j][2] * (s * swv[j].z), acc[i][j][3] * (s * swv[j].w)));
      }
    }
  }
  if (grp == 0) f8p_barrier();   // matches group 1's stagger barrier
}

}  // namespace

// Y = diag(sx) (X8 . W8^T) diag(sw), bf16: x [M, K] e4m3fn row-major, sx [M] fp32, w in the packed
// layout cfc_f8dgemm_pack wrote for this same bn, sw [N] fp32; bf16 rows at out + m * ldo (out points
// at the first column of the written range [0, N), 8-byte aligned).  M >= 1, N % 64 == 0,
// K % 128 == 0, bn in {64, 96, 112, 128}, ldo % 4 == 0, ldo >= N, X and the padded W under 4 GiB.
// Returns a negative code (nothing launched) for anything else.
CFC_API int cfc_f8pgemm(const void* x, const float* sx, const void* w, const float* sw, int M, int N, int K, int bn,
                        void* out, int ldo, hipStream_t stream) {
  if (M < 1 || N <= 0 || N % 64 || K <= 0 || K % 128 || !x || !sx || !w || !sw || !out) return -1;
  if (bn != 64 && bn != 96 && bn != 112 && bn != 128) return -5;
  if (ldo < N || ldo % 4 || ((uintptr_t)out & 7) || ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)sw & 15))
    return -6;
  if ((uint64_t)M * K >= (1ull << 32) || (uint64_t)((N + bn - 1) / bn) * bn * K >= (1ull << 32)) return -6;
  const int tm = (M + F8P_BM - 1) / F8P_BM, tn = (N + F8P_BN - 1) / F8P_BN;
  if ((long long)tm * tn >= (1ll << 31)) return -6;
  f8pgemm_kernel<<<tm * tn, 512, 0, stream>>>((const uint8_t*)x, sx, (const uint8_t*)w, sw, (uint16_t*)out, M, N, K,
                                              ldo, tm, tn, bn / 16);
  return CFC_CHECK_LAUNCH();
}
