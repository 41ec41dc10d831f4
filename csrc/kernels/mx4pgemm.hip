// W4A8 MXFP4 prefill GEMM for gfx950 at any M >= 1 (built for M in the hundreds to tens of thousands):
//   Y[M, N] (bf16) = diag(sx) . (X8[M, K] . dequant(W4)[N, K]^T)
// X8 row-major OCP e4m3fn with sx fp32 per row (rmsnorm_fp8 / silu_mul_fp8 / quant_fp8_rows); W4 the
// PackedWeightMX4 the MXFP4 decode GEMM reads (cfc_mx4dgemm_pack's quad layout, any of its bn): one
// 4.25-bit copy of the projections serves prefill and decode, nothing is repacked or dequantised,
// and the e8m0 block scales go into the matrix unit through mx4_mfma<b> (common.h).
//
// Design built: W straight to registers, not staged in LDS.  It fits the 256 registers two waves per
// SIMD leave (see "Compiled" below), so the LDS fallback for the code fragments was not needed.
//
// Work split (f8pgemm.hip's geometry).  256 x 256 output tile per workgroup of 8 waves, launch bound
// 1; wave (grp, wc) owns rows 128 grp .. + 128, columns 64 wc .. + 64: acc[8][4] of f32x4.  blockIdx
// -> tile by the bijective XCD remap, then groups of 8 M-tiles sweeping the N-tiles.  The two 4-wave
// groups run one barrier apart, so on each SIMD one wave's MFMA part covers its partner's load part.
//
// What differs from f8pgemm.hip: LDS holds X only, W never touches it.
//   X: K-tile = one 128-k block = 2 halves of 128 rows x 128 B (X0 = tile rows {0-63, 128-191}, X1 =
//      {64-127, 192-255}), a ring of FOUR K-tiles = 128 KB, filled by LDS-DMA three K-tiles ahead;
//      every wave issues two 1-KB pieces per half.  The image is f8pgemm.hip's: chunk c (16 B) of
//      image row r at r * 128 + ((c ^ (r & 7)) << 4), the swizzle applied through the DMA's source
//      address.  A fragment is two ds_read_b128, lane (row l & 15, group g = l >> 4) reading chunk
//      g, then chunk 4 + g -- UNPERMUTED: with a 4-bit A against an 8-bit B the B lane group g must
//      hold k = 16 g .. + 15 and 64 + 16 g .. + 15 (measured, mx4dgemm.hip header point 2), which is
//      exactly this pair.  Bank argument: mx4dgemm.hip's, the same image and read; reasoned only.
//   W: each wave loads its four n-tiles' 1-KB code fragments (16 B per lane) with buffer loads
//      straight into a register ring, two K-tiles ahead: ring slot = block in quad, three of the
//      four slots live at any point = 48 VGPRs.  Each lane also loads one scale dword per n-tile
//      and quad (byte b = its own 32 codes' e8m0 scale in block b; op_sel picks it), for quad q + 1
//      during block 2 of quad q into a second set that block 0 of quad q + 1 takes over.  The K loop
//      is unrolled by one quad so that the op_sel byte and the ring slots (W's and X's) are
//      compile-time; its tail runs the K / 128 % 4 remaining blocks.  Record of 16-row group G and quad q:
//      (((G / nw) * ceil(K / 512) + q) * nw + G % nw) * 4352, nw = bn / 16, G / nw and G % nw taken
//      per n-tile, so a 256-column tile may straddle the packed bn-row groups (bn 96, 112).  Each
//      fragment is fetched by the two waves (grp 0 and 1) that use it: L2 traffic per K-tile and
//      workgroup is 32 KB of W + 32 KB of X, f8pgemm.hip's 64 KB.
//
// Schedule of K-tile kt (block b of its quad), per wave:
//   segment A  load part: DMA X0 of kt + 3; buffer loads W of kt + 2 (+ 4 scale dwords if b == 2);
//                         8 ds_read_b128 of X0 of kt;  counted wait + barrier
//              MFMA part: 16 mx4_mfma<b> (m-tiles 0-3 x 4 n-tiles);  barrier
//   segment B  load part: DMA X1 of kt + 3; 8 ds_read_b128 of X1 of kt;  lgkmcnt(0) + barrier
//              MFMA part: 16 mx4_mfma<b> (m-tiles 4-7), the W registers reused;  barrier
//   A DMA target (the ring slot of K-tile kt - 1) was last read one segment pair earlier, and those
//   ds_reads retired before a barrier in front of the issue in either group's order.
//
// Wait counts.  LDS-DMA and register loads share vmcnt and retire in issue order.  Every step
// issues the same loads, so the counts are constants and the K loop holds no branch (a run of steps
// is one basic block; with branches between them the compiler sank each MFMA part towards the
// accumulators' next use and spilled).  Per wave the order is
//   .. W(kt) | X1(kt+1) X0(kt+2) W(kt+1) X1(kt+2) X0(kt+3) W(kt+2) | segment A's wait,
// 2 pieces per X half and 4 loads per W, + 4 scale dwords in the W of blocks b == 2: the wait
// allows 16 (20 for b in {2, 3}) outstanding, which retires W(kt) and everything before it: X1(kt)
// and X0(kt+1), the halves read after this barrier.  Segment B needs no vmcnt wait.  The prologue
// issues X of tiles 0-2, the scale dwords of quad 0, W(0), W(1) and waits for X(0): 20 left.
// Past the end of K the loads stay unconditional and touch real data only: W re-reads the last
// quad (its blocks past K / 128 are the packer's zero codes), X re-stages K-tile K / 128 - 1 into
// the ring slot nobody reads any more (at most three K-tiles of extra L2 reads per workgroup); a
// block at or past K / 128 is never staged and never multiplied, and vmcnt(0) after the loop keeps
// the last pieces from landing in another workgroup's LDS.
// The W loads are compiler builtins and the compiler adds its own vmcnt waits before their first
// use.  It does not count the DMA pieces (inline asm), so its counts (11 .. 8 where 16 would do) are
// stricter than the order needs: they hold W(kt + 1) and X0(kt + 2) to about one K-tile of latency
// rather than two and three.  Correctness never depends on them: every X half is covered by the
// explicit counts above.
//
// Clamping: rows past M read row M - 1, row groups past N read group N / 16 - 1, nothing past M or
// N is stored; W goes through a buffer descriptor of the padded weight's size.
//
// Epilogue: acc * sx[m] rounded to bf16, one 8-byte store per lane and accumulator (lane = X row
// 16 i + (l & 15) at the 4 consecutive columns 16 j + 4 (l >> 4) ..); sx loaded after the K loop.
//
// Bounds: M >= 1, N % 64 == 0, K % 128 == 0, ldo % 4 == 0, X and padded-W byte spans < 4 GiB.
// Not built (follow-ups, as in f8pgemm.hip): SwiGLU epilogue, LDS-staged stores, a persistent
// variant, fp32 partials for tensor parallel, a second tile shape or split-K for short M.
//
// Compiled for gfx950: 256 VGPRs (0 AGPRs), 62 SGPRs, 128 KB LDS, no scratch, no spill.
// Measured on one MI355X: profiles/ROOFLINE.md, "MXFP4 prefill GEMM" (scripts/probes/
// mx4pgemm_probe.py): 0.86-0.97 of f8pgemm.hip's time at M = 16384 .. 256 on Mistral-7B's four
// projections.  Reasoned, NOT measured: that dropping W from LDS (16 KB instead of 24 KB of
// ds_read per wave and K-tile) relieves an LDS-bandwidth limit; the MFMA rate with an FP4 operand;
// the bank behaviour of the X read.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void mxp_lds_t;
typedef unsigned int mxp_u32x4 __attribute__((ext_vector_type(4)));

constexpr int MXP_BM = 256, MXP_BN = 256, MXP_BK = 128;
constexpr int MXP_GROUP_M = 8;
constexpr int MXP_HALF = 128 * 128;        // bytes of one X half-tile (128 rows x 128 k)
constexpr int MXP_SLOT = 2 * MXP_HALF;     // X0 X1 of one K-tile
constexpr int MXP_SLOTS = 4;               // X ring depth in K-tiles
constexpr int MXP_REC = 4 * 1024 + 256;    // one quad of one 16-row group: codes + scale dwords

// One 1-KB LDS-DMA piece from sbase + voff (per lane): lane l's 16 bytes land at lds_addr + 16 l
// (f8pgemm.hip's f8p_glds16)
__device__ __forceinline__ void mxp_glds16(uint32_t voff, const void* sbase, uint32_t lds_addr) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory");
}

__device__ __forceinline__ void mxp_barrier() { asm volatile("s_barrier" ::: "memory"); }
__device__ __forceinline__ void mxp_lgkm_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int N>
__device__ __forceinline__ void mxp_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}

template <int V>
using mxp_int = std::integral_constant<int, V>;

__global__ void __launch_bounds__(512, 1)
    mx4pgemm_kernel(const uint8_t* __restrict__ X, const float* __restrict__ sx, const uint8_t* __restrict__ W,
                    uint16_t* __restrict__ out, int M, int N, int K, int ldo, int tiles_m, int tiles_n, int wnw,
                    uint32_t wbytes) {
  __shared__ __attribute__((aligned(16))) char smem[MXP_SLOTS * MXP_SLOT];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = w >> 2, wc = w & 3;

  // ---- tile of this workgroup: XCD-local id, then GROUP_M-row groups sweeping the N tiles
  const int nwg = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int per_group = MXP_GROUP_M * tiles_n;
  const int first_m = (id / per_group) * MXP_GROUP_M;
  const int gsz = min(tiles_m - first_m, MXP_GROUP_M);
  const int in_group = id % per_group;
  const int m0 = (first_m + in_group % gsz) * MXP_BM;
  const int n0 = (in_group / gsz) * MXP_BN;
  const int nk = K / MXP_BK;
  const int nqk = (nk + 3) >> 2;             // quads of the padded K

  // ---- X DMA sources (byte offsets): pieces w and w + 8 of half h = image rows 8 p .. 8 p + 7
  // (lane: row lane >> 3, chunk lane & 7 through the swizzle)
  uint32_t vx[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = 8 * (w + 8 * i) + (lane >> 3);
      const int trow = (r >> 6) * 128 + 64 * h + (r & 63);
      const int c = (lane & 7) ^ (r & 7);
      vx[h][i] = (uint32_t)min(m0 + trow, M - 1) * (uint32_t)K + 16u * c;
    }
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(mxp_lds_t*)smem + w * 1024);
  // K-tile kt's half h into ring slot `slot`.  Past the end the source is K-tile nk - 1 again, into a
  // slot nobody reads: every step issues the same number of pieces, so the wait counts are constants
  // and the K loop has no branch, and no block at or past K / 128 is ever staged
  auto issue_x = [&](int kt, int slot, int h) {
    const uint8_t* src = X + (size_t)min(kt, nk - 1) * MXP_BK;
    const uint32_t la = lds0 + slot * MXP_SLOT + h * MXP_HALF;
    mxp_glds16(vx[h][0], src, la);
    mxp_glds16(vx[h][1], src, la + 8192);
  };

  // ---- W: n-tile j of this wave is 16-row group n0 / 16 + 4 wc + j; its quad-0 record, then
  // quad q at + q * nw * 4352, block b's codes at + 1024 b + 16 lane, scale dwords at + 4096 + 4 lane
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)W, (short)0, (int)wbytes, 0x00020000);
  uint32_t wbase[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int G = min(n0 / 16 + 4 * wc + j, N / 16 - 1);
    wbase[j] = __builtin_amdgcn_readfirstlane((uint32_t)((G / wnw) * nqk * wnw + G % wnw) * (uint32_t)MXP_REC);
  }
  const uint32_t qstep = (uint32_t)wnw * MXP_REC;
  const int cvoff = lane * 16, svoff = 4096 + lane * 4;
  uint4 wr[4][4];        // [block in quad][n-tile]: three of the four slots live at any point
  uint32_t sc[4], scn[4];   // scale dwords per n-tile: this quad's, the next quad's
  auto load_w = [&](int blk, auto Slot) {
    constexpr int slot = decltype(Slot)::value;
    const uint32_t so = (uint32_t)min(blk >> 2, nqk - 1) * qstep + (uint32_t)(blk & 3) * 1024u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const mxp_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrs, cvoff, (int)(wbase[j] + so), 0);
      wr[slot][j] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  auto load_scn = [&](int q) {
    const uint32_t so = (uint32_t)min(q, nqk - 1) * qstep;
#pragma unroll
    for (int j = 0; j < 4; ++j) scn[j] = __builtin_amdgcn_raw_buffer_load_b32(wrs, svoff, (int)(wbase[j] + so), 0);
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // X fragment read: image row 64 grp + 16 i + (lane & 15) of the half, chunk 4 hh + (lane >> 4)
  // through the swizzle (row & 7 == lane & 7)
  // X fragment read: image row 64 grp + 16 i + (lane & 15) of the half, chunk 4 hh + (lane >> 4)
  // through the swizzle (row & 7 == lane & 7).  One base register per hh and ring half (a ds_read
  // offset has 16 bits), the rest a constant
  const int swz = lane & 7;
  uint32_t xrd[2][2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    xrd[0][hh] = (64 * grp + (lane & 15)) * 128 + (((4 * hh + (lane >> 4)) ^ swz) << 4);
    xrd[1][hh] = xrd[0][hh] + 2 * MXP_SLOT;
    asm volatile("" : "+v"(xrd[1][hh]));     // keep it a register of its own
  }
  auto rd_x = [&](int slot, int h, int i, int hh) {   // all four compile-time
    return *reinterpret_cast<const uint4*>(smem + xrd[slot >> 1][hh] + (slot & 1) * MXP_SLOT + h * MXP_HALF +
                                           i * 16 * 128);
  };

  // ---- prologue: X of tiles 0-2, scales of quad 0, W of tiles 0 and 1; X(0) landed in every wave
  issue_x(0, 0, 0);
  issue_x(0, 0, 1);
  issue_x(1, 1, 0);
  issue_x(1, 1, 1);
  issue_x(2, 2, 0);
  issue_x(2, 2, 1);
  load_scn(0);
  load_w(0, mxp_int<0>{});
  load_w(1, mxp_int<1>{});
  mxp_wait_barrier<20>();
  if (grp == 1) mxp_barrier();   // the stagger: group 1 runs one barrier behind group 0

  uint4 xf[4][2];
  // K-tile kt = block b of its quad (kt & 3 == b at every call, so the ring slots are compile-time).
  // No branch inside: a run of steps is one basic block, which keeps each MFMA part where it is
  // written (an accumulator's next use is the next step's MFMA, and the compiler sinks towards it)
  auto step = [&](auto Bc, int kt) {
    constexpr int b = decltype(Bc)::value;
    // ======== segment A: load part
    issue_x(kt + 3, (b + 3) & 3, 0);
    if constexpr (b == 2) load_scn((kt + 2) >> 2);
    load_w(kt + 2, mxp_int<(b + 2) & 3>{});
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) xf[i][hh] = rd_x(b, 0, i, hh);
    mxp_wait_barrier<(b >= 2 ? 20 : 16)>();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (b == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[j] = scn[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mx4_mfma<b>(wr[b][j], sc[j], xf[i][0], xf[i][1], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    mxp_barrier();
    // ======== segment B: load part
    issue_x(kt + 3, (b + 3) & 3, 1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) xf[i][hh] = rd_x(b, 1, i, hh);
    mxp_lgkm_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 + i][j] = mx4_mfma<b>(wr[b][j], sc[j], xf[i][0], xf[i][1], acc[4 + i][j]);
    __builtin_amdgcn_sched_barrier(0);
    mxp_barrier();
  };

  // whole quads, then the K / 128 % 4 blocks of the last one: a block at or past K / 128 is never
  // multiplied
  int kt = 0;
  for (; kt + 4 <= nk; kt += 4) {
    step(mxp_int<0>{}, kt);
    step(mxp_int<1>{}, kt + 1);
    step(mxp_int<2>{}, kt + 2);
    step(mxp_int<3>{}, kt + 3);
  }
  if (nk - kt > 0) step(mxp_int<0>{}, kt);
  if (nk - kt > 1) step(mxp_int<1>{}, kt + 1);
  if (nk - kt > 2) step(mxp_int<2>{}, kt + 2);
  // the pieces past the end are still in flight towards this workgroup's LDS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: lane holds rows m = mw + 16 i + (lane & 15) (segment A's m-tiles i < 4 = tile rows
  // 128 grp + 16 i, segment B's = 128 grp + 64 + 16 (i - 4)), columns nq + 16 j .. + 3
  const int mw = m0 + grp * 128 + (lane & 15);
  const int nq = n0 + wc * 64 + 4 * (lane >> 4);
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
              make_uint2(pack2bf(acc[i][j][0] * s, acc[i][j][1] * s), pack2bf(acc[i][j][2] * s, acc[i][j][3] * s));
      }
    }
  }
  if (grp == 0) mxp_barrier();   // matches group 1's stagger barrier
}

}  // namespace

// Y = diag(sx) (X8 . dequant(W4)^T), bf16: x [M, K] e4m3fn row-major, sx [M] fp32, w in the quad
// layout cfc_mx4dgemm_pack wrote for this same bn; bf16 rows at out + m * ldo (out points at the
// first column of the written range [0, N), 8-byte aligned).  M >= 1, N % 64 == 0, K % 128 == 0,
// bn in {64, 96, 112, 128}, ldo % 4 == 0, ldo >= N, X and the padded W under 4 GiB.  Returns a
// negative code (nothing launched) for anything else.
CFC_API int cfc_mx4pgemm(const void* x, const float* sx, const void* w, int M, int N, int K, int bn, void* out, int ldo,
                         hipStream_t stream) {
  if (M < 1 || N <= 0 || N % 64 || K <= 0 || K % 128 || !x || !sx || !w || !out) return -1;
  if (bn != 64 && bn != 96 && bn != 112 && bn != 128) return -5;
  if (ldo < N || ldo % 4 || ((uintptr_t)out & 7) || ((uintptr_t)x & 15) || ((uintptr_t)w & 15)) return -6;
  const uint64_t wbytes = (uint64_t)((N + bn - 1) / bn) * ((K / 128 + 3) / 4) * (bn / 16) * MXP_REC;
  if ((uint64_t)M * K >= (1ull << 32) || wbytes >= (1ull << 32)) return -6;
  const int tm = (M + MXP_BM - 1) / MXP_BM, tn = (N + MXP_BN - 1) / MXP_BN;
  if ((long long)tm * tn >= (1ll << 31)) return -6;
  mx4pgemm_kernel<<<tm * tn, 512, 0, stream>>>((const uint8_t*)x, sx, (const uint8_t*)w, (uint16_t*)out, M, N, K, ldo,
                                               tm, tn, bn / 16, (uint32_t)wbytes);
  return CFC_CHECK_LAUNCH();
}
