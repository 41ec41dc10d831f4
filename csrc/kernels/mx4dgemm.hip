// W4A8 MXFP4 decode GEMM for gfx950 at 1 <= M <= 128 rows:
//   Y[M, N] = diag(sx) . (X8[M, K] . dequant(W4)[N, K]^T)
// W4: OCP MXFP4 -- e2m1 codes, two per byte (value 2 j in the low nibble of byte j), and one e8m0
// scale per 32 consecutive k of a row (quant_mxfp4_weight).  X8 OCP e4m3fn with sx fp32 per row
// (rmsnorm_fp8 / silu_mul_fp8 / quant_fp8_rows / splitk_residual_rmsnorm_fp8), fp32 accumulate.  A
// decode projection is a weight stream (dgemm.hip, ROOFLINE.md); 4.25 bits per weight are 0.53 of
// the FP8 stream and 0.27 of the bf16 one, and v_mfma_scale_f32_16x16x128_f8f6f4 takes the codes
// and their block scales as they lie in memory: the scale multiplies inside the matrix unit, so
// there is no dequantisation and no VALU work per weight (qdgemm.hip, the other 4-bit route,
// dequantises on the VALU and is instruction-bound at ~1 TB/s).
//
// This is f8dgemm.hip's streamer -- compute waves that own 16 W rows and keep a register ring of
// fragments loaded straight from HBM, X staged by loader waves with LDS-DMA, a 1-D grid remapped
// XCD-locally (xcd_remap), zero-row padding to whole workgroups, the same two epilogues -- with
// four things redesigned for 4-bit fragments.
//
// 1. Fragment and scale layout (cfc_mx4dgemm_pack).  The unit is a QUAD, four consecutive 128-k
//    blocks of one wave's 16 rows, 4352 B:
//      Wp[ceil(N / BN)][ceil(K / 512)][BN / 16]{ codes [4 blocks][64 lanes][16 B], scales [64 lanes][4 B] }
//    Lane l = 16 g + r of block b holds the 32 codes of row r at k = 128 (4 q + b) + 32 g .. + 31:
//    a fragment is 1 KB contiguous in lane order, one 16-byte load per lane (the form dgemm.hip
//    measured at 6.0 TB/s against 3.8-4.2 for strided fragments).  The lane's scale dword holds, in
//    byte b, the e8m0 scale of exactly those 32 values for block b of the quad: one 256-B load per
//    wave serves four blocks and the instruction's op_sel picks the byte, so a scale costs 1/16 of
//    a load instruction per MFMA and never an ALU instruction.  op_sel is an immediate, hence the
//    quad: inside it b is a compile-time constant whatever block the K part starts at.  Codes and
//    scales of a quad are adjacent and a workgroup's slice (BN rows x its K part) is ONE contiguous
//    span read front to back.  K is padded to whole quads and N to whole workgroups with zero codes
//    under scale 1.0 (e8m0 127; 255 is NaN and never written).
//    K parts are whole 128-k blocks and may begin and end inside a quad: such a part loads its two
//    edge quads whole (at most 6 KB per wave that it does not use; nothing when the part boundaries
//    are multiples of 512 k, as at the splits the cost model picks for Mistral-7B's projections:
//    1, 4 or 8 on K = 4096, 4 on K = 14336) and skips the blocks outside [kb, ke) with a
//    wave-uniform branch that holds no vector-memory load.
//
// 2. A lane's 32 values are exactly one MX block, and which k they are now matters.  f8dgemm.hip
//    needs no knowledge of where the hardware puts k inside a lane: with two 8-bit operands byte i
//    of lane group g meets byte i of lane group g, and the sum over k is order-free.  With a 4-bit
//    A against an 8-bit B that no longer holds -- the two operands spread the instruction's K
//    index over the lanes DIFFERENTLY, measured on an MI355X by reading W back through one-hot rows
//    of X:
//      A (e2m1, 16 B per lane): lane group g holds K = 32 g .. 32 g + 31, value j in nibble j;
//      B (e4m3, 32 B per lane): lane group g holds K = 16 g .. + 15 in its first 16 bytes and
//                               K = 64 + 16 g .. + 15 in its second 16;
//      the scale byte of lane l multiplies that lane's own 32 A values.
//    So the A lane's 32 values are 32 CONSECUTIVE k (the packer gives it one MX block of its row)
//    and its single scale is right for all of them, while the X fragment the same lane must feed
//    is chunks (16 B) g and 4 + g of the row's 128-byte stage, not 2 g and 2 g + 1.  An earlier
//    version of this kernel permuted the LDS-DMA's source chunks so that the lane read 2 g and
//    2 g + 1; it paired W's k 16..31 with X's k 32..47.  The X image is therefore f8dgemm.hip's,
//    unpermuted: chunk c of row r at r * 128 + ((c ^ (r & 7)) << 4), the swizzle applied through
//    the DMA's source address, and a fragment read is two ds_read_b128 per row tile, lane (r, g)
//    reading chunk g, then chunk 4 + g.  Its bank argument holds word for word: LDS has 64 4-byte
//    banks = 16 chunk slots per 256-B bank row; rows r and r + 1 fill one bank row; within one
//    instruction the 64 lanes hit slot 8 (r & 1) + ((4 h + g) ^ (r & 7)), h = 0 / 1.  For fixed
//    r & 1 the 4 x 4 pairs (g, r & 7) cover the 8 slots of that half exactly twice (bit 2 from r,
//    bit 1 from g ^ r, bit 0 from g), and with r, r + 8 every one of the 16 slots is read by
//    exactly 4 lanes: the four 256-B passes a 1-KB read needs anyway.
//
// 3. Ring depth.  A block is 16 B per lane, not 32.  The ring holds DQ = 4 quads = 16 blocks of
//    128 k, twice f8dgemm.hip's depth in k at the same 17 KB per wave in flight.  Per lane: ring
//    4 x (16 + 1) = 68 VGPRs, accumulators 4 per row tile = 32 at M = 128, two X fragments 16, the
//    zero upper half of the A operand and addresses: see the measured counts below.  Every ring
//    load is unconditional -- refills past the end of the part re-read its last (real) quad -- and
//    the ring's are the wave's only vector-memory loads, so the counted vmcnt waits stay exact.
//    The 9-wave BN = 128 workgroup (three waves on one SIMD: 168 VGPRs) keeps the same depth.
//
// 4. Balance at M = 128.  Per 1 KB of codes a wave issues what f8dgemm.hip issues per 2 KB: one
//    MFMA per row tile, 8 passes (32 cycles) each with an 8-bit B operand.  At M = 128 that is
//    256 cycles per KB and SIMD, 4 SIMDs x 256 CUs x 2.4 GHz / 256 = 9.6 TB/s of codes if the
//    matrix unit never idles, against a ~6.4 TB/s stream: the margin that is 3x in the FP8 kernel
//    is 1.5x here, at M = 64 it is 3x.  Reasoned only; nobody has measured this instruction's rate
//    with an FP4 operand.  ops/kernels.py mx4dgemm_config therefore carries its own cost model:
//    17/32 byte per weight and the larger of the stream and the MFMA time per workgroup.
//
// Instruction: mx4_mfma in common.h -- cbsz = 4 (A = e2m1, the low four dwords of the operand),
// B = e4m3 under the constant e8m0 scale 1.0.  A = W fragment, B = X fragment, so a lane ends up
// with X row 16 t + (l & 15) at the four consecutive W rows n0 + 16 w + 4 (l >> 4) + i: one 16-byte
// (fp32) or 8-byte (bf16) store per row tile.
//
// Epilogues, both after acc * sx[m]: fp32 split-K slabs [split][M][ldo] stored write-through, plain
// stores and no atomics (bit-reproducible; splitk_reduce, splitk_residual_rmsnorm(_fp8),
// rope_kv_write_part and the fused RoPE attention prologue read them unchanged), or bf16 [M][ldo]
// at split 1.  part / out may be a column range of a wider buffer.
//
// Compiled for gfx950: 90 / 102 / 112 / 128 VGPRs at BM = 16 / 32 / 64 / 128, the same at every BN;
// no scratch and no spill at any of the 32 instantiations (4 BM x 4 BN x 2 epilogues).
// Measured on one MI355X: ROOFLINE.md, "MXFP4 decode GEMM" (scripts/probes/mx4dgemm_probe.py).
// Taken over from dgemm.hip / f8dgemm.hip, not re-measured: contiguous 1-KB pieces, nontemporal
// weight loads, the loader-wave split, write-through slabs.  Reasoned only: the bank argument, the
// MFMA balance.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void mx_lds_t;
typedef unsigned int mx_u32x4 __attribute__((ext_vector_type(4)));

enum { MX_PART = 0, MX_BF16 = 1 };
constexpr int MX_REC = 4 * 1024 + 256;     // bytes of one quad of one wave: codes + scale dwords

template <int BN>
constexpr int mx_loaders() { return BN / 16 >= 7 ? 1 : 2; }

template <int BM, int BN>
struct MxShape {
  static constexpr int NW = BN / 16;                    // compute waves
  static constexpr int LOADERS = mx_loaders<BN>();
  static constexpr int WAVES = NW + LOADERS;
  static constexpr int MT = BM / 16;                    // row tiles per compute wave
  static constexpr int DQ = 4;                          // W register ring depth in quads (16 blocks)
  static constexpr int XSTAGE = BM * 128;               // X bytes per 128-k stage
  static constexpr int XP = BM / 8 / LOADERS;           // 1-KB DMA pieces per loader wave and stage
  static constexpr int NSX_BASE = BM == 128 ? 6 : 8;    // X ring slots, as f8dgemm.hip
  static constexpr int NSX = (NSX_BASE - 2 <= 63 / XP ? NSX_BASE : 2 + 63 / XP);
  static_assert(XP >= 1 && XP * LOADERS * 8 == BM, "X stage must divide over the loader waves");
};

// One 1-KB LDS-DMA piece: lane l's 16 source bytes land at lds_addr + 16 l (f8dgemm.hip's f8_glds16)
__device__ __forceinline__ void mx_glds16(const void* gsrc, uint32_t lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}

template <int N>
__device__ __forceinline__ void mx_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(N) : "memory");
}

template <int P, int MAXA>
__device__ __forceinline__ void mx_wait_ahead(int ahead) {
  if constexpr (MAXA == 0) {
    mx_wait_barrier<0>();
  } else {
    if (ahead >= MAXA) mx_wait_barrier<MAXA * P>();
    else mx_wait_ahead<P, MAXA - 1>(ahead);
  }
}

// compute waves: W loads stay in flight across the barrier, the LDS reads of the previous stage retire
__device__ __forceinline__ void mx_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct MxQuad {
  uint4 c[4];      // the lane's 32 codes of each of the quad's four blocks
  uint32_t sc;     // their four e8m0 scales, byte b for block b
};

template <int BM, int BN, int EPI>
__global__ void __launch_bounds__((64 * MxShape<BM, BN>::WAVES), 1)
    mx4dgemm_kernel(const uint8_t* __restrict__ X, const float* __restrict__ sx, const uint8_t* __restrict__ W, int M,
                    int N, int K, int ntiles, int split, float* __restrict__ part, uint16_t* __restrict__ out,
                    long long slab, int ldo) {
  using S = MxShape<BM, BN>;
  constexpr int NW = S::NW;
  constexpr int DQ = S::DQ;
  __shared__ __attribute__((aligned(16))) char smem[S::NSX * S::XSTAGE];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // logical block: the blocks of one XCD take consecutive ids, i.e. (mostly) one K part
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int ks = lid / ntiles, tile = lid % ntiles;
  const int n0 = tile * BN;
  const int nks = K >> 7;
  const int kb = (int)((long)ks * nks / split), ke = (int)((long)(ks + 1) * nks / split);
  const int nst = ke - kb;                              // blocks of the part, >= 1: split <= K / 128
  const int q0 = kb >> 2, nq = ((ke - 1) >> 2) - q0 + 1;   // the quads that hold them
  const int g = lane >> 4;
  // K-order rotation (dgemm.hip) in whole quads: workgroup lid starts at quad q0 + rotq and wraps.
  // The blocks of [kb, ke) met on that walk, ascending inside each quad, are the part rotated by
  // rot blocks, which is all the X loaders need to know
  const int rotq = (int)((unsigned)lid * 37u % (unsigned)nq);
  const int rot = max(4 * (q0 + rotq), kb) - kb;
  auto phys = [&](int s) { s += rot; return s >= nst ? s - nst : s; };
  auto physq = [&](int i) { i += rotq; return q0 + (i >= nq ? i - nq : i); };

  if (w >= NW) {
    // ---------------- X loader wave l: rows 8 XP l .. 8 XP (l + 1) - 1 of the X stage image
    const int l = w - NW;
    const int prow = lane >> 3, pch = (lane & 7) ^ prow;   // row & 7 == prow for every piece
    const uint8_t* xsrc[S::XP];
#pragma unroll
    for (int i = 0; i < S::XP; ++i) {
      const int m = min(8 * S::XP * l + 8 * i + prow, M - 1);   // rows past M: results dropped
      xsrc[i] = X + (size_t)m * K + (size_t)kb * 128 + 16 * pch;
    }
    const uint32_t lds0 =
        __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(mx_lds_t*)smem + 8 * S::XP * l * 128);
    auto issue = [&](int st, int slot) {
#pragma unroll
      for (int i = 0; i < S::XP; ++i) mx_glds16(xsrc[i] + phys(st) * 128, lds0 + slot * S::XSTAGE + i * 1024);
    };
#pragma unroll
    for (int p = 0; p < S::NSX - 1; ++p)
      if (p < nst) issue(p, p);
    int slot = 0;
    for (int st = 0; st < nst; ++st) {
      mx_wait_ahead<S::XP, S::NSX - 2>(nst - 1 - st);
      // the slot read in iteration st - 1 is free once every wave passed this barrier
      if (st + S::NSX - 1 < nst) issue(st + S::NSX - 1, slot == 0 ? S::NSX - 1 : slot - 1);
      slot = slot + 1 == S::NSX ? 0 : slot + 1;
    }
    return;
  }

  // ---------------- compute wave w: W rows n0 + 16 w + (lane & 15)
  MxQuad ring[DQ];
  const int nqk = (nks + 3) >> 2;                       // quads of the whole (padded) K
  const int tile_bytes = nqk * NW * MX_REC;
  const uint8_t* span = W + (size_t)tile * (size_t)tile_bytes;
  const uint32_t span_lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)span);
  const uint32_t span_hi = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)span >> 32));
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(((uintptr_t)span_hi << 32) | span_lo), (short)0, tile_bytes, 0x00020000);
  const int cvoff = lane * 16, svoff = 4096 + lane * 4;
  auto load_quad = [&](int q, MxQuad& dst) {            // q: quad of K; nontemporal, once-read bytes
    const int so = __builtin_amdgcn_readfirstlane((q * NW + w) * MX_REC);
    dst.sc = __builtin_amdgcn_raw_buffer_load_b32(wrs, svoff, so, 2);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const mx_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrs, cvoff, so + 1024 * b, 2);
      dst.c[b] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
#pragma unroll
  for (int p = 0; p < DQ; ++p) load_quad(physq(min(p, nq - 1)), ring[p]);
  f32x4_t acc[S::MT];
#pragma unroll
  for (int i = 0; i < S::MT; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int xoff = (lane & 15) * 128;
  const int c0 = (g ^ (lane & 7)) << 4, c1 = ((4 + g) ^ (lane & 7)) << 4;
  int xslot = 0;
  // block B of quad q (a compile-time op_sel), if the part holds it: one X stage, one MFMA per row tile
  auto block = [&](auto B, int q, const MxQuad& wq) {
    constexpr int b = decltype(B)::value;
    const int blk = 4 * q + b;
    if (blk < kb || blk >= ke) return;                  // wave-uniform; an edge quad of the part
    mx_barrier();                                       // the X stage of this block is in LDS
    const char* ximg = smem + xslot * S::XSTAGE + xoff;
#pragma unroll
    for (int i = 0; i < S::MT; ++i) {
      const uint4 x0 = *reinterpret_cast<const uint4*>(ximg + i * 16 * 128 + c0);
      const uint4 x1 = *reinterpret_cast<const uint4*>(ximg + i * 16 * 128 + c1);
      acc[i] = mx4_mfma<b>(wq.c[b], wq.sc, x0, x1, acc[i]);
    }
    xslot = xslot + 1 == S::NSX ? 0 : xslot + 1;
  };
  auto compute = [&](int q, const MxQuad& wq) {
    block(std::integral_constant<int, 0>{}, q, wq);
    block(std::integral_constant<int, 1>{}, q, wq);
    block(std::integral_constant<int, 2>{}, q, wq);
    block(std::integral_constant<int, 3>{}, q, wq);
  };

  // Quad i of the walk lives in ring slot i % DQ; after computing it the slot is refilled with quad
  // i + DQ, or past the end of the part with its last quad again (real bytes, never computed twice)
  int qi = 0;
  for (; qi + DQ <= nq; qi += DQ) {
#pragma unroll
    for (int u = 0; u < DQ; ++u) {
      compute(physq(qi + u), ring[u]);
      load_quad(physq(min(qi + u + DQ, nq - 1)), ring[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < DQ; ++u)
    if (qi + u < nq) compute(physq(qi + u), ring[u]);

  // ---- epilogue: lane holds X row 16 i + (lane & 15) at the W rows nc .. nc + 3
  const int nc = n0 + 16 * w + 4 * g;
  if (nc >= N) return;                       // the padding of the last workgroup (wave-uniform: N % 16 == 0)
  const int mr = lane & 15;
  if constexpr (EPI == MX_PART) {
    // write-through (sc1) 16-byte stores through a buffer descriptor of this part's slab
    const float* base = part + (size_t)ks * slab;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)base >> 32));
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uintptr_t)hi << 32) | lo), (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < S::MT; ++i) {
      const int m = mr + 16 * i;
      if (m < M) {
        const float s = sx[m];
        const mx_u32x4 v = {__float_as_uint(acc[i][0] * s), __float_as_uint(acc[i][1] * s),
                            __float_as_uint(acc[i][2] * s), __float_as_uint(acc[i][3] * s)};
        __builtin_amdgcn_raw_buffer_store_b128(v, prs, (m * ldo + nc) * 4, 0, 16);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < S::MT; ++i) {
      const int m = mr + 16 * i;
      if (m < M) {
        const float s = sx[m];
        *reinterpret_cast<uint2*>(out + (size_t)m * ldo + nc) =
            make_uint2(pack2bf(acc[i][0] * s, acc[i][1] * s), pack2bf(acc[i][2] * s, acc[i][3] * s));
      }
    }
  }
}

struct MxArgs {
  const uint8_t* x;
  const float* sx;
  const uint8_t* w;
  int M, N, K, split, epi;
  float* part;
  uint16_t* out;
  long long slab;
  int ldo;
  hipStream_t st;
};

template <int BM, int BN>
int mx_launch(const MxArgs& a) {
  const int ntiles = (a.N + BN - 1) / BN;
  const dim3 grid(ntiles * a.split);
  const int threads = 64 * MxShape<BM, BN>::WAVES;
  if (a.epi == MX_PART)
    mx4dgemm_kernel<BM, BN, MX_PART><<<grid, threads, 0, a.st>>>(a.x, a.sx, a.w, a.M, a.N, a.K, ntiles, a.split, a.part,
                                                                 a.out, a.slab, a.ldo);
  else
    mx4dgemm_kernel<BM, BN, MX_BF16><<<grid, threads, 0, a.st>>>(a.x, a.sx, a.w, a.M, a.N, a.K, ntiles, a.split, a.part,
                                                                 a.out, a.slab, a.ldo);
  return CFC_CHECK_LAUNCH();
}

template <int BM>
int mx_rows(const MxArgs& a, int bn) {
  switch (bn) {
    case 64: return mx_launch<BM, 64>(a);
    case 96: return mx_launch<BM, 96>(a);
    case 112: return mx_launch<BM, 112>(a);
    case 128: return mx_launch<BM, 128>(a);
    default: return -5;
  }
}

// Row-major codes [N][K / 2] + scales [N][K / 32] -> the quad layout for bn-row workgroups; rows
// past N and blocks past K: zero codes, scale 127.  One thread per 16 bytes of the output (a
// lane's 16 code bytes of one block, or the scale dwords of four lanes).
__global__ void mx4dgemm_pack_kernel(const uint8_t* __restrict__ C, const uint8_t* __restrict__ Sc,
                                     uint4* __restrict__ Wp, int N, int K, int nw, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  constexpr int PER = MX_REC / 16;           // 272: 256 code pieces + 16 pieces of scale dwords
  const int j = (int)(i % PER);
  const size_t rec = i / PER;
  const int nks = K >> 7, nqk = (nks + 3) >> 2;
  const int w = (int)(rec % nw);
  const size_t t2 = rec / nw;
  const int q = (int)(t2 % nqk), t = (int)(t2 / nqk);
  const int row0 = 16 * (t * nw + w);
  uint4 v;
  if (j < 256) {
    const int b = j >> 6, l = j & 63, row = row0 + (l & 15), blk = 4 * q + b;
    v = make_uint4(0, 0, 0, 0);
    if (row < N && blk < nks) v = *reinterpret_cast<const uint4*>(C + (size_t)row * (K / 2) + 64 * blk + 16 * (l >> 4));
  } else {
    uint32_t d[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = 4 * (j - 256) + e, row = row0 + (l & 15);
      d[e] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int blk = 4 * q + b;
        const uint32_t s = (row < N && blk < nks) ? Sc[(size_t)row * (K / 32) + 4 * blk + (l >> 4)] : 127u;
        d[e] |= s << (8 * b);
      }
    }
    v = make_uint4(d[0], d[1], d[2], d[3]);
  }
  Wp[i] = v;
}

}  // namespace

// Y = diag(sx) (X8 . dequant(W4)^T): x [M, K] e4m3fn row-major, sx [M] fp32, w in the quad layout
// cfc_mx4dgemm_pack wrote for this same bn.  1 <= M <= 128, N % 64 == 0, K % 128 == 0, bn in
// {64, 96, 112, 128}, 1 <= split <= K / 128.
//   epi 0: fp32 slabs, part p's row m at part + p * slab + m * ldo (16-byte aligned, ldo % 4 == 0);
//   epi 1 (split 1): bf16 rows at out + m * ldo (8-byte aligned).
// part / out point at the first column of the written range [0, N).  Returns a negative code
// (nothing launched) for anything else.
CFC_API int cfc_mx4dgemm(const void* x, const float* sx, const void* w, int M, int N, int K, int split, int epi, int bn,
                         float* part, void* out, long long slab, int ldo, hipStream_t stream) {
  if (M < 1 || M > 128 || N <= 0 || N % 64 || K <= 0 || K % 128 || !x || !sx || !w) return -1;
  if (split < 1 || split > K / 128) return -3;
  if (epi == MX_PART ? !part : (epi != MX_BF16 || !out || split != 1)) return -2;
  if (ldo < N || ldo % 4 || slab % 4 || slab < 0 || (long long)M * ldo >= (1ll << 29)) return -6;
  if (epi == MX_PART ? ((uintptr_t)part & 15) : ((uintptr_t)out & 7)) return -6;
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15)) return -6;
  if ((long long)((K / 128 + 3) / 4) * (bn / 16) * MX_REC >= (1ll << 31)) return -6;
  const MxArgs a{(const uint8_t*)x, sx, (const uint8_t*)w, M, N, K, split, epi, part, (uint16_t*)out, slab, ldo, stream};
  if (M <= 16) return mx_rows<16>(a, bn);
  if (M <= 32) return mx_rows<32>(a, bn);
  if (M <= 64) return mx_rows<64>(a, bn);
  return mx_rows<128>(a, bn);
}

// Row-major MXFP4 W (codes [N][K / 2], e8m0 scales [N][K / 32]) -> the quad layout for bn-row
// workgroups: ceil(N / bn) * ceil(K / 512) * (bn / 16) * 4352 bytes at wp.  N % 16 == 0,
// K % 128 == 0, bn in {64, 96, 112, 128}.
CFC_API int cfc_mx4dgemm_pack(const void* codes, const void* scales, void* wp, int N, int K, int bn, hipStream_t stream) {
  if (N <= 0 || N % 16 || K <= 0 || K % 128 || !codes || !scales || !wp || codes == wp) return -1;
  if (bn != 64 && bn != 96 && bn != 112 && bn != 128) return -5;
  if (((uintptr_t)codes & 15) || ((uintptr_t)wp & 15)) return -6;
  const size_t total = (size_t)((N + bn - 1) / bn) * ((K / 128 + 3) / 4) * (bn / 16) * (MX_REC / 16);
  mx4dgemm_pack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>((const uint8_t*)codes, (const uint8_t*)scales,
                                                                           (uint4*)wp, N, K, bn / 16, total);
  return CFC_CHECK_LAUNCH();
}
