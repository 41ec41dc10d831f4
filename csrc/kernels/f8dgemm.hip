// W8A8 FP8 decode GEMM for gfx950 at 1 <= M <= 128 rows:
//   Y[M, N] = diag(sx) . (X8[M, K] . W8[N, K]^T) . diag(sw)
// X8 / W8 OCP e4m3fn, sx fp32 per row of X (what rmsnorm_fp8 / silu_mul_fp8 / quant_fp8_rows emit),
// sw fp32 per row of W (quant_fp8_weight), fp32 accumulate.  At these M a projection is a weight
// stream (dgemm.hip header, ROOFLINE.md); the FP8 copy is half the bytes of the bf16 stream, so this
// kernel is dgemm.hip's streamer with one-byte elements and the 128-deep FP8 matrix instruction.
//
// Work split.  Workgroup = BN / 16 compute waves + 1-2 X-loader waves; it owns BN rows of W, ALL
// ceil(M / 16) row tiles of X (BM = 16 / 32 / 64 / 128) and one K part.  The grid is 1-D,
// ceil(N / BN) x split workgroups (BN from {64, 96, 112, 128} so that about one workgroup per CU
// runs: ops/kernels.py f8dgemm_config), remapped XCD-locally (xcd_remap) so that the workgroups of
// one XCD share a K part and therefore one X slice in that XCD's L2, as dgemm.hip does; a 2-D grid
// would leave the part index out of the remap.  K parts are whole 128-k blocks and may differ by one
// block.  N need not be a multiple of BN: the packed weight is padded with zero rows to whole
// workgroups, the waves past N stream the padding and store nothing.
//
// W never goes through LDS.  Compute wave w owns the 16 W rows n0 + 16 w .. + 15 for every row tile
// and loads its fragments from HBM straight into a D-stage register ring, D = 8 stages of one
// 128-k block = 2 KB per wave and stage, 16 KB per wave in flight (D = 6 for the 9-wave BN = 128
// workgroup).  Budget per lane: ring 8 D = 64 VGPRs, accumulators 4 per row tile = 32 at M = 128,
// two X fragments 16, addresses ~10: ~125 of the 256 a lane may hold at two waves per SIMD (the
// launch bound), so nothing spills and the ring could grow.  The wave's only vector-memory loads
// are the ring's, so the compiler's counted vmcnt waits are exact; every load is unconditional --
// the refills past the end of the K part re-read its last (real) stage -- so no branch join forces
// a vmcnt(0).  The ring is never read past the part.
//
// Packed layout (cfc_f8dgemm_pack): Wp[ceil(N / BN)][K / 128][BN / 16][2][64][16 B]; lane l of
// piece h of a fragment holds W[16-row tile row l & 15][128 kb + 64 h + 16 (l >> 4) .. + 15].  A
// fragment (16 rows x 128 k) is 2 KB contiguous, a lane's share is two whole 16-byte loads, and a
// workgroup's slice (BN rows x its K part) is ONE contiguous span read front to back.  The two
// 16-byte pieces of a lane are 1 KB apart rather than adjacent so that each load instruction reads
// one contiguous 1-KB piece in lane order, the form dgemm.hip measured at 6.0 TB/s against 3.8-4.2
// for strided fragments.  Which k of the 128 the hardware puts where inside a lane's 32 bytes need
// not be known: the reduction over k is order-free, and it is enough that lane group l >> 4,
// byte i, of the W fragment and of the X fragment carry the same k (qdgemm.hip pairs its
// dequantized fragments with X by the same argument).  Here both carry k = 64 (i / 16) +
// 16 (l >> 4) + i % 16 of the block.
//
// X (an L2 hit shared by all waves of the workgroup) is staged by the loader waves with LDS-DMA
// into a ring of NSX stage images, dgemm.hip's scheme unchanged: a 128-k FP8 stage of X is 128 B
// per row, exactly the bf16 kernel's 64-k stage.  Loader waves rather than qdgemm.hip's register
// double buffering because vmcnt counts in order: a compute wave that waited for an X load would
// wait for every older W load too and drain the ring once per stage; the loaders' counter is
// their own.  Image: chunk c (16 B) of row r at r * 128 + ((c ^ (r & 7)) << 4), the swizzle applied
// through the DMA's source address.  A fragment read is two ds_read_b128 per row tile, lane
// (row r = l & 15, group g = l >> 4) reading chunk g, then chunk 4 + g.  Bank argument: LDS has 64
// 4-byte banks = 16 chunk slots per 256-B bank row; rows r and r + 1 fill one bank row, and within
// one instruction the 64 lanes hit slot 8 (r & 1) + ((4 h + g) ^ (r & 7)).  For fixed r & 1 the
// pairs (g, r & 7) -- 4 x 4 values -- map onto the 8 slots of that half exactly twice each (bit 2
// from r, bit 1 from g ^ r, bit 0 from g), so with r and r + 8 every one of the 16 slots is read
// by exactly 4 of the 64 lanes: the four 256-B passes a 1-KB read needs anyway, no pass has two
// lanes on one slot.  (Chunks 2 g and 2 g + 1 -- a lane's 32 bytes adjacent -- would NOT do: bit 0
// of the chunk would be the same for all lanes of one instruction and half the slots idle.)  This
// is the bf16 kernel's read pattern (its kk = our h), for which the profile showed no conflicts;
// for this kernel the claim is reasoned, not measured.  Rows past M are clamped to row M - 1 on
// load and never stored.
//
// Instruction: v_mfma_f32_16x16x128_f8f6f4 (both operands e4m3, no block scales; f8_mfma in
// common.h, shared with the FP8 prefill GEMM f8pgemm.hip, which reads the same packed weight for
// M > 128 so that one FP8 weight copy serves prefill and decode): one instruction
// per 128-k block and row tile, and 2 LDS reads per 32 K flop where 16x16x32 fp8 needs 4 reads of
// 8 bytes.  A = W fragment, B = X fragment, so a lane ends up with X row 16 t + (l & 15) at the four
// consecutive W rows n0 + 16 w + 4 (l >> 4) + r: one 16-byte (fp32) or 8-byte (bf16) store per
// row tile.
//
// Epilogues, both after acc * (sx[m] * sw[n]): fp32 split-K slabs [split][M][ldo] (scaling is
// linear, so splitk_reduce, splitk_residual_rmsnorm(_fp8), rope_kv_write_part and the fused RoPE
// attention prologue read them unchanged), stored write-through like dgemm.hip's DG_PART_WT, plain
// stores and no atomics: bit-reproducible from replay to replay; or bf16 [M][ldo] at split 1.
// There is no SwiGLU epilogue: the next projection needs a per-row amax over the whole FFN width
// (silu_mul_fp8 follows the bf16 output).
//
// Measured / reasoned.  Measured on one MI355X: see ROOFLINE.md, "FP8 decode GEMM"
// (scripts/probes/f8dgemm_probe.py).  Taken over from dgemm.hip's measurements, not re-measured
// here: the contiguous 1-KB pieces, the nontemporal weight loads, the ring depth, the loader-wave
// split, write-through slabs.  Reasoned only: the bank argument above and the VGPR budget.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void f8_lds_t;
typedef unsigned int f8_u32x4 __attribute__((ext_vector_type(4)));

enum { F8_PART = 0, F8_BF16 = 1 };

// X-loader waves: fill the workgroup up to 8 waves (2 per SIMD), at least one, at most two
template <int BN>
constexpr int f8_loaders() { return BN / 16 >= 7 ? 1 : 2; }

template <int BM, int BN>
struct F8Shape {
  static constexpr int NW = BN / 16;                    // compute waves
  static constexpr int LOADERS = f8_loaders<BN>();
  static constexpr int WAVES = NW + LOADERS;
  static constexpr int MT = BM / 16;                    // row tiles per compute wave
  static constexpr int D = WAVES > 8 ? 6 : 8;           // W register ring depth (128-k stages)
  static constexpr int XSTAGE = BM * 128;               // X bytes per stage
  static constexpr int XP = BM / 8 / LOADERS;           // 1-KB DMA pieces per loader wave and stage
  // X ring slots (16-96 KB); a loader keeps NSX - 2 stages in flight at its wait, and vmcnt counts
  // at most 63 of its pieces
  static constexpr int NSX_BASE = BM == 128 ? 6 : 8;
  static constexpr int NSX = (NSX_BASE - 2 <= 63 / XP ? NSX_BASE : 2 + 63 / XP);
  static_assert(XP >= 1 && XP * LOADERS * 8 == BM, "X stage must divide over the loader waves");
};

// One 1-KB LDS-DMA piece: lane l's 16 source bytes land at lds_addr + 16 l (dgemm.hip's dg_glds16:
// inline asm so that the compiler orders nothing behind it; M0 saved and restored in the statement)
__device__ __forceinline__ void f8_glds16(const void* gsrc, uint32_t lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}

// loader waves: s_waitcnt vmcnt(n) + s_barrier as ONE statement (n = DMA pieces still allowed in flight)
template <int N>
__device__ __forceinline__ void f8_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(N) : "memory");
}

template <int P, int MAXA>
__device__ __forceinline__ void f8_wait_ahead(int ahead) {
  if constexpr (MAXA == 0) {
    f8_wait_barrier<0>();
  } else {
    if (ahead >= MAXA) f8_wait_barrier<MAXA * P>();
    else f8_wait_ahead<P, MAXA - 1>(ahead);
  }
}

// compute waves: their W loads stay in flight across the barrier; their LDS reads of the previous
// stage are retired first, so the loaders' next DMA into that slot cannot overtake them
__device__ __forceinline__ void f8_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// per-lane part of the offset in voff, the wave-uniform stage part in soff; nontemporal (once-read bytes)
__device__ __forceinline__ uint4 f8_ldw(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  const f8_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 2);
  return make_uint4(v.x, v.y, v.z, v.w);
}

template <int BM, int BN, int EPI>
__global__ void __launch_bounds__((64 * F8Shape<BM, BN>::WAVES), 1)
    f8dgemm_kernel(const uint8_t* __restrict__ X, const float* __restrict__ sx, const uint8_t* __restrict__ W,
                   const float* __restrict__ sw, int M, int N, int K, int ntiles, int split, float* __restrict__ part,
                   uint16_t* __restrict__ out, long long slab, int ldo) {
  using S = F8Shape<BM, BN>;
  constexpr int NW = S::NW;
  constexpr int D = S::D;
  __shared__ __attribute__((aligned(16))) char smem[S::NSX * S::XSTAGE];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // logical block: the blocks of one XCD take consecutive ids, i.e. (mostly) one K part
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int ks = lid / ntiles, tile = lid % ntiles;
  const int n0 = tile * BN;
  const int nks = K >> 7;
  const int kb = (int)((long)ks * nks / split), ke = (int)((long)(ks + 1) * nks / split);
  const int nst = ke - kb;                  // >= 1: split <= K / 128
  const int g = lane >> 4;
  // K-order rotation (dgemm.hip): workgroup lid walks its part starting at stage rot and wraps, so
  // the concurrent workgroups do not all read the same power-of-2-strided addresses in lock step
  const int rot = (int)((unsigned)lid * 37u % (unsigned)nst);
  auto phys = [&](int s) { s += rot; return s >= nst ? s - nst : s; };

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
        __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(f8_lds_t*)smem + 8 * S::XP * l * 128);
    auto issue = [&](int st, int slot) {
#pragma unroll
      for (int i = 0; i < S::XP; ++i) f8_glds16(xsrc[i] + phys(st) * 128, lds0 + slot * S::XSTAGE + i * 1024);
    };
#pragma unroll
    for (int p = 0; p < S::NSX - 1; ++p)
      if (p < nst) issue(p, p);
    int slot = 0;
    for (int st = 0; st < nst; ++st) {
      f8_wait_ahead<S::XP, S::NSX - 2>(nst - 1 - st);
      // the slot read in iteration st - 1 is free once every wave passed this barrier
      if (st + S::NSX - 1 < nst) issue(st + S::NSX - 1, slot == 0 ? S::NSX - 1 : slot - 1);
      slot = slot + 1 == S::NSX ? 0 : slot + 1;
    }
    return;
  }

  // ---------------- compute wave w: W rows n0 + 16 w + (lane & 15)
  uint4 ring[D][2];
  // the workgroup's span (tile n0 / BN over all of K; the K parts are sub-ranges of it) as a buffer
  // descriptor built from wave-uniform values
  const uint8_t* span = W + (size_t)tile * ((size_t)BN * K);
  const uint32_t span_lo = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)span);
  const uint32_t span_hi = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)span >> 32));
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)span_hi << 32) | span_lo), (short)0, BN * K, 0x00020000);
  const int wvoff = lane * 16;
  const int wsoff = __builtin_amdgcn_readfirstlane((kb * NW + w) * 2048);
  auto load_stage = [&](int s, uint4 (&dst)[2]) {     // s: physical stage of the part
    const int so = __builtin_amdgcn_readfirstlane(wsoff + s * NW * 2048);
    dst[0] = f8_ldw(wrs, wvoff, so);
    dst[1] = f8_ldw(wrs, wvoff, so + 1024);
  };
#pragma unroll
  for (int p = 0; p < D; ++p) load_stage(phys(min(p, nst - 1)), ring[p]);
  f32x4_t acc[S::MT];
#pragma unroll
  for (int i = 0; i < S::MT; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int xoff = (lane & 15) * 128;
  const int c0 = (g ^ (lane & 7)) << 4, c1 = ((4 + g) ^ (lane & 7)) << 4;
  int xslot = 0;
  auto compute = [&](const uint4 (&b)[2]) {
    const char* ximg = smem + xslot * S::XSTAGE + xoff;
#pragma unroll
    for (int i = 0; i < S::MT; ++i) {
      const uint4 x0 = *reinterpret_cast<const uint4*>(ximg + i * 16 * 128 + c0);
      const uint4 x1 = *reinterpret_cast<const uint4*>(ximg + i * 16 * 128 + c1);
      acc[i] = f8_mfma(b[0], b[1], x0, x1, acc[i]);
    }
    xslot = xslot + 1 == S::NSX ? 0 : xslot + 1;
  };

  // Stage s lives in ring slot s % D; after computing stage s the slot is refilled with stage
  // s + D, or past the end of the part with its last stage again (a real stage, never computed
  // twice: the tail below stops at nst)
  int st = 0;
  for (; st + D <= nst; st += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      f8_barrier();   // X stage st + u is in LDS
      compute(ring[u]);
      load_stage(phys(min(st + u + D, nst - 1)), ring[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < D; ++u) {
    if (st + u < nst) {
      f8_barrier();
      compute(ring[u]);
    }
  }

  // ---- epilogue: lane holds X row 16 i + (lane & 15) at the W rows nq .. nq + 3
  const int nq = n0 + 16 * w + 4 * g;
  if (nq >= N) return;                       // the padding of the last workgroup (wave-uniform: N % 16 == 0)
  const float4 swv = *reinterpret_cast<const float4*>(sw + nq);
  const int mr = lane & 15;
  if constexpr (EPI == F8_PART) {
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
        const f8_u32x4 v = {__float_as_uint(acc[i][0] * (s * swv.x)), __float_as_uint(acc[i][1] * (s * swv.y)),
                            __float_as_uint(acc[i][2] * (s * swv.z)), __float_as_uint(acc[i][3] * (s * swv.w))};
        __builtin_amdgcn_raw_buffer_store_b128(v, prs, (m * ldo + nq) * 4, 0, 16);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < S::MT; ++i) {
      const int m = mr + 16 * i;
      if (m < M) {
        const float s = sx[m];
        *reinterpret_cast<uint2*>(out + (size_t)m * ldo + nq) =
            make_uint2(pack2bf(acc[i][0] * (s * swv.x), acc[i][1] * (s * swv.y)),
                       pack2bf(acc[i][2] * (s * swv.z), acc[i][3] * (s * swv.w)));
      }
    }
  }
}

struct F8Args {
  const uint8_t* x;
  const float* sx;
  const uint8_t* w;
  const float* sw;
  int M, N, K, split, epi;
  float* part;
  uint16_t* out;
  long long slab;
  int ldo;
  hipStream_t st;
};

template <int BM, int BN>
int f8_launch(const F8Args& a) {
  const int ntiles = (a.N + BN - 1) / BN;
  const dim3 grid(ntiles * a.split);
  const int threads = 64 * F8Shape<BM, BN>::WAVES;
  if (a.epi == F8_PART)
    f8dgemm_kernel<BM, BN, F8_PART><<<grid, threads, 0, a.st>>>(a.x, a.sx, a.w, a.sw, a.M, a.N, a.K, ntiles, a.split,
                                                                a.part, a.out, a.slab, a.ldo);
  else
    f8dgemm_kernel<BM, BN, F8_BF16><<<grid, threads, 0, a.st>>>(a.x, a.sx, a.w, a.sw, a.M, a.N, a.K, ntiles, a.split,
                                                                a.part, a.out, a.slab, a.ldo);
  return CFC_CHECK_LAUNCH();
}

template <int BM>
int f8_rows(const F8Args& a, int bn) {
  switch (bn) {
    case 64: return f8_launch<BM, 64>(a);
    case 96: return f8_launch<BM, 96>(a);
    case 112: return f8_launch<BM, 112>(a);
    case 128: return f8_launch<BM, 128>(a);
    default: return -5;
  }
}

// Row-major W8[N][K] -> Wp[ceil(N / bn)][K / 128][nw = bn / 16][2][64][16 B], rows past N zero.
// One thread per 16-byte piece.
__global__ void f8dgemm_pack_kernel(const uint8_t* __restrict__ W, uint4* __restrict__ Wp, int N, int K, int nw,
                                    size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int l = (int)(i & 63), h = (int)((i >> 6) & 1);
  const size_t frag = i >> 7;
  const int kbs = K / 128;
  const int w = (int)(frag % nw);
  const size_t t2 = frag / nw;
  const int kb = (int)(t2 % kbs), t = (int)(t2 / kbs);
  const int row = 16 * (t * nw + w) + (l & 15);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (row < N) v = *reinterpret_cast<const uint4*>(W + (size_t)row * K + 128 * kb + 64 * h + 16 * (l >> 4));
  Wp[i] = v;
}

}  // namespace

// Y = diag(sx) (X8 . W8^T) diag(sw): x [M, K] e4m3fn row-major, sx [M] fp32, w in the packed layout
// cfc_f8dgemm_pack wrote for this same bn, sw [N] fp32.  1 <= M <= 128, N % 64 == 0, K % 128 == 0,
// bn in {64, 96, 112, 128}, 1 <= split <= K / 128.
//   epi 0: fp32 slabs, part p's row m at part + p * slab + m * ldo (16-byte aligned, ldo % 4 == 0);
//   epi 1 (split 1): bf16 rows at out + m * ldo (8-byte aligned).
// part / out point at the first column of the written range [0, N).  Returns a negative code
// (nothing launched) for anything else.
CFC_API int cfc_f8dgemm(const void* x, const float* sx, const void* w, const float* sw, int M, int N, int K, int split,
                        int epi, int bn, float* part, void* out, long long slab, int ldo, hipStream_t stream) {
  if (M < 1 || M > 128 || N <= 0 || N % 64 || K <= 0 || K % 128 || !x || !sx || !w || !sw) return -1;
  if (split < 1 || split > K / 128) return -3;
  if (epi == F8_PART ? !part : (epi != F8_BF16 || !out || split != 1)) return -2;
  if (ldo < N || ldo % 4 || slab % 4 || slab < 0 || (long long)M * ldo >= (1ll << 29)) return -6;
  if (epi == F8_PART ? ((uintptr_t)part & 15) : ((uintptr_t)out & 7)) return -6;
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)sw & 15) || (long long)bn * K >= (1ll << 31)) return -6;
  const F8Args a{(const uint8_t*)x, sx, (const uint8_t*)w, sw, M, N, K, split, epi, part, (uint16_t*)out, slab, ldo,
                 stream};
  if (M <= 16) return f8_rows<16>(a, bn);
  if (M <= 32) return f8_rows<32>(a, bn);
  if (M <= 64) return f8_rows<64>(a, bn);
  return f8_rows<128>(a, bn);
}

// Row-major e4m3fn W[N][K] -> the packed layout for bn-row workgroups: ceil(N / bn) * bn * K bytes
// at wp, the rows past N zero.  N % 16 == 0, K % 128 == 0, bn in {64, 96, 112, 128}.
CFC_API int cfc_f8dgemm_pack(const void* w, void* wp, int N, int K, int bn, hipStream_t stream) {
  if (N <= 0 || N % 16 || K <= 0 || K % 128 || !w || !wp || w == wp) return -1;
  if (bn != 64 && bn != 96 && bn != 112 && bn != 128) return -5;
  if (((uintptr_t)w & 15) || ((uintptr_t)wp & 15)) return -6;
  const size_t total = (size_t)((N + bn - 1) / bn) * bn * K / 16;
  f8dgemm_pack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>((const uint8_t*)w, (uint4*)wp, N, K,
                                                                          bn / 16, total);
  return CFC_CHECK_LAUNCH();
}
