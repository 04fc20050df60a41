// fp32-operand GEMM for gfx950 — the dense contraction of the fp32 build of the library (libreed_hip_f32.so, -DREED_FP32):
// the reference's `--mixed-precision no` training (image/train.py:505) and `generate.py --no-tf32` sampling
// (image/generate.py:41,183), where every nn.Linear multiplies fp32 operands and accumulates in fp32.
//
//   C[M,N] (+)= sum_k P(m,k) * Q(n,k)        same three operand layouts and the same epilogue ids as csrc/gemm.hip
//
// Matrix instruction: v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate; exact fp32 products, 64 cycles per SIMD = 1/16 of
// the bf16 rate, MI355X_MICROARCH.md "Matrix cores").  The matrix pipe is slow enough that the loop can stay the plain form:
// tile 128x128x16, four waves of 64x64 (2x2 MFMA tiles, 64 accumulator registers), two workgroups per CU, operands staged
// global -> registers -> LDS k-major ([16][128+32] floats per operand: a fragment read is 2 rows x 32 consecutive floats, the
// 32-float pad puts the two rows on disjoint bank halves), double buffered, one barrier per K step, XCD-contiguous tile map.
// Measured (tools/_ab/time_gemm_f32.py): 81-112 TFLOP/s at M = 8192, 112-127 at M = 65536 (71-81 % of the 157 TFLOP/s fp32
// MFMA peak).  (The geometry is a template on the wave grid: a 256x256 tile of SIXTEEN waves, one workgroup of 1024 threads
// per CU, was built for its 64 flop per operand byte and measured 59-120 TFLOP/s — level at M = 65536, 20-40 % slower at
// M = 8192 — so only the 2 x 2 grid is instantiated.)  Every bound
// (ragged M, N, K; split-K ranges) is a guard on the staging loads and on the stores, so there are no shape restrictions
// beyond 4-element alignment.  In this build `bf16` IS float (common.hpp): C, C2, R, bias and the gate are fp32 arrays and
// every rounding point of the mixed-precision epilogues is the identity — one kernel per layout, the epilogue a run-time
// switch.  This file is not part of the 16-bit builds (reed_amd/build.py).
//
// A second kernel template, gemm_f32_split_kernel below, computes the same contraction with every fp32 product taken as three
// bf16 MFMA products (reed_gemm_f32_split(1): the reference's --allow-tf32); its header comment has the arithmetic, the LDS
// layout and the corner cases.  Both share the epilogue, the tile map, the window gather's geometry and the host side.
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <utility>

#include "../../include/reed_hip.h"
#include "gemm_plan.h"

#ifndef REED_FP32
#error "gemm_f32.hip belongs to the fp32-operand build (-DREED_FP32) only"
#endif

namespace {

constexpr int BK = 16;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// Tile geometry for a W x W grid of 64x64 waves: BT rows / columns, NT threads, LDT floats per k-row of an LDS tile (BT + 32
// pad), PP 16-byte pieces per thread, operand and K step.
template <int W>
struct Geo {
  static constexpr int BT = 64 * W, NT = 64 * W * W, LDT = BT + 32, TILE_FLOATS = BK * LDT, PP = BT * 4 / NT;
};

template <int N, class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl<N>(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

template <int PP>
struct Stage {       // one K step of one operand in registers: PP float4 per thread
  f32x4 v[PP];
};

// k-contiguous operand X[rows][K] (ld floats per row): tile rows r0.. x k [k0, k0+16).  Piece p = t + i NT: row p>>2, k (p&3)*4.
template <int W>
__device__ __forceinline__ void load_row(Stage<Geo<W>::PP>& s, const float* X, long ld, int r0, int rows, int k0, int kend, int t) {
#pragma unroll
  for (int i = 0; i < Geo<W>::PP; ++i) {
    const int p = t + i * Geo<W>::NT;
    const int r = r0 + (p >> 2), k = k0 + (p & 3) * 4;
    s.v[i] = (r < rows && k < kend) ? *(const f32x4*)(X + (long)r * ld + k) : f32x4{0.f, 0.f, 0.f, 0.f};   // K % 4 == 0
  }
}
template <int W>
__device__ __forceinline__ void store_row(const Stage<Geo<W>::PP>& s, float* tile, int t) {
#pragma unroll
  for (int i = 0; i < Geo<W>::PP; ++i) {
    const int p = t + i * Geo<W>::NT;
    const int r = p >> 2, kq = (p & 3) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[(kq + e) * Geo<W>::LDT + r] = s.v[i][e];
  }
}
// k-strided operand X[K][cols]: tile k [k0, k0+16) x cols c0..  Piece p = t + i NT: k-row p / (BT/4), columns (p % (BT/4))*4.
template <int W>
__device__ __forceinline__ void load_tr(Stage<Geo<W>::PP>& s, const float* X, long ld, int c0, int cols, int k0, int kend, int t) {
  constexpr int Q = Geo<W>::BT / 4;
#pragma unroll
  for (int i = 0; i < Geo<W>::PP; ++i) {
    const int p = t + i * Geo<W>::NT;
    const int k = k0 + p / Q, c = c0 + (p % Q) * 4;
    s.v[i] = (k < kend && c < cols) ? *(const f32x4*)(X + (long)k * ld + c) : f32x4{0.f, 0.f, 0.f, 0.f};     // cols % 4 == 0
  }
}
template <int W>
__device__ __forceinline__ void store_tr(const Stage<Geo<W>::PP>& s, float* tile, int t) {
  constexpr int Q = Geo<W>::BT / 4;
#pragma unroll
  for (int i = 0; i < Geo<W>::PP; ++i) {
    const int p = t + i * Geo<W>::NT;
    *(f32x4*)(tile + (p / Q) * Geo<W>::LDT + (p % Q) * 4) = s.v[i];
  }
}

__device__ __forceinline__ float act_fwd(int epi, int variant, float x) {
  if (epi == EPI_GELU) return gelu_tanh_f(x);
  if (epi == EPI_SILU) return silu_f(x);
  return variant ? gelu_erf_f(x) : x * sigmoid_f(1.702f * x);   // EPI_QGELU
}

// C > 0 (NT only): P is not a matrix but the 3x3 window gather of an NHWC activation a.P f32 [B, Hi, Wi, C] — row m = output pixel
// (b, y, x) of the [B, Hi << up, Wi << up] grid, column k = tap * C + c = a(b, (y + tap / 3 - 1) >> up, (x + tap % 3 - 1) >> up, c),
// zero outside the grid: the convolutions of the SD-VAE decoder (reed_conv3x3) without an im2col matrix.  down = 1 (up = 0): the
// stride-2 form of the SD-VAE encoder's downsamplers (reed_conv3x3_down), row m = output pixel (b, y, x) of [B, Hi / 2, Wi / 2],
// column k = a(b, 2y + tap / 3, 2x + tap % 3, c), zero at or beyond Hi / Wi.  C == 0: a plain GEMM.
struct ConvGeo {
  int C, Hi, Wi, up, down;
};

// ---- epilogue: lane owns column n (32 consecutive lanes = 32 consecutive columns) of 16 rows per MFMA tile (the C / D layout of
// every 32x32 MFMA: both kernels of this file end here) ----
__device__ __forceinline__ void epilogue_f32(const GemmArgs& a, int epi, const f32x16 (&acc)[2][2], int m0, int n0, int wm, int wn,
                                             int lane, int z) {
  const float* bias = a.bias;
  const float* Rf = (const float*)a.R;
  float* C = (float*)a.C;
  float* C2 = (float*)a.C2;
  // (compile-time indices into the accumulators: with run-time ones — a loop the compiler does not fully unroll around the
  //  epilogue switch — the 64 accumulator registers become a scratch array that is written back after EVERY K step: 16 KiB per
  //  wave and step, four times the operand traffic; that was the first version of this kernel at 35-50 TFLOP/s)
  auto elem = [&](auto I, auto J, auto Rr) {
    constexpr int i = decltype(I)::value, j = decltype(J)::value, r = decltype(Rr)::value;
    const int n = n0 + wn * 64 + j * 32 + (lane & 31);
    const int m = m0 + wm * 64 + i * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
    if (n >= a.N || m >= a.M) return;
    const float v = acc[i][j][r] + (bias ? bias[n] : 0.f);
    switch (epi) {
      case EPI_BF16: C[(long)m * a.ldc + n] = v; break;
      case EPI_GELU: case EPI_SILU: case EPI_QGELU:
        if (C) C[(long)m * a.ldc + n] = v;
        C2[(long)m * a.ldc2 + n] = act_fwd(epi, a.act_variant, v);
        break;
      case EPI_GATE_RES: {
        if (C2) C2[(long)m * a.ldc2 + n] = v;
        const float g = a.gate[(long)(m / a.rows_per_gate) * a.ldgate + n];
        C[(long)m * a.ldc + n] = Rf[(long)m * a.ldr + n] + g * v;
      } break;
      case EPI_LS_RES: C[(long)m * a.ldc + n] = Rf[(long)m * a.ldr + n] + a.gate[n] * v; break;
      case EPI_GELU_G: case EPI_SILU_G: {   // C carries the activation's derivative (fp32 here: no rounding), gemm.h
        float av, gv;
        if (epi == EPI_GELU_G) gelu_tanh_both(v, av, gv);
        else silu_both(v, av, gv);
        if (C) C[(long)m * a.ldc + n] = gv;
        C2[(long)m * a.ldc2 + n] = av;
      } break;
      case EPI_MUL: C[(long)m * a.ldc + n] = v * Rf[(long)m * a.ldr + n]; break;
      case EPI_DGELU: C[(long)m * a.ldc + n] = v * gelu_tanh_grad_f(Rf[(long)m * a.ldr + n]); break;
      case EPI_DSILU: C[(long)m * a.ldc + n] = v * silu_grad_f(Rf[(long)m * a.ldr + n]); break;
      case EPI_RES_BF16: C[(long)m * a.ldc + n] = v + Rf[(long)m * a.ldr + n]; break;
      case EPI_F32: {
        float* cp = C + (long)z * a.slab_stride + (long)m * a.ldc + n;
        *cp = a.accumulate ? *cp + v : v;
      } break;
      case EPI_ADDF32_RB: C[(long)m * a.ldc + n] += v; break;
      case EPI_ATOMIC_F32: atomicAdd(C + (long)m * a.ldc + n, v); break;
    }
  };
  static_for<2>([&](auto I) { static_for<2>([&](auto J) { static_for<16>([&](auto Rr) { elem(I, J, Rr); }); }); });
}

// block -> tile: XCD-contiguous runs (consecutive workgroup ids alternate over the 8 XCDs), grouped along M: the tiles an
// XCD works on at a time share operand panels in its L2
__device__ __forceinline__ void tile_of_block(int bid, int ntm, int ntn, int& tm, int& tn) {
  const int nwg = ntm * ntn;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  constexpr int GM = 8;
  const int per_group = GM * ntn;
  const int group = bid / per_group, first_m = group * GM;
  const int gs = min(ntm - first_m, GM);
  tm = first_m + (bid % per_group) % gs;
  tn = (bid % per_group) / gs;
}

template <int LAY, int W>
__global__ __launch_bounds__(64 * W * W, W == 2 ? 2 : 1) void gemm_f32_kernel(GemmArgs a, int epi, ConvGeo cg) {
  constexpr int BM = Geo<W>::BT, BN = Geo<W>::BT, LDT = Geo<W>::LDT, TILE_FLOATS = Geo<W>::TILE_FLOATS;
  extern __shared__ __attribute__((aligned(16))) float smem_f32[];        // [buffer][P | Q][TILE_FLOATS]
  float (*smem)[2][TILE_FLOATS] = (float (*)[2][TILE_FLOATS])smem_f32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / W, wn = wave % W;
  int tm, tn;
  tile_of_block(blockIdx.x, (a.M + BM - 1) / BM, (a.N + BN - 1) / BN, tm, tn);
  const int z = blockIdx.y;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = z * a.ksplit_len;
  const int kend = min(a.K, kbeg + a.ksplit_len);
  const int nt = (kend - kbeg + BK - 1) / BK;

  typedef Stage<Geo<W>::PP> stage_t;
  // window gather: the output pixel of each of this thread's row pieces, decomposed once
  int cy[Geo<W>::PP], cx[Geo<W>::PP], cb[Geo<W>::PP];
  if (LAY == LAY_NT && cg.C > 0) {
    const int Ho = cg.down ? cg.Hi >> 1 : cg.Hi << cg.up, Wo = cg.down ? cg.Wi >> 1 : cg.Wi << cg.up;
#pragma unroll
    for (int i = 0; i < Geo<W>::PP; ++i) {
      const int m = m0 + ((tid + i * Geo<W>::NT) >> 2);
      const int b = m / (Ho * Wo), rem = m - b * (Ho * Wo);
      cy[i] = (m < a.M ? rem / Wo : -4) * (1 + cg.down);   // a row beyond M: every tap lands outside
      cx[i] = (rem - (rem / Wo) * Wo) * (1 + cg.down);
      cb[i] = b * cg.Hi * cg.Wi;
    }
  }
  auto load = [&](int t, stage_t& sp, stage_t& sq) {
    const int k0 = kbeg + t * BK;
    if constexpr (LAY == LAY_TN) load_tr<W>(sp, a.P, a.ldp, m0, a.M, k0, kend, tid);
    else if (LAY == LAY_NT && cg.C > 0) {
      const int Hg = cg.Hi << cg.up, Wg = cg.Wi << cg.up, pad = 1 - cg.down;   // the grid the taps index, its top / left pad
#pragma unroll
      for (int i = 0; i < Geo<W>::PP; ++i) {
        const int k = k0 + ((tid + i * Geo<W>::NT) & 3) * 4;
        const int tap = k / cg.C, c = k - tap * cg.C;
        const int yy = cy[i] + tap / 3 - pad, xx = cx[i] + (tap - (tap / 3) * 3) - pad;
        const bool in = k < kend && (unsigned)yy < (unsigned)Hg && (unsigned)xx < (unsigned)Wg;
        sp.v[i] = in ? *(const f32x4*)(a.P + ((long)(cb[i] + (yy >> cg.up) * cg.Wi + (xx >> cg.up)) * cg.C + c))
                     : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else load_row<W>(sp, a.P, a.ldp, m0, a.M, k0, kend, tid);
    if constexpr (LAY == LAY_NT) load_row<W>(sq, a.Q, a.ldq, n0, a.N, k0, kend, tid);
    else load_tr<W>(sq, a.Q, a.ldq, n0, a.N, k0, kend, tid);
  };
  auto store = [&](int buf, const stage_t& sp, const stage_t& sq) {
    if constexpr (LAY == LAY_TN) store_tr<W>(sp, smem[buf][0], tid);
    else store_row<W>(sp, smem[buf][0], tid);
    if constexpr (LAY == LAY_NT) store_row<W>(sq, smem[buf][1], tid);
    else store_tr<W>(sq, smem[buf][1], tid);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // TN: the bias gradient dbias[m] = sum_k P[k][m] (column sums of dY) rides along in the blocks of the first column tile:
  // thread t < 128 owns column m0 + t of the staged P tile
  const bool do_dbias = (LAY == LAY_TN) && a.dbias != nullptr && tn == 0;
  float bsum = 0.f;

  stage_t sp, sq;
  if (nt > 0) {
    load(0, sp, sq);
    store(0, sp, sq);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load(t + 1, sp, sq);
    const float* tp = smem[buf][0];
    const float* tq = smem[buf][1];
    const int kr = lane >> 5, c = lane & 31;
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks) {
      float pf[2], qf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        pf[i] = tp[(2 * ks + kr) * LDT + wm * 64 + i * 32 + c];
        qf[i] = tq[(2 * ks + kr) * LDT + wn * 64 + i * 32 + c];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf[i], qf[j], acc[i][j], 0, 0, 0);
    }
    if (do_dbias && tid < BM) {
#pragma unroll
      for (int k = 0; k < BK; ++k) bsum += tp[k * LDT + tid];
    }
    if (t + 1 < nt) store(buf ^ 1, sp, sq);
    __syncthreads();
  }

  epilogue_f32(a, epi, acc, m0, n0, wm, wn, lane, z);
  if (do_dbias && tid < BM) {
    const int m = m0 + tid;
    if (m < a.M) {
      if (gridDim.y > 1) a.dbias[(long)z * a.slab_stride + m] = bsum;   // split-K: per-slice slab (C's stride)
      else if (a.accumulate) a.dbias[m] += bsum;
      else a.dbias[m] = bsum;
    }
  }
}

// ---- the split kernel (reed_gemm_f32_split(1)) ------------------------------------------------------------------------------
// The same contraction on the bf16 matrix instruction: gfx950 has no xf32 MFMA, so the reference's --allow-tf32 (fp32 operands
// in memory, a short mantissa in the multiplier, fp32 accumulation) is computed as THREE bf16 products.  Every operand element x
// is split in registers, between the global load and the LDS store, into
//     hi = bf16_rne(x),   lo = bf16_rne(x - float(hi))          (the subtraction is exact in fp32)
// and a*b is taken as a_hi*b_lo + a_lo*b_hi + a_hi*b_hi, all three accumulated in fp32 into the same accumulators by
// v_mfma_f32_32x32x16_bf16.  The dropped terms (a_lo*b_lo and the rounding of lo) bound the error of one product by 3 * 2^-16 of
// |a||b| (TF32's own rounding: 2 * 2^-11) at fp32's exponent range; the matrix work per K is 3/16 of the fp32 instruction's.
//
// Same contract as gemm_f32_kernel: the same GemmArgs, layouts, epilogue (epilogue_f32: the 32x32 C / D layout is the same),
// TN bias gradient, split-K, window gather, tile map, shape rules and guards.  Tile 128x128x32, four waves of 64x64 (2x2 MFMA
// tiles), double buffered, 64 KiB of LDS (two workgroups per CU): per buffer and operand a `hi` and a `lo` tile of [128 rows][32 k]
// bf16 — together the bytes of the fp32 tile they replace.  A row is 64 bytes = four 16-byte chunks of 8 k, one chunk = one lane's
// fragment of the MFMA (lane l: row l & 31, k = 8 (l >> 5) ..+8); chunk c of row r is stored at chunk c ^ ((r >> 2) & 3), which
// makes the ds_read_b128 of a fragment conflict-free in each of the instruction's 16-lane groups (MI355X: rows {0-3, 12-15, 20-27}
// and {4-11, 16-19, 28-31}).  A k-contiguous operand (P of NT / NN, Q of NT, the window gather) loads two float4 = 8 consecutive
// k of one row per piece and stores one 16-byte chunk per half; a k-strided operand (Q of NN, both of TN) loads the same four
// columns of four consecutive k-rows and repacks in registers: per column one 8-byte store of 4 k per half (no transposing LDS
// read).  A float4 that lies beyond K, the split-K range or the matrix is loaded as zeros, whose hi AND lo are zero: K % 8 == 4
// and a K range that ends inside a chunk need no special case.  The TN bias gradient is summed from the fp32 registers of the
// staged P (not from the bf16 tiles): plain fp32 column sums, as in gemm_f32_kernel, in another order.
//
// Corner cases: an operand with |x| > 3.3895e38 rounds to hi = +-inf, and so does an infinite operand; lo = x - hi is then -+inf
// or NaN and the output row / column it feeds is NaN where the fp32 kernel gives +-inf (finite fp32 of ordinary range are unaffected;
// a NaN operand gives NaN in both).  lo is a bf16 subnormal when |x - hi| < 2^-126, i.e. for |x| below about 2^-118; whether the
// bf16 MFMA reads subnormal operands as they are or as zero is not documented and NOT MEASURED here — the tests keep subnormals
// out of their inputs, and the error budget (tests/tf32_ref.py) does not cover operands that small.
typedef __attribute__((ext_vector_type(8))) __bf16 hbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 hbf16x4;
constexpr int SBK = 32;                       // K step
constexpr int SHALF = 128 * SBK;              // bf16 elements of one hi or lo tile (8 KiB)
constexpr int SPLIT_LDS = 2 * 2 * 2 * SHALF * 2;   // [buffer][P | Q][hi | lo] = 64 KiB

struct SplitStage {   // one K step of one operand in registers: four float4 per thread
  f32x4 v[4];
};

__device__ __forceinline__ void split4(const f32x4 x, hbf16x4& hi, hbf16x4& lo) {
  hi = __builtin_convertvector(x, hbf16x4);
  lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x4), hbf16x4);
}

// k-contiguous operand: piece g = t + 256 i (i < 2) is chunk g & 3 of row g >> 2: float4 v[2 i] = k c*8 ..+4, v[2 i + 1] = k c*8+4 ..+4
__device__ __forceinline__ void split_load_row(SplitStage& s, const float* X, long ld, int r0, int rows, int k0, int kend, int t) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int g = t + (q >> 1) * 256;
    const int r = r0 + (g >> 2), k = k0 + (g & 3) * 8 + (q & 1) * 4;
    s.v[q] = (r < rows && k < kend) ? *(const f32x4*)(X + (long)r * ld + k) : f32x4{0.f, 0.f, 0.f, 0.f};   // K % 4 == 0
  }
}
__device__ __forceinline__ void split_store_row(const SplitStage& s, __bf16* tile, int t) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int g = t + i * 256;
    const int r = g >> 2, c = (g & 3) ^ ((r >> 2) & 3);
    hbf16x4 h0, l0, h1, l1;
    split4(s.v[2 * i], h0, l0);
    split4(s.v[2 * i + 1], h1, l1);
    *(hbf16x8*)(tile + r * SBK + c * 8) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    *(hbf16x8*)(tile + SHALF + r * SBK + c * 8) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}
// k-strided operand X[K][cols]: thread t (wave w = t >> 6, lane l) owns columns (l >> 1) * 4 ..+4 of the four k-rows
// (2 w + (l & 1)) * 4 ..+4: v[kk] = one k-row (32 lanes of a load = 512 contiguous bytes)
__device__ __forceinline__ void split_load_tr(SplitStage& s, const float* X, long ld, int c0, int cols, int k0, int kend, int t) {
  const int c = c0 + ((t & 63) >> 1) * 4, kb = k0 + ((t >> 6) * 2 + (t & 1)) * 4;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    s.v[kk] = (kb + kk < kend && c < cols) ? *(const f32x4*)(X + (long)(kb + kk) * ld + c) : f32x4{0.f, 0.f, 0.f, 0.f};   // cols % 4 == 0
}
__device__ __forceinline__ void split_store_tr(const SplitStage& s, __bf16* tile, int t) {
  const int cgrp = (t & 63) >> 1;
  const int off = ((t >> 6) ^ (cgrp & 3)) * 8 + (t & 1) * 4;   // rows 4 cgrp + j: (row >> 2) & 3 = cgrp & 3
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hbf16x4 hi, lo;
    split4(f32x4{s.v[0][j], s.v[1][j], s.v[2][j], s.v[3][j]}, hi, lo);
    *(hbf16x4*)(tile + (cgrp * 4 + j) * SBK + off) = hi;
    *(hbf16x4*)(tile + SHALF + (cgrp * 4 + j) * SBK + off) = lo;
  }
}

template <int LAY>
__global__ __launch_bounds__(256, 2) void gemm_f32_split_kernel(GemmArgs a, int epi, ConvGeo cg) {
  constexpr int BM = 128, BN = 128;
  extern __shared__ __attribute__((aligned(16))) float smem_f32[];        // [buffer][P | Q][hi | lo][SHALF] bf16
  __bf16 (*smem)[2][2 * SHALF] = (__bf16 (*)[2][2 * SHALF])smem_f32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn;
  tile_of_block(blockIdx.x, (a.M + BM - 1) / BM, (a.N + BN - 1) / BN, tm, tn);
  const int z = blockIdx.y;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = z * a.ksplit_len;
  const int kend = min(a.K, kbeg + a.ksplit_len);
  const int nt = (kend - kbeg + SBK - 1) / SBK;

  // window gather: the output pixel of each of this thread's two rows, decomposed once
  int cy[2], cx[2], cb[2];
  if (LAY == LAY_NT && cg.C > 0) {
    const int Ho = cg.down ? cg.Hi >> 1 : cg.Hi << cg.up, Wo = cg.down ? cg.Wi >> 1 : cg.Wi << cg.up;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + ((tid + i * 256) >> 2);
      const int b = m / (Ho * Wo), rem = m - b * (Ho * Wo);
      cy[i] = (m < a.M ? rem / Wo : -4) * (1 + cg.down);   // a row beyond M: every tap lands outside
      cx[i] = (rem - (rem / Wo) * Wo) * (1 + cg.down);
      cb[i] = b * cg.Hi * cg.Wi;
    }
  }
  auto load = [&](int t, SplitStage& sp, SplitStage& sq) {
    const int k0 = kbeg + t * SBK;
    if constexpr (LAY == LAY_TN) split_load_tr(sp, a.P, a.ldp, m0, a.M, k0, kend, tid);
    else if (LAY == LAY_NT && cg.C > 0) {
      const int Hg = cg.Hi << cg.up, Wg = cg.Wi << cg.up, pad = 1 - cg.down;   // the grid the taps index, its top / left pad
#pragma unroll
      for (int q = 0; q < 4; ++q) {   // per float4: C % 4 == 0, so the two halves of a chunk may lie in different taps
        const int k = k0 + (tid & 3) * 8 + (q & 1) * 4;
        const int tap = k / cg.C, c = k - tap * cg.C;
        const int yy = cy[q >> 1] + tap / 3 - pad, xx = cx[q >> 1] + (tap - (tap / 3) * 3) - pad;
        const bool in = k < kend && (unsigned)yy < (unsigned)Hg && (unsigned)xx < (unsigned)Wg;
        sp.v[q] = in ? *(const f32x4*)(a.P + ((long)(cb[q >> 1] + (yy >> cg.up) * cg.Wi + (xx >> cg.up)) * cg.C + c))
                     : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else split_load_row(sp, a.P, a.ldp, m0, a.M, k0, kend, tid);
    if constexpr (LAY == LAY_NT) split_load_row(sq, a.Q, a.ldq, n0, a.N, k0, kend, tid);
    else split_load_tr(sq, a.Q, a.ldq, n0, a.N, k0, kend, tid);
  };
  // TN: the bias gradient dbias[m] = sum_k P[k][m] rides along in the blocks of the first column tile, summed from the fp32
  // registers on their way to LDS: this thread's four columns of its four k-rows per step
  const bool do_dbias = (LAY == LAY_TN) && a.dbias != nullptr && tn == 0;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  auto store = [&](int buf, const SplitStage& sp, const SplitStage& sq) {
    if constexpr (LAY == LAY_TN) {
      split_store_tr(sp, smem[buf][0], tid);
      if (do_dbias) bsum += (sp.v[0] + sp.v[1]) + (sp.v[2] + sp.v[3]);
    } else split_store_row(sp, smem[buf][0], tid);
    if constexpr (LAY == LAY_NT) split_store_row(sq, smem[buf][1], tid);
    else split_store_tr(sq, smem[buf][1], tid);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  SplitStage sp, sq;
  if (nt > 0) {
    load(0, sp, sq);
    store(0, sp, sq);
  }
  __syncthreads();
  // fragment of lane l: row l & 31 of its 32-row tile, chunk 2 ks + (l >> 5), swizzled by (row >> 2) & 3 = (l >> 2) & 3
  const int frow = (lane & 31) * SBK, fsw = (lane >> 2) & 3, fh = lane >> 5;
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load(t + 1, sp, sq);
    const __bf16* tp = smem[buf][0] + wm * 64 * SBK + frow;
    const __bf16* tq = smem[buf][1] + wn * 64 * SBK + frow;
#pragma unroll
    for (int ks = 0; ks < SBK / 16; ++ks) {
      const int co = ((2 * ks + fh) ^ fsw) * 8;
      hbf16x8 ph[2], pl[2], qh[2], ql[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ph[i] = *(const hbf16x8*)(tp + i * 32 * SBK + co);
        pl[i] = *(const hbf16x8*)(tp + SHALF + i * 32 * SBK + co);
        qh[i] = *(const hbf16x8*)(tq + i * 32 * SBK + co);
        ql[i] = *(const hbf16x8*)(tq + SHALF + i * 32 * SBK + co);
      }
      // the two cross products, then the main one, into the same accumulators
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph[i], ql[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pl[i], qh[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph[i], qh[j], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < nt) store(buf ^ 1, sp, sq);
    __syncthreads();
  }

  epilogue_f32(a, epi, acc, m0, n0, wm, wn, lane, z);
  if (do_dbias) {   // (block-uniform) the eight k-row groups' partial sums of each column meet in LDS, free after the last barrier
    float* red = smem_f32;   // [8 k-row groups][128 columns]
    *(f32x4*)(red + ((tid >> 6) * 2 + (tid & 1)) * BM + (lane >> 1) * 4) = bsum;
    __syncthreads();
    const int m = m0 + tid;
    if (tid < BM && m < a.M) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) s += red[g * BM + tid];
      if (gridDim.y > 1) a.dbias[(long)z * a.slab_stride + m] = s;   // split-K: per-slice slab (C's stride)
      else if (a.accumulate) a.dbias[m] += s;
      else a.dbias[m] = s;
    }
  }
}

template <int LAY, int W>
int launch_w(const GemmArgs& a, int epi, int splits, hipStream_t stream, ConvGeo cg) {
  constexpr int lds = 2 * 2 * Geo<W>::TILE_FLOATS * (int)sizeof(float);
  static bool reserved = false;
  if (const int rc = reed_reserve_lds(reserved, (const void*)gemm_f32_kernel<LAY, W>, lds, "gemm_f32")) return rc;
  dim3 grid(cdiv(a.M, Geo<W>::BT) * cdiv(a.N, Geo<W>::BT), splits, 1);
  REED_KLAUNCH((gemm_f32_kernel<LAY, W>), grid, dim3(Geo<W>::NT), lds, stream, a, epi, cg);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

template <int LAY>
int launch_split(const GemmArgs& a, int epi, int splits, hipStream_t stream, ConvGeo cg) {
  static bool reserved = false;
  if (const int rc = reed_reserve_lds(reserved, (const void*)gemm_f32_split_kernel<LAY>, SPLIT_LDS, "gemm_f32 (split)")) return rc;
  dim3 grid(cdiv(a.M, 128) * cdiv(a.N, 128), splits, 1);
  REED_KLAUNCH((gemm_f32_split_kernel<LAY>), grid, dim3(256), SPLIT_LDS, stream, a, epi, cg);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

// reed_gemm_f32_split (gemm_plan.cpp) selects between the two kernels, for reed_gemm and for the convolutions alike
template <int LAY>
int launch(const GemmArgs& a, int epi, int splits, hipStream_t stream, ConvGeo cg = ConvGeo{0, 0, 0, 0, 0}) {
  if (reed_gemm_f32_split_on()) return launch_split<LAY>(a, epi, splits, stream, cg);
  return launch_w<LAY, 2>(a, epi, splits, stream, cg);
}

}  // namespace

// (the tile-selection knobs of the 16-bit kernels — gemm_plan.cpp — are accepted and without effect here: one tile; the one
// knob this build reads is reed_gemm_f32_split)

// The grouped weight-gradient launch is a 16-bit MFMA kernel (gemm_tn.hip): not part of this build; the caller falls back to
// one reed_gemm(TN) per weight (ops.wgrad_group returns False on this code).
int reed_gemm_tn_group_launch(int, const GemmArgs*, hipStream_t) {
  reed_set_error("reed_wgrad_group: not built for fp32 operands (one reed_gemm(TN) per weight instead)");
  return REED_ERR_UNSUPPORTED;
}

extern "C" int reed_wgrad_group_deal(int, const int*, const int*, const int*, int, unsigned*) { return 0; }   // (16-bit builds only)

// 3x3 convolution, padding 1, optional nearest x2 upsampling of the input, as an implicit GEMM on the fp32 MFMA kernel above (the
// 16-bit builds have their own: conv.hip): out f32 [B*Ho*Wo, ldc] (+)= conv(a f32 NHWC [B, Hi, Wi, C]; w f32 [N, 9 C]) + bias.
static int conv3x3_f32(const char* what, const void* act, const void* w, const float* bias, float* out, int64_t ldc, int B, int Hi,
                       int Wi, int C, int N, int upsample, int down, int accumulate, void* stream) {
  REED_CHECK_ARG(act && w && out && B > 0 && Hi > down && Wi > down && C > 0 && N > 0, "%s: empty problem", what);
  REED_CHECK_ARG(upsample == 0 || upsample == 1, "%s: upsample must be 0 or 1 (nearest x2)", what);
  REED_CHECK_ARG(C % 4 == 0 && N % 4 == 0 && ldc >= N, "%s(fp32): C=%d and N=%d must be multiples of 4, ldc >= N", what, C, N);
  const long M = down ? (long)B * (Hi >> 1) * (Wi >> 1) : (long)B * (Hi << upsample) * (Wi << upsample);
  REED_CHECK_ARG(M < (1l << 31) - 256 && (long)B * Hi * Wi < (1l << 31), "%s: too many positions for one call", what);
  REED_CHECK_ARG(((uintptr_t)act % 16) == 0 && ((uintptr_t)w % 16) == 0 && (!bias || (uintptr_t)bias % 16 == 0),
                 "%s: operands must be 16-byte aligned", what);
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.P = (const float*)act;
  a.Q = (const float*)w;
  a.ldp = 9 * C;
  a.ldq = 9 * C;
  a.M = (int)M;
  a.N = N;
  a.K = 9 * C;
  a.C = out;
  a.ldc = ldc;
  a.bias = bias;
  a.accumulate = accumulate;
  a.rows_per_gate = 1;
  a.ksplit_len = a.K;
  return launch<LAY_NT>(a, EPI_F32, 1, (hipStream_t)stream, ConvGeo{C, Hi, Wi, upsample, down});
}

extern "C" int reed_conv3x3(const void* act, const void* w, const float* bias, float* out, int64_t ldc, int B, int Hi, int Wi, int C,
                            int N, int upsample, int accumulate, void* stream) {
  return conv3x3_f32("reed_conv3x3", act, w, bias, out, ldc, B, Hi, Wi, C, N, upsample, 0, accumulate, stream);
}

// the stride-2 form with diffusers' (0, 1, 0, 1) padding (the SD-VAE encoder's downsamplers): out [B * (Hi / 2) * (Wi / 2), ldc]
extern "C" int reed_conv3x3_down(const void* act, const void* w, const float* bias, float* out, int64_t ldc, int B, int Hi, int Wi,
                                 int C, int N, int accumulate, void* stream) {
  REED_CHECK_ARG(Hi > 1 && Wi > 1, "reed_conv3x3_down: Hi=%d, Wi=%d must be at least 2", Hi, Wi);
  return conv3x3_f32("reed_conv3x3_down", act, w, bias, out, ldc, B, Hi, Wi, C, N, 0, 1, accumulate, stream);
}

// The shape rules of the one kernel, and its split-K arithmetic: the same as the 16-bit kernels' (units of 64), so callers that size
// slab workspaces by it (ops.linear_wgrad, engine.py) see the same slab count from either build.
static int plan_f32(int& layout, int epi, int M, int N, int K, int& splits, bool has_slab, int* ksplit_len) {
  REED_CHECK_ARG(M > 0 && N > 0 && K > 0, "reed_gemm: empty problem M=%d N=%d K=%d", M, N, K);
  REED_CHECK_ARG(N % 4 == 0, "reed_gemm(fp32): leading dims and N must be multiples of 4 elements");
  if (layout == LAY_TN_TALL || layout == LAY_TN_WIDE) layout = LAY_TN;   // tile hints of the 16-bit weight-gradient kernel
  if (layout == LAY_TN) REED_CHECK_ARG(M % 4 == 0, "reed_gemm(TN, fp32): M=%d must be a multiple of 4", M);
  else REED_CHECK_ARG(K % 4 == 0, "reed_gemm(NT/NN, fp32): K=%d must be a multiple of 4", K);
  REED_CHECK_ARG(epi_in(EPIS_F32, epi), "reed_gemm: unknown epilogue %d", epi);
  if (splits < 1) splits = 1;
  const int ksteps = cdiv(K, 64);
  const int per = cdiv(ksteps, splits);
  splits = cdiv(ksteps, per);
  *ksplit_len = per * 64;
  if (splits > 1)
    REED_CHECK_ARG(epi == EPI_ATOMIC_F32 || (epi == EPI_F32 && has_slab), "reed_gemm: split-K needs the atomic or slab fp32 epilogue");
  REED_CHECK_ARG(layout == LAY_NT || layout == LAY_NN || layout == LAY_TN, "reed_gemm: unknown layout %d", layout);
  return REED_OK;
}

// the dry run of include/reed_hip.h: one kernel, whatever the tile knobs say — the exact one, or the split one while
// reed_gemm_f32_split(1) holds
extern "C" int reed_gemm_plan(int layout, int epilogue, int M, int N, int K, int split_k, int flags, int, int, int, int, int, int,
                              int* launches) {
  int ksplit_len = 0;
  if (epilogue == EPI_GELU_ERF) epilogue = EPI_QGELU;   // (as reed_gemm: the variant is a run-time switch of this build)
  if (!epi_layout_ok(layout, epilogue, N, split_k) || epilogue == EPI_SWIGLU) {
    reed_set_error("reed_gemm: epilogue %d: NT only, no split-K (17: not part of the fp32-operand build)", epilogue);
    return -REED_ERR_ARG;
  }
  if (const int rc = plan_f32(layout, epilogue, M, N, K, split_k, (flags & 2) != 0, &ksplit_len)) return -rc;
  // (both kernels work on 128 x 128 tiles: the mode changes the kernel id, not the grid)
  const int v[GEMM_LAUNCH_INTS] = {reed_gemm_f32_split_on() ? GK_F32_SPLIT : GK_F32, 0, M, 0, N, split_k, ksplit_len, 0,
                                   cdiv(M, 128) * cdiv(N, 128)};
  if (launches) memcpy(launches, v, sizeof(v));
  return 1;
}

int reed_gemm_launch(int layout, int epi, GemmArgs a, int splits, hipStream_t stream) {
  REED_CHECK_ARG(a.ldp % 4 == 0 && a.ldq % 4 == 0, "reed_gemm(fp32): leading dims and N must be multiples of 4 elements");
  REED_CHECK_ARG(((uintptr_t)a.P % 16) == 0 && ((uintptr_t)a.Q % 16) == 0, "reed_gemm: operands must be 16-byte aligned");
  if (const int rc = plan_f32(layout, epi, a.M, a.N, a.K, splits, a.slab_stride > 0, &a.ksplit_len)) return rc;
  switch (layout) {
    case LAY_NT: return launch<LAY_NT>(a, epi, splits, stream);
    case LAY_NN: return launch<LAY_NN>(a, epi, splits, stream);
  }
  return launch<LAY_TN>(a, epi, splits, stream);
}
