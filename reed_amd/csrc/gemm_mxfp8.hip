// MX-fp8 block GEMM for gfx950 (the sampling path's opt-in 8-bit mode) and the quantiser that feeds it.
//
// Format (OCP MX, fixed in DESIGN.md §3.1): elements e4m3fn (bias 7, max 448, NaN 0x7F / 0xFF, no infinities), blocks of 32
// consecutive k with one E8M0 scale byte (value 2^(byte - 127)).  For a finite block with amax > 0:
//   X = clamp(floor(log2 amax) - 8, -127, 127), byte = X + 127, code_i = sat448(rne_e4m3(x_i 2^-X)).
// amax = 0: byte 127, signed-zero codes.  A block with an inf or a NaN: byte 0xFF and every code 0x7F, so every output that
// consumes the block is NaN whichever of the two the matrix pipe looks at.
//
//   C[M,N] = epi( sum_blocks 2^(Xa + Xw) sum_{k in block} a w  [+ bias] )      NT: Aq [M,K], Wq [N,K], both k-contiguous
//
// on v_mfma_scale_f32_16x16x128_f8f6f4.  Its operand map, measured with tools/micro/mx_mfma_probe.hip (profiles/mxfp8_sampling.txt)
// and held by the exact-integer probe of tests/test_mxfp8_gemm_gpu.py: lane (i = lane & 15, g = lane >> 4) holds, of row i of its
// operand, k = 16 g .. 16 g + 15 in registers 0-3 and k = 64 + 16 g .. 64 + 16 g + 15 in registers 4-7 — two 16x16x64 halves — while
// the scale of block b (k = 32 b .. 32 b + 31) of row i is read from the op_sel'th byte of the scale register of lane i + 16 b:
// a lane's scale does NOT belong to the lane's own 32 codes.
//
// Structure = gemm.hip's: 128 x 128 output tile, 4 waves (2 x 2) of 4 x 4 MFMA tiles, one 128-BYTE K step (128 codes: the
// same [128][128 B] swizzled LDS tiles as the bf16 kernel's 64-element step, LDS-DMA staging with the hardware range check,
// two buffers, one barrier per step), the MFMA issued "swapped" (W as the A operand) so that tile_epilogue applies unchanged.
// The scale bytes (4 per row and K step = one dword) come straight from global memory a step ahead.
#include "gemm_common.hpp"
#include "../../include/reed_hip.h"

namespace {
using namespace gemm_detail;

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------------------
// quantiser: four lanes per block of 32 (8 elements = 16 B in, 8 B out per lane), amax over the quad
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned e4m3_code(float v) {   // |v| finite; RNE onto the e4m3 grid, saturating at 448
  const unsigned b = __builtin_bit_cast(unsigned, v);
  const unsigned sign = (b >> 24) & 0x80u;
  float a = __builtin_bit_cast(float, b & 0x7FFFFFFFu);
  a = fminf(a, 448.f);
  unsigned code;
  if (a < 0.015625f) {   // below 2^-6: the subnormal grid, multiples of 2^-9 (8 = the smallest normal's code)
    code = (unsigned)__builtin_rintf(a * 512.f);
  } else {
    unsigned r = __builtin_bit_cast(unsigned, a);
    r += 0x7FFFFu + ((r >> 20) & 1u);
    code = (((r >> 23) - 120u) << 3) | ((r >> 20) & 7u);
  }
  return sign | code;
}

__global__ __launch_bounds__(256) void mx_quantize_kernel(const bf16* __restrict__ x, long ldx, unsigned char* __restrict__ q,
                                                          long ldq, unsigned char* __restrict__ s, long lds, int R, int K) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int cpr = K >> 3;                 // 8-element chunks per row
  const long row = t / cpr;
  const int ch = (int)(t - row * cpr);
  const bool live = row < R;              // (whole quads are live or dead together: cpr is a multiple of 4)
  bf16x8 v = bf16x8{};
  if (live) v = *(const bf16x8*)(x + row * ldx + ch * 8);
  float f[8];
  unsigned am = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = bf2f(v[e]);
    const unsigned ab = __builtin_bit_cast(unsigned, f[e]) & 0x7FFFFFFFu;   // integer order = magnitude order, NaN above inf
    am = ab > am ? ab : am;
  }
  unsigned o = (unsigned)__shfl_xor((int)am, 1);
  am = o > am ? o : am;
  o = (unsigned)__shfl_xor((int)am, 2);
  am = o > am ? o : am;
  unsigned sb, lo = 0, hi = 0;
  if (am >= 0x7F800000u) {
    sb = 0xFFu;
    lo = hi = 0x7F7F7F7Fu;
  } else {
    int X = (int)(am >> 23) - 127 - 8;
    X = am == 0 ? 0 : (X < -127 ? -127 : X);
    sb = (unsigned)(X + 127);
    const float inv = __builtin_bit_cast(float, (unsigned)(127 - X) << 23);   // 2^-X: X in [-127, 119]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= e4m3_code(f[e] * inv) << (8 * e);
      hi |= e4m3_code(f[e + 4] * inv) << (8 * e);
    }
  }
  if (live) {
    *(u32x2*)(q + row * ldq + ch * 8) = u32x2{lo, hi};
    if ((ch & 3) == 0) s[row * lds + (ch >> 2)] = (unsigned char)sb;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int BM = 128, BN = 128, BKB = 128;   // K step in codes = bytes
constexpr int TILE_BYTES = 16384;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;

struct MxOperands {
  const unsigned char *A, *As, *W, *Ws;
  long lda, ldas, ldw, ldws;
};

// rows [0,128) x bytes [k0, k0 + 128) of a k-contiguous code matrix; rsrc based at the tile's first row (gemm.hip: stage_row)
__device__ __forceinline__ void stage_codes(__amdgpu_buffer_rsrc_t rs, char* tile, long ld, int k0, int tid, int wave) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int L = i * 256 + tid;
    const int r = L >> 3, cp = L & 7;
    const int c = cp ^ ((r >> 1) & 7);
    const int voff = (int)((long)r * ld + k0 + c * 16);
    char* dst = tile + (i * 256 + wave * 64) * 16;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, voff, 0, 0, 0);
  }
}
// lane (i, g): the codes k = 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15 of row rowbase + i (the instruction's map, above)
__device__ __forceinline__ i32x8 frag_codes(const char* tile, int rowbase, int lane) {
  const int row = rowbase + (lane & 15), g = lane >> 4, sw = (row >> 1) & 7;
  const i32x4 lo = *(const i32x4*)(tile + row * 128 + ((g ^ sw) << 4));
  const i32x4 hi = *(const i32x4*)(tile + row * 128 + (((g + 4) ^ sw) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_mxfp8_kernel(GemmArgs a, MxOperands mx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- block -> tile (XCD-aware, grouped along M: gemm.hip) ----
  const int ntm = (a.M + BM - 1) / BM, ntn = a.N / BN;
  const int nwg = ntm * ntn;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  constexpr int GM = 8;
  const int per_group = GM * ntn;
  const int group = bid / per_group, first_m = group * GM;
  const int gs = min(ntm - first_m, GM);
  const int tm = first_m + (bid % per_group) % gs;
  const int tn = (bid % per_group) / gs;
  const int m0 = tm * BM, n0 = tn * BN;
  const int nt = a.K / BKB;
  const int kb = a.K >> 5;   // scale bytes per row

  // descriptors based at the tile origin; rows past M / N read as zero codes and zero scale bytes (2^-127 x 0)
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(mx.A + (long)m0 * mx.lda, (long)(a.M - m0 - 1) * mx.lda + a.K);
  const __amdgpu_buffer_rsrc_t rsW = make_rsrc(mx.W + (long)n0 * mx.ldw, (long)(a.N - n0 - 1) * mx.ldw + a.K);
  const __amdgpu_buffer_rsrc_t rsAs = make_rsrc(mx.As + (long)m0 * mx.ldas, (long)(a.M - m0 - 1) * mx.ldas + kb);
  const __amdgpu_buffer_rsrc_t rsWs = make_rsrc(mx.Ws + (long)n0 * mx.ldws, (long)(a.N - n0 - 1) * mx.ldws + kb);
  const int i16 = lane & 15, sh = 8 * (lane >> 4);
  int soA[4], soW[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    soA[i] = (int)((long)(wm * 64 + i * 16 + i16) * mx.ldas);
    soW[i] = (int)((long)(wn * 64 + i * 16 + i16) * mx.ldws);
  }

  auto stage = [&](int t, int buf) {
    char* tp = smem + buf * STAGE_BYTES;
    stage_codes(rsA, tp, mx.lda, t * BKB, tid, wave);
    stage_codes(rsW, tp + TILE_BYTES, mx.ldw, t * BKB, tid, wave);
  };
  unsigned sa[4], sw[4];   // the K step's four scale bytes of this lane's rows
  auto load_scales = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa[i] = __builtin_amdgcn_raw_buffer_load_b32(rsAs, soA[i] + 4 * t, 0, 0);
      sw[i] = __builtin_amdgcn_raw_buffer_load_b32(rsWs, soW[i] + 4 * t, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  load_scales(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    int ca[4], cw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ca[i] = (int)((sa[i] >> sh) & 0xFFu);
      cw[i] = (int)((sw[i] >> sh) & 0xFFu);
    }
    if (t + 1 < nt) {
      stage(t + 1, buf ^ 1);
      load_scales(t + 1);
    }
    const char* tp = smem + buf * STAGE_BYTES;
    const char* tq = tp + TILE_BYTES;
    i32x8 pf[4], qf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pf[i] = frag_codes(tp, wm * 64 + i * 16, lane);
      qf[i] = frag_codes(tq, wn * 64 + i * 16, lane);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qf[j], pf[i], acc[i][j], 0, 0, 0, cw[j], 0, ca[i]);
    __syncthreads();
  }
  // (the K loop ended on a __syncthreads: the tile buffers are free, each wave stages through its own 4 KiB)
  tile_epilogue<EPI, 4>(a, acc, m0, wm * 64, n0 + wn * 64, lane, 0, smem + wave * EPI_STAGE_BYTES);
}

template <int EPI>
int launch(const GemmArgs& a, const MxOperands& mx, hipStream_t stream) {
  static bool reserved = false;
  if (const int rc = reed_reserve_lds(reserved, (const void*)gemm_mxfp8_kernel<EPI>, 2 * STAGE_BYTES, "gemm_mxfp8")) return rc;
  const int ntm = cdiv(a.M, BM), ntn = a.N / BN;
  REED_KLAUNCH((gemm_mxfp8_kernel<EPI>), dim3(ntm * ntn), dim3(256), 2 * STAGE_BYTES, stream, a, mx);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

}  // namespace

extern "C" int reed_mx_quantize(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, int R, int K,
                                void* stream) {
  REED_CHECK_ARG(x && codes && scales, "reed_mx_quantize: null pointer");
  REED_CHECK_ARG(R >= 1 && K >= 32 && K % 32 == 0, "reed_mx_quantize: R=%d >= 1, K=%d a positive multiple of 32", R, K);
  REED_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ldq >= K && ldq % 8 == 0 && lds >= K / 32,
                 "reed_mx_quantize: leading dims ldx=%ld, ldq=%ld >= K in multiples of 8, lds=%ld >= K/32", (long)ldx, (long)ldq,
                 (long)lds);
  REED_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)codes % 8) == 0, "reed_mx_quantize: x must be 16-byte, codes 8-byte aligned");
  const long threads = (long)R * (K / 8);
  const long blocks = (threads + 255) / 256;
  REED_CHECK_ARG(blocks < (1l << 31), "reed_mx_quantize: too many elements for one launch");
  REED_KLAUNCH(mx_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (long)ldx,
               (unsigned char*)codes, (long)ldq, (unsigned char*)scales, (long)lds, R, K);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_gemm_mxfp8(int epilogue, const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Wq, int64_t ldw,
                               const void* Ws, int64_t ldws, int M, int N, int K, void* C, int64_t ldc, void* C2, int64_t ldc2,
                               const void* R, int64_t ldr, const void* bias, const void* gate, int64_t ldgate, int rows_per_gate,
                               void* stream) {
  if (const int rc = reed_gemm_mxfp8_plan(epilogue, M, N, K)) return rc;
  REED_CHECK_ARG(Aq && As && Wq && Ws && (C || epilogue == EPI_GELU), "reed_gemm_mxfp8: null operand");
  if (epilogue == EPI_GELU) REED_CHECK_ARG(C2, "reed_gemm_mxfp8: activation epilogue needs C2");
  if (epilogue == EPI_GATE_RES) REED_CHECK_ARG(R && gate, "reed_gemm_mxfp8: gate-residual epilogue needs R and gate");
  REED_CHECK_ARG(lda >= K && ldw >= K && lda % 16 == 0 && ldw % 16 == 0 && ((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0,
                 "reed_gemm_mxfp8: code matrices must be 16-byte aligned with leading dims >= K in multiples of 16");
  REED_CHECK_ARG(ldas >= K / 32 && ldws >= K / 32 && ldas % 4 == 0 && ldws % 4 == 0 && ((uintptr_t)As % 4) == 0 && ((uintptr_t)Ws % 4) == 0,
                 "reed_gemm_mxfp8: scale matrices must be 4-byte aligned with leading dims >= K/32 in multiples of 4");
  REED_CHECK_ARG(lda < (1 << 20) && ldw < (1 << 20) && ldas < (1 << 20) && ldws < (1 << 20),
                 "reed_gemm_mxfp8: operand leading dims must be below 2^20 (32-bit tile offsets)");
  REED_CHECK_ARG(ldc >= 0 && ldc < (1 << 20) && ldc2 >= 0 && ldc2 < (1 << 20) && ldr >= 0 && ldr < (1 << 20) && ldc % 8 == 0 &&
                     ldc2 % 8 == 0 && ldr % 8 == 0 && ((uintptr_t)C % 16) == 0 && ((uintptr_t)C2 % 16) == 0 && ((uintptr_t)R % 16) == 0,
                 "reed_gemm_mxfp8: output/residual must be 16-byte aligned with leading dims in multiples of 8 below 2^20");
  GemmArgs a{};
  a.M = M;
  a.N = N;
  a.K = K;
  a.C = C;
  a.ldc = ldc;
  a.C2 = C2;
  a.ldc2 = ldc2;
  a.R = R;
  a.ldr = ldr;
  a.bias = (const bf16*)bias;
  a.gate = (const bf16*)gate;
  a.ldgate = ldgate;
  a.rows_per_gate = rows_per_gate > 0 ? rows_per_gate : 1;
  const MxOperands mx{(const unsigned char*)Aq, (const unsigned char*)As, (const unsigned char*)Wq, (const unsigned char*)Ws,
                      (long)lda, (long)ldas, (long)ldw, (long)ldws};
  int rc = REED_ERR_ARG;   // (reed_gemm_mxfp8_plan has refused every epilogue outside the set)
  epi_dispatch<EPIS_MXFP8>(epilogue, [&](auto e) { rc = launch<decltype(e)::value>(a, mx, (hipStream_t)stream); });
  return rc;
}
