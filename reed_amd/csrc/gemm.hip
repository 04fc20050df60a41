// bf16 MFMA GEMM for gfx950 with fused epilogues — the dense contraction behind every
// nn.Linear on the SiT hot path (reference: image/models/sit.py:17-24,114-124,126-129,146-150
// and timm Attention/Mlp linears; backward = autograd of the same).
//
//   C[M,N] (+)= sum_k P(m,k) * Q(n,k)
//
// Three operand layouts, all row-major in HBM, no transposed copies anywhere:
//   NT  P = A[M,K]  (k contiguous)   Q = B[N,K]  (k contiguous)   forward:  y = x W^T
//   NN  P = A[M,K]  (k contiguous)   Q = B[K,N]  (k strided)      dgrad:    dx = dy W
//   TN  P = A[K,M]  (k strided)      Q = B[K,N]  (k strided)      wgrad:    dW = dy^T x
// k-contiguous operands are staged as [128][64] LDS tiles (128-B rows, XOR-swizzled 16-B chunks)
// and read with ds_read_b128; k-strided operands are staged as [64][128] tiles (256-B rows,
// swizzled) and read with the gfx950 transposing read ds_read_b64_tr_b16.  Staging is
// buffer_load_dwordx4 ... lds (LDS-DMA, 16 B/lane) with hardware bounds checking, so ragged M
// (and ragged K for TN) need no masking code: out-of-range rows read as zero.
//
// Tile 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 tiles of
// v_mfma_f32_16x16x32_bf16.  The MFMA is issued "swapped" (Q fragment as A operand, P fragment
// as B operand) so each lane ends up holding 4 consecutive n for one m: 8-B bf16 / 16-B fp32
// epilogue accesses.  LDS is double buffered (64 KiB), one barrier per K step.
//
// Below the kernel: reed_gemm_launch, the entry of every reed_gemm call — pointer checks, the plan of gemm_plan.cpp (which kernels,
// on which rows and columns), and the loop that launches it.
#include "gemm_common.hpp"
#include "gemm_plan.h"

// the kernels' launchers: each runs what it is told on the problem it is given (the selection is gemm_plan.cpp's)
int reed_gemm144_launch(int layout, int epi, GemmArgs a, hipStream_t stream);                    // gemm144.hip: 256x144 tiles
int reed_gemm288_launch(int epi, GemmArgs a, hipStream_t stream);                                // gemm288.hip: 256x288 tiles (NT)
int reed_gemm256_launch(int layout, int epi, GemmArgs a, int splits, hipStream_t stream);        // gemm256.hip: 256^2, eight waves
int reed_gemm256w_launch(int layout, int epi, GemmArgs a, bool persistent, int grid, hipStream_t stream);   // gemm256w.hip: 256^2, four waves
int reed_gemm_skinny_launch(int epi, GemmArgs a, hipStream_t stream);                            // gemm_skinny.hip: 16 x 64 tiles
int reed_gemm_tn_launch(int tile, GemmArgs a, int splits, hipStream_t stream);                   // gemm_tn.hip: 256x128 / 128x256 (TN)

namespace {
using namespace gemm_detail;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 16384;          // one operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;

// ---- staging ----------------------------------------------------------------
// k-contiguous operand: tile rows [0,128) x k [k0,k0+64); rsrc is based at the tile's first row.
__device__ __forceinline__ void stage_row(__amdgpu_buffer_rsrc_t rs, char* tile, long ld, int k0,
                                          int tid, int wave) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int L = i * 256 + tid;
    int r = L >> 3, cp = L & 7;
    int c = cp ^ ((r >> 1) & 7);
    int voff = (int)(((long)r * ld + k0 + c * 8) * 2);
    char* dst = tile + (i * 256 + wave * 64) * 16;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, voff, 0, 0, 0);
  }
}
// k-strided operand: k rows [k0,k0+64) x cols [0,128); rsrc is based at column c0 of row 0.
__device__ __forceinline__ void stage_tr(__amdgpu_buffer_rsrc_t rs, char* tile, long ld, int k0,
                                         int tid, int wave) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int L = i * 256 + tid;
    int r = L >> 4, chp = L & 15;
    int ch = chp ^ tr_sw(r);
    int voff = (int)(((long)(k0 + r) * ld + ch * 8) * 2);
    char* dst = tile + (i * 256 + wave * 64) * 16;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, voff, 0, 0, 0);
  }
}

template <int LAY, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- block -> tile (XCD-aware, grouped along M) ----
  const int ntm = (a.M + BM - 1) / BM, ntn = a.N / BN;
  const int nwg = ntm * ntn;
  int bid = blockIdx.x;
  {
    int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  constexpr int GM = 8;
  const int per_group = GM * ntn;
  const int group = bid / per_group, first_m = group * GM;
  const int gs = min(ntm - first_m, GM);
  const int tm = first_m + (bid % per_group) % gs;
  const int tn = (bid % per_group) / gs;
  const int z = blockIdx.y;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = z * a.ksplit_len;
  const int kend = min(a.K, kbeg + a.ksplit_len);
  const int nt = (kend - kbeg + BK - 1) / BK;

  // ---- buffer descriptors based at this block's tile origin ----
  __amdgpu_buffer_rsrc_t rsP, rsQ;
  if constexpr (LAY == LAY_TN) {
    // P = A[K, M]: rows are k; records end at row kend
    rsP = make_rsrc(a.P + m0, ((long)kend * a.ldp - m0) * 2);
  } else {
    rsP = make_rsrc(a.P + (long)m0 * a.ldp, ((long)(a.M - m0) * a.ldp) * 2);
  }
  if constexpr (LAY == LAY_NT) {
    rsQ = make_rsrc(a.Q + (long)n0 * a.ldq, ((long)(a.N - n0) * a.ldq) * 2);
  } else {
    rsQ = make_rsrc(a.Q + n0, ((long)kend * a.ldq - n0) * 2);
  }

  auto stage = [&](int t, int buf) {
    char* tp = smem + buf * STAGE_BYTES;
    char* tq = tp + TILE_BYTES;
    int k0 = kbeg + t * BK;
    if constexpr (LAY == LAY_TN) stage_tr(rsP, tp, a.ldp, k0, tid, wave);
    else stage_row(rsP, tp, a.ldp, k0, tid, wave);
    if constexpr (LAY == LAY_NT) stage_row(rsQ, tq, a.ldq, k0, tid, wave);
    else stage_tr(rsQ, tq, a.ldq, k0, tid, wave);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_dbias = (LAY == LAY_TN) && a.dbias != nullptr && tn == 0 && wn == 0;
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;

  if (nt > 0) stage(0, 0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) stage(t + 1, buf ^ 1);
    const char* tp = smem + buf * STAGE_BYTES;
    const char* tq = tp + TILE_BYTES;
    bf16x8 pf[2][4], qf[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (LAY == LAY_TN) pf[ks][i] = frag_tr(tp, wm * 64 + i * 16, ks, lane);
        else pf[ks][i] = frag_row(tp, wm * 64 + i * 16, ks, lane);
        if constexpr (LAY == LAY_NT) qf[ks][i] = frag_row(tq, wn * 64 + i * 16, ks, lane);
        else qf[ks][i] = frag_tr(tq, wn * 64 + i * 16, ks, lane);
      }
    if constexpr (LAY != LAY_NT) REED_LDS_WAIT();  // asm transposing reads: the compiler does not count them
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = REED_MFMA_16x16x32(qf[ks][j], pf[ks][i], acc[i][j]);
      if constexpr (LAY == LAY_TN) {
        if (do_dbias) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            accb[i] = REED_MFMA_16x16x32(ones, pf[ks][i], accb[i]);
        }
      }
    }
    __syncthreads();
  }

  // (the K loop ended on a __syncthreads: the tile buffers are free, each wave stages through its own 4 KiB)
  tile_epilogue<EPI, 4>(a, acc, m0, wm * 64, n0 + wn * 64, lane, z, smem + wave * EPI_STAGE_BYTES);
  if constexpr (LAY == LAY_TN) {
    if (do_dbias && (lane >> 4) == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m < a.M) {
          if (gridDim.y > 1) a.dbias[(long)z * a.slab_stride + m] = accb[i][0];  // split-K: per-slice slab (C's stride)
          else if (a.accumulate) a.dbias[m] += accb[i][0];
          else a.dbias[m] = accb[i][0];
        }
      }
    }
  }
}

template <int LAY, int EPI>
int launch(const GemmArgs& a, int splits, hipStream_t stream) {
  static bool reserved = false;
  if (const int rc = reed_reserve_lds(reserved, (const void*)gemm_kernel<LAY, EPI>, 2 * STAGE_BYTES, "gemm")) return rc;
  const int ntm = cdiv(a.M, BM), ntn = a.N / BN;
  dim3 grid(ntm * ntn, splits, 1);
  REED_KLAUNCH((gemm_kernel<LAY, EPI>), grid, dim3(256), 2 * STAGE_BYTES, stream, a);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

template <int LAY>
int dispatch_epi(int epi, const GemmArgs& a, int splits, hipStream_t s) {
  int rc = REED_ERR_ARG;
  if (epi_dispatch<epis_128(LAY)>(epi, [&](auto e) { rc = launch<LAY, decltype(e)::value>(a, splits, s); })) return rc;
  reed_set_error("reed_gemm: unknown epilogue %d", epi);
  return REED_ERR_ARG;
}

}  // namespace

static int launch128(int layout, int epi, const GemmArgs& a, int splits, hipStream_t stream) {
  switch (layout) {
    case LAY_NT: return dispatch_epi<LAY_NT>(epi, a, splits, stream);
    case LAY_NN: return dispatch_epi<LAY_NN>(epi, a, splits, stream);
    case LAY_TN: return dispatch_epi<LAY_TN>(epi, a, splits, stream);
  }
  reed_set_error("reed_gemm: unknown layout %d", layout);
  return REED_ERR_ARG;
}

// Validate (in the order the checks have always had), ask gemm_plan.cpp which kernels run on which part of the problem, and
// launch them in order, each on the operands offset to its part (the same kernels on offset pointers: a split is bit-invisible).
int reed_gemm_launch(int layout, int epi, GemmArgs a, int splits, hipStream_t stream) {
  const GemmShape shape{layout, epi, a.M, a.N, a.K, splits, a.dbias != nullptr, a.slab_stride > 0, a.R && a.C2, a.rows_per_gate};
  if (const int rc = reed_gemm_check_dims(shape)) return rc;
  REED_CHECK_ARG(a.ldp % 8 == 0 && a.ldq % 8 == 0, "reed_gemm: leading dims must be multiples of 8 elements");
  REED_CHECK_ARG(a.ldc >= 0 && a.ldc < (1 << 20) && a.ldc2 >= 0 && a.ldc2 < (1 << 20) && a.ldr >= 0 && a.ldr < (1 << 20) &&
                     a.ldc % 8 == 0 && a.ldc2 % 8 == 0 && a.ldr % 8 == 0,
                 "reed_gemm: output/residual leading dims must be multiples of 8 below 2^20 (32-bit tile offsets)");
  REED_CHECK_ARG(((uintptr_t)a.P % 16) == 0 && ((uintptr_t)a.Q % 16) == 0 && ((uintptr_t)a.C % 16) == 0,
                 "reed_gemm: operands must be 16-byte aligned");
  GemmPlan plan;
  if (const int rc = reed_gemm_plan_shape(shape, reed_gemm_knobs(), &plan)) return rc;
  if (layout == LAY_TN_TALL || layout == LAY_TN_WIDE) layout = LAY_TN;
  const long ob = epi_out_bytes(epi);   // bytes per element of C and of R
  for (int i = 0; i < plan.n; ++i) {
    const GemmLaunch& l = plan.launch[i];
    GemmArgs b = a;
    b.M = l.rows;
    b.N = l.cols;
    b.ksplit_len = l.ksplit_len;
    b.tile_gm = l.tile_gm;
    if (l.row0 || l.col0) {   // (NT / NN only)
      b.P = a.P + (long)l.row0 * a.ldp;
      b.Q = layout == LAY_NT ? a.Q + (long)l.col0 * a.ldq : a.Q + l.col0;
      if (a.C) b.C = (char*)a.C + ((long)l.row0 * a.ldc + l.col0) * ob;
      if (a.C2) b.C2 = (char*)a.C2 + ((long)l.row0 * a.ldc2 + l.col0) * 2;
      if (a.R) b.R = (const char*)a.R + ((long)l.row0 * a.ldr + l.col0) * ob;
      if (a.bias) b.bias = a.bias + l.col0;
      if (a.gate) b.gate = a.gate + l.col0;
    }
    int rc = REED_ERR_ARG;
    switch (l.kernel) {
      case GK_128: rc = launch128(layout, epi, b, l.splits, stream); break;
      case GK_144: rc = reed_gemm144_launch(layout, epi, b, stream); break;
      case GK_288: rc = reed_gemm288_launch(epi, b, stream); break;
      case GK_256X8: rc = reed_gemm256_launch(layout, epi, b, l.splits, stream); break;
      case GK_256W: rc = reed_gemm256w_launch(layout, epi, b, false, l.grid, stream); break;
      case GK_256WP: rc = reed_gemm256w_launch(layout, epi, b, true, l.grid, stream); break;
      case GK_SKINNY: rc = reed_gemm_skinny_launch(epi, b, stream); break;
      case GK_TN_TALL: rc = reed_gemm_tn_launch(1, b, l.splits, stream); break;
      case GK_TN_WIDE: rc = reed_gemm_tn_launch(2, b, l.splits, stream); break;
    }
    if (rc != REED_OK) return rc;
  }
  return REED_OK;
}
