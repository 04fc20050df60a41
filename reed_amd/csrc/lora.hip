// LoRA (low-rank adapters W' = W + s B A on a block linear): the merge that keeps the hot GEMMs untouched, and the adapters'
// gradients from the (dy, x) pair of the linear.
//
// reed_lora_merge   one pass over W: w' = w + s * sum_j b[n, j] a[j, k] (fp32, j ascending, one fma per j from 0; the update is
//                   added with one more fma; an update that is exactly zero leaves w as it is, sign of zero included), written as
//                   the operand-type shadow r(w') and / or as fp32.  A workgroup owns a 256-column chunk of `a` in LDS (R x 1 KiB)
//                   and walks 64 rows of W, a wave per row: 4 bytes read and 2 written per element of W, `a` and `b` from L2.
//
// reed_lora_grads   with u = r(s * (x a^T)) and v = r(s * (dy b)), both [M, R] in the operand type:
//                     db[n, j] (+)= sum_m dy[m, n] u[m, j]        da[j, k] (+)= sum_m v[m, j] x[m, k]
//                   THE SCALE IS APPLIED TO u AND v, in fp32, in front of their rounding; the two products that follow carry none.
//   16-bit builds, four launches, v_mfma_f32_16x16x32 throughout (the R-wide side is the 16-wide side of the tile; R = 8 is
//   padded with zero FRAGMENTS: a lane whose column is >= R never forms an address):
//     1  bt = b^T [R, N]                                        (N R elements; so that step 2 is one kernel form)
//     2  u, v: a wave owns 16 rows of x (dy) and all R columns; operands straight from global memory, 16 bytes per lane
//     3  per (128-column strip of dy | x, row slab of M): the strip in 32-row steps through LDS (the contraction runs over
//        M, the strided index of both operands), a wave owns 32 columns x R; fp32 partials [slab][N, R] | [slab][R, K]
//     4  the partials summed over the slabs in ascending order, then added to the prior value when `accumulate`
//   No atomics anywhere: two runs give the same bits.
//   Bytes moved: x and dy are each read TWICE (steps 2 and 3): 4 M (N + K) bytes, plus 8 M R for u and v written and read,
//   plus 8 S R (N + K) for the S <= 32 slabs of partials written and read.  The floor named in the issue (x twice, dy once)
//   would need v formed inside step 3 from the very strip it contracts, which a 128-column strip does not hold.
//   fp32 build: the same entry point composed of that build's own kernels: reed_gemm (NT for u, NN for v), one scaling pass
//   over u | v, reed_smallk_wgrad in its two layouts (its own fixed-order two-stage reduction).
#include "../../include/reed_hip.h"
#include "common.hpp"
#include "gemm.h"

namespace {

constexpr int MG_COLS = 256;   // columns of W per workgroup of the merge (64 lanes x 4)
constexpr int MG_ROWS = 64;    // rows of W per workgroup

__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ w, const float* __restrict__ a,
                                                         const float* __restrict__ b, float scale, bf16* __restrict__ w_op,
                                                         float* __restrict__ w32, int N, int K, int R) {
  extern __shared__ __attribute__((aligned(16))) float al[];   // [R][MG_COLS]
  const int k0 = blockIdx.x * MG_COLS, n0 = blockIdx.y * MG_ROWS;
  for (int i = threadIdx.x; i < R * (MG_COLS / 4); i += 256) {
    const int j = i / (MG_COLS / 4), c = (i % (MG_COLS / 4)) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k0 + c < K) v = *(const f32x4*)(a + (long)j * K + k0 + c);   // K % 4 == 0
    *(f32x4*)(al + j * MG_COLS + c) = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = k0 + lane * 4;
  if (k >= K) return;
  const int n_end = min(N, n0 + MG_ROWS);
  for (int n = n0 + wave; n < n_end; n += 4) {
    const float* br = b + (long)n * R;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < R; ++j) {
      const float bj = br[j];
      const f32x4 av = *(const f32x4*)(al + j * MG_COLS + lane * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(bj, av[e], acc[e]);
    }
    const long o = (long)n * K + k;
    const f32x4 wv = *(const f32x4*)(w + o);
    f32x4 r;
    bf16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = acc[e] == 0.f ? wv[e] : fmaf(scale, acc[e], wv[e]);
      h[e] = f2bf(r[e]);
    }
    if (w32) *(f32x4*)(w32 + o) = r;
    if (w_op) *(bf16x4*)(w_op + o) = h;
  }
}

#if !defined(REED_FP32)
// out[i] (+)= part[0][i] + part[1][i] + ... (ascending), for the two outputs of one call laid end to end: i < n0 -> out0
__global__ __launch_bounds__(256) void lora_reduce_kernel(const float* __restrict__ part0, const float* __restrict__ part1,
                                                          int nslab, float* __restrict__ out0, long n0, float* __restrict__ out1,
                                                          long n1, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n0 + n1) return;
  const bool first = i < n0;
  const float* p = first ? part0 + i : part1 + (i - n0);
  const long stride = first ? n0 : n1;
  float s = p[0];
  for (int k = 1; k < nslab; ++k) s += p[(long)k * stride];
  float* o = first ? out0 + i : out1 + (i - n0);
  *o = accumulate ? *o + s : s;
}


constexpr int UV_ROWS = 64;      // rows of x | dy per workgroup of step 2 (4 waves x 16)
constexpr int WG_STEP = 32;      // rows of M per MFMA step of step 3 (the K of v_mfma_f32_16x16x32)
constexpr int WG_COLS = 128;     // columns of dy | x per workgroup of step 3
constexpr int WG_PITCH = WG_COLS + 8;   // LDS row pitch of the strip (16-byte aligned rows)
constexpr int WG_SLABS = 32;     // at most this many row slabs of M

__global__ __launch_bounds__(256) void lora_bt_kernel(const bf16* __restrict__ b, bf16* __restrict__ bt, int N, int R) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // over bt [R, N]
  if (i >= (long)N * R) return;
  const int j = (int)(i / N), n = (int)(i % N);
  bt[i] = b[(long)n * R + j];
}

// blockIdx.y = 0: u = r(s x a^T) (contraction K); 1: v = r(s dy bt^T) (contraction N).  No LDS, no barrier.
template <int RT>
__global__ __launch_bounds__(256) void lora_uv_kernel(const bf16* __restrict__ x, const bf16* __restrict__ a,
                                                      const bf16* __restrict__ dy, const bf16* __restrict__ bt,
                                                      bf16* __restrict__ u, bf16* __restrict__ v, float scale, int M, int N,
                                                      int K, int R) {
  const bool second = blockIdx.y != 0;
  const bf16* in = second ? dy : x;
  const bf16* wt = second ? bt : a;
  bf16* out = second ? v : u;
  const int Kd = second ? N : K;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
  const int m0 = blockIdx.x * UV_ROWS + wave * 16;
  if (m0 >= M) return;
  const bool row_ok = m0 + c < M;
  const bf16* ir = in + (long)(m0 + c) * Kd + 8 * h;
  const bf16x8 zero = {};
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Kd; k0 += 32) {
    const bf16x8 af = row_ok ? *(const bf16x8*)(ir + k0) : zero;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int j = t * 16 + c;
      const bf16x8 bf = j < R ? *(const bf16x8*)(wt + (long)j * Kd + k0 + 8 * h) : zero;
      acc[t] = REED_MFMA_16x16x32(af, bf, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int j = t * 16 + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 4 * h + e;
      if (m < M && j < R) out[(long)m * R + j] = f2bf(scale * acc[t][e]);
    }
  }
}

// blockIdx.x < N / 128: db partial of this strip of dy (with u); otherwise da partial of a strip of x (with v).
template <int RT>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                         const bf16* __restrict__ u, const bf16* __restrict__ v,
                                                         float* __restrict__ part_db, float* __restrict__ part_da, int M, int N,
                                                         int K, int R, int slab_rows) {
  constexpr int SP = RT * 16 + 8;     // LDS row pitch of the u | v tile
  __shared__ __attribute__((aligned(16))) bf16 wl[WG_STEP * WG_PITCH];
  __shared__ __attribute__((aligned(16))) bf16 sl[WG_STEP * SP];
  const int nbN = N / WG_COLS;
  const bool isdb = (int)blockIdx.x < nbN;
  const bf16* wide = isdb ? dy : x;
  const bf16* small = isdb ? u : v;
  const int ldw = isdb ? N : K;
  const int c0 = (isdb ? blockIdx.x : blockIdx.x - nbN) * WG_COLS;
  const int m_begin = blockIdx.y * slab_rows, m_end = min(M, m_begin + slab_rows);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, h = lane >> 4;
  const bf16x8 zero = {};
  f32x4 acc[2][RT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m0 = m_begin; m0 < m_end; m0 += WG_STEP) {
    for (int i = tid; i < WG_STEP * (WG_COLS / 8); i += 256) {
      const int row = i >> 4, ch = i & 15;
      bf16x8 val = zero;
      if (m0 + row < m_end) val = *(const bf16x8*)(wide + (long)(m0 + row) * ldw + c0 + ch * 8);
      *(bf16x8*)(wl + row * WG_PITCH + ch * 8) = val;
    }
    if (tid < WG_STEP * RT * 2) {
      const int row = tid / (RT * 2), ch = tid % (RT * 2);
      bf16x8 val = zero;
      if (m0 + row < m_end && ch * 8 < R) val = *(const bf16x8*)(small + (long)(m0 + row) * R + ch * 8);   // R % 8 == 0
      *(bf16x8*)(sl + row * SP + ch * 8) = val;
    }
    __syncthreads();
    bf16x8 af[2], bf[RT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) af[i][j] = wl[(8 * h + j) * WG_PITCH + wave * 32 + i * 16 + c];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) bf[t][j] = sl[(8 * h + j) * SP + t * 16 + c];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[i][t] = REED_MFMA_16x16x32(af[i], bf[t], acc[i][t]);
    __syncthreads();
  }
  // C tile: row (a column of dy | x) = 4 h + e, column (the adapter index) = c
  float* part = isdb ? part_db + (long)blockIdx.y * N * R : part_da + (long)blockIdx.y * R * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int j = t * 16 + c;
      if (j >= R) continue;
      const int col = c0 + wave * 32 + i * 16 + 4 * h;
      if (isdb) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(long)(col + e) * R + j] = acc[i][t][e];
      } else {
        *(f32x4*)(part + (long)j * K + col) = acc[i][t];
      }
    }
}

inline int wg_slab_rows(int M) { return cdiv(cdiv(M, WG_SLABS), WG_STEP) * WG_STEP; }
#else
__global__ __launch_bounds__(256) void lora_scale_kernel(float* __restrict__ p, long n, float scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = scale * p[i];
}
#endif

inline int64_t align4(int64_t n) { return (n + 3) / 4 * 4; }

bool lora_rank_ok(int R) { return R == 8 || R == 16 || R == 32 || R == 64; }

}  // namespace

extern "C" int reed_lora_merge(const float* w, const float* a, const float* b, float scale, void* w_op, float* w32, int N, int K,
                               int R, void* stream) {
  REED_CHECK_ARG(w && a && b && (w_op || w32), "lora_merge: null pointer");
  REED_CHECK_ARG(lora_rank_ok(R), "lora_merge: R=%d must be 8, 16, 32 or 64", R);
  REED_CHECK_ARG(N > 0 && K > 0 && K % 4 == 0, "lora_merge: N=%d, K=%d (K a positive multiple of 4)", N, K);
  REED_CHECK_ARG(((uintptr_t)w % 16) == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)w_op % (4 * sizeof(bf16))) == 0 && ((uintptr_t)w32 % 16) == 0,
                 "lora_merge: w, a, w32 must be 16-byte aligned (w_op: 4 elements)");
  REED_KLAUNCH(lora_merge_kernel, dim3(cdiv(K, MG_COLS), cdiv(N, MG_ROWS)), dim3(256), (size_t)R * MG_COLS * sizeof(float),
               (hipStream_t)stream, w, a, b, scale, (bf16*)w_op, w32, N, K, R);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

static int lora_grads_domain(int M, int N, int K, int R) {
#if defined(REED_FP32)
  const int q = 4;
#else
  const int q = 128;
#endif
  REED_CHECK_ARG(lora_rank_ok(R), "lora_grads: R=%d must be 8, 16, 32 or 64", R);
  REED_CHECK_ARG(M >= 1 && N > 0 && K > 0 && N % q == 0 && K % q == 0, "lora_grads: M=%d, N=%d, K=%d (N and K multiples of %d)", M, N,
                 K, q);
  return REED_OK;
}

extern "C" int64_t reed_lora_grads_ws_floats(int M, int N, int K, int R) {
  if (lora_grads_domain(M, N, K, R) != REED_OK) return -1;
#if defined(REED_FP32)
  return 2 * align4((int64_t)M * R) + reed_smallk_wgrad_ws_floats(N > K ? N : K, R);
#else
  const int64_t nslab = cdiv(M, wg_slab_rows(M));
  return align4((int64_t)M * R) + align4((int64_t)N * R / 2) + nslab * (int64_t)R * ((int64_t)N + K);
#endif
}

extern "C" int reed_lora_grads(const void* x, const void* dy, const void* a16, const void* b16, float scale, float* da, float* db,
                               float* ws, int M, int N, int K, int R, int accumulate, void* stream) {
  REED_CHECK_ARG(x && dy && a16 && b16 && da && db && ws, "lora_grads: null pointer");
  if (int rc = lora_grads_domain(M, N, K, R)) return rc;
  REED_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)a16 % 16) == 0 && ((uintptr_t)b16 % 16) == 0 &&
                     ((uintptr_t)ws % 16) == 0 && ((uintptr_t)da % 16) == 0,
                 "lora_grads: x, dy, a16, b16, da, ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
#if defined(REED_FP32)
  float* u = ws;
  float* v = u + align4((int64_t)M * R);
  float* ws2 = v + align4((int64_t)M * R);
  int rc = reed_gemm(LAY_NT, EPI_BF16, x, K, a16, K, M, R, K, u, R, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 1, nullptr, 0, 1, 0,
                     stream);
  if (rc) return rc;
  rc = reed_gemm(LAY_NN, EPI_BF16, dy, N, b16, R, M, R, N, v, R, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 1, nullptr, 0, 1, 0,
                 stream);
  if (rc) return rc;
  const long nuv = (long)(v - u) + (long)M * R;   // u | gap | v in one pass (the gap is workspace)
  REED_KLAUNCH(lora_scale_kernel, dim3(cdiv(nuv, 256)), dim3(256), 0, st, u, nuv, scale);
  REED_LAUNCH_CHECK();
  rc = reed_smallk_wgrad(dy, 0, u, ws2, db, nullptr, nullptr, M, N, R, 0, accumulate, stream);   // db[n R + j]
  if (rc) return rc;
  return reed_smallk_wgrad(x, 0, v, ws2, da, nullptr, nullptr, M, K, R, 1, accumulate, stream);   // da[j K + k]
#else
  const int slab_rows = wg_slab_rows(M), nslab = cdiv(M, slab_rows);
  bf16* u = (bf16*)ws;
  bf16* v = u + (int64_t)M * R;
  bf16* bt = (bf16*)(ws + align4((int64_t)M * R));
  float* part_db = ws + align4((int64_t)M * R) + align4((int64_t)N * R / 2);
  float* part_da = part_db + (int64_t)nslab * N * R;
  REED_KLAUNCH(lora_bt_kernel, dim3(cdiv((long)N * R, 256)), dim3(256), 0, st, (const bf16*)b16, bt, N, R);
  REED_LAUNCH_CHECK();
  const dim3 guv(cdiv(M, UV_ROWS), 2), gwg(N / WG_COLS + K / WG_COLS, nslab);
#define LORA_LAUNCH(RT)                                                                                                        \
  do {                                                                                                                         \
    REED_KLAUNCH(lora_uv_kernel<RT>, guv, dim3(256), 0, st, (const bf16*)x, (const bf16*)a16, (const bf16*)dy, (const bf16*)bt, u, \
                 v, scale, M, N, K, R);                                                                                        \
    REED_LAUNCH_CHECK();                                                                                                       \
    REED_KLAUNCH(lora_wgrad_kernel<RT>, gwg, dim3(256), 0, st, (const bf16*)dy, (const bf16*)x, (const bf16*)u, (const bf16*)v,   \
                 part_db, part_da, M, N, K, R, slab_rows);                                                                     \
    REED_LAUNCH_CHECK();                                                                                                       \
  } while (0)
  if (R <= 16) LORA_LAUNCH(1);
  else if (R == 32) LORA_LAUNCH(2);
  else LORA_LAUNCH(4);
#undef LORA_LAUNCH
  const long n0 = (long)N * R, n1 = (long)R * K;
  REED_KLAUNCH(lora_reduce_kernel, dim3(cdiv(n0 + n1, 256)), dim3(256), 0, st, part_db, part_da, nslab, db, n0, da, n1, accumulate);
  REED_LAUNCH_CHECK();
  return REED_OK;
#endif
}
