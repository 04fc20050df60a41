// Optimiser side of the train step as ONE pass over a flat parameter arena
// (image/train.py:402-409 clip_grad_norm_(1.0) + AdamW.step, :94-105/:411-412 update_ema):
// the reference walks 298 tensors with foreach kernels (~40 B/param of HBM traffic spread over
// hundreds of launches); here grads, master weights, both Adam moments, the EMA copy and the bf16
// compute shadow are contiguous arenas with identical layout, so it is three launches:
// squared-norm partials, finalize (norm + clip coefficient stay on the device: no host sync), and a
// fused clip * AdamW + EMA + bf16-shadow update.  Deterministic (fixed reduction order).
#include "../../include/reed_hip.h"
#include <stdlib.h>

#include "common.hpp"

#ifndef REED_OPT_NT
#define REED_OPT_NT 1
#endif
namespace {

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, long n4, long n,
                                                     float* __restrict__ partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 v = *(const f32x4*)(g + i * 4);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { float v = g[(n4 << 2) + threadIdx.x]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void clip_finalize_kernel(const float* __restrict__ partial, int nb, float max_norm,
                                                            float* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += (double)partial[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float norm = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
    out[0] = norm;
    out[1] = fminf(1.f, max_norm / (norm + 1e-6f));
  }
}

// Dynamic loss scaling for fp16 training (torch.amp.GradScaler as accelerate drives it: scale(loss).backward(), unscale_
// before clip_grad_norm_, step skipped on inf / nan, update(); image/train.py:401-409 under --mixed-precision fp16), on the
// device: state = [scale, growth_tracker, found_inf (this step), good_steps (optimiser steps actually taken)].
// The gradients in the arena are scale x the true ones; out[0] = the true norm (inf / nan on overflow, as the reference
// logs it), out[1] = clip coefficient / scale (unscale and clip in the one multiply the update applies), 0 on overflow.
__global__ __launch_bounds__(256) void clip_finalize_scaled_kernel(const float* __restrict__ partial, int nb, float max_norm,
                                                                   float* __restrict__ out, float* __restrict__ st,
                                                                   float growth, float backoff, float interval) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += (double)partial[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float scale = st[0];
    const float norm_s = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
    const bool bad = !(norm_s <= 3.0e38f);          // inf or nan anywhere in the scaled gradients
    const float norm = norm_s / scale;
    out[0] = norm;
    out[1] = bad ? 0.f : (max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f) / scale;
    if (bad) {
      st[0] = scale * backoff;
      st[1] = 0.f;
      st[2] = 1.f;
    } else {
      float tr = st[1] + 1.f;
      if (tr >= interval) { st[0] = scale * growth; tr = 0.f; }
      st[1] = tr;
      st[2] = 0.f;
      st[3] += 1.f;
    }
  }
}

struct AdamArgs {
  float lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay;
};

// The terms every thread of an update kernel derives from its arguments (adamw_ema_kernel and adamw_ema_ranges_kernel).
struct AdamStep {
  float clip, step_size, bc2s;
  bool skip;
};

__device__ __forceinline__ AdamStep adam_step(const float* __restrict__ norm_clip, const float* __restrict__ scaler,
                                              const AdamArgs& a) {
  AdamStep s;
  s.clip = norm_clip ? norm_clip[1] : 1.f;
  // with a loss scaler: an overflowed step leaves p, m, v untouched (GradScaler.step skips optimizer.step; the EMA update
  // and the shadow still run, train.py:411-412), and the bias corrections count the steps actually taken
  s.skip = scaler && scaler[2] != 0.f;
  const float bc1 = scaler ? 1.f - powf(a.beta1, scaler[3]) : a.bc1;
  const float bc2 = scaler ? 1.f - powf(a.beta2, scaler[3]) : a.bc2;
  s.step_size = a.lr / bc1;
  s.bc2s = sqrtf(bc2);
  return s;
}

// REED_OPT_NT (round 4, default): the state arrays (read once and written once per step: 38 B per parameter) with the
// non-temporal policy, so that the pass, which runs beside the next forward, does not walk through the caches its GEMMs'
// operands are served from; the 16-bit weights it writes for that forward keep the default policy.  Bit-identical.  The pass
// alone 5.13 -> 4.84 ms (5.60 -> 5.94 TB/s); whole step at b = 32 934.5 -> 947.8 images/s (three pairs), at b = 256 unchanged
// (profiles/r4_optimizer_nt.txt)
#if REED_OPT_NT
#define OPT_LD(ptr) __builtin_nontemporal_load((const f32x4*)(ptr))
#define OPT_ST(ptr, val) __builtin_nontemporal_store((val), (f32x4*)(ptr))
#else
#define OPT_LD(ptr) (*(const f32x4*)(ptr))
#define OPT_ST(ptr, val) (*(f32x4*)(ptr) = (val))
#endif

// clip * AdamW of the four elements at i (torch.optim.AdamW: decoupled decay, lerp / addcmul moments); pv holds p on entry and
// the updated p on return
__device__ __forceinline__ void adam_update4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long i, f32x4& pv, const AdamStep& s, const AdamArgs& a) {
  f32x4 gv = OPT_LD(g + i * 4);
  f32x4 mv = OPT_LD(m + i * 4);
  f32x4 vv = OPT_LD(v + i * 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float gg = gv[j] * s.clip;
    float pp = pv[j] * (1.f - a.lr * a.wd);
    mv[j] = mv[j] + (1.f - a.beta1) * (gg - mv[j]);           // exp_avg.lerp_(grad, 1-beta1)
    vv[j] = vv[j] * a.beta2 + (1.f - a.beta2) * gg * gg;      // mul_(beta2).addcmul_(g, g, 1-beta2)
    float denom = sqrtf(vv[j]) / s.bc2s + a.eps;
    pv[j] = pp - s.step_size * (mv[j] / denom);
  }
  OPT_ST(p + i * 4, pv);
  OPT_ST(m + i * 4, mv);
  OPT_ST(v + i * 4, vv);
}

// update_ema's lerp towards (the possibly just updated) pv and the 16-bit copy of pv, both optional
__device__ __forceinline__ void ema_shadow4(float* __restrict__ ema, bf16* __restrict__ shadow, long i, const f32x4& pv,
                                            const AdamArgs& a) {
  if (ema) {
    f32x4 ev = OPT_LD(ema + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = ev[j] * a.ema_decay + pv[j] * (1.f - a.ema_decay);  // mul_(d).add_(p, alpha=1-d)
    OPT_ST(ema + i * 4, ev);
  }
  if (shadow) {
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f2bf(pv[j]);
    *(bf16x4*)(shadow + i * 4) = o;
  }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, bf16* __restrict__ shadow, long n4_train,
                                                        long n4_total, const float* __restrict__ norm_clip,
                                                        const float* __restrict__ scaler, AdamArgs a) {
  const AdamStep s = adam_step(norm_clip, scaler, a);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4_total; i += (long)gridDim.x * 256) {
    f32x4 pv = OPT_LD(p + i * 4);
    if (i < n4_train && !s.skip) adam_update4(p, g, m, v, i, pv, s, a);
    ema_shadow4(ema, shadow, i, pv, a);
  }
}

// ---- the same two passes over a SET of ranges of the arena (a partly frozen model: reed_amd/optim.py) -------------------------
// The table: nranges sorted, disjoint [begin, end) pairs in arena elements, every bound a multiple of 4, so that a 4-element
// vector lies wholly inside a range or wholly outside.  Every block copies it into LDS once, in units of 4 elements (int: an
// arena of up to 2^33 elements), and looks ranges up there: no HBM traffic per element beyond the pass's own.
constexpr int kMaxRanges = 1024;

// exclusive prefix sums of the range lengths into pre[0 .. nr] (pre[nr] = the union's length), four ranges per thread
__device__ __forceinline__ void range_prefix(const int* __restrict__ sb, const int* __restrict__ se, int nr, int* __restrict__ pre,
                                             int* __restrict__ wsum) {
  const int t = threadIdx.x;
  int len[4], own = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = 4 * t + k;
    len[k] = r < nr ? se[r] - sb[r] : 0;
    own += len[k];
  }
  int inc = own;   // inclusive scan over the wave, then over the four waves through LDS
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if ((t & 63) >= d) inc += up;
  }
  if ((t & 63) == 63) wsum[t >> 6] = inc;
  __syncthreads();
  int base = inc - own;
  for (int w = 0; w < (t >> 6); ++w) base += wsum[w];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = 4 * t + k;
    if (r <= nr) pre[r] = base;
    base += len[k];
  }
  if (t == 255 && nr == 4 * 256) pre[nr] = base;   // a full table: the total has no slot among the 1024 above
  __syncthreads();
}

// Squared-norm partials over the union of the ranges: the union's vectors are numbered 0 .. total4 - 1 in arena order and dealt
// to the threads exactly as sqnorm_kernel deals [0, n4): vector j to thread j mod (256 gridDim) — a fixed assignment, no atomics,
// every block writes its partial.
__global__ __launch_bounds__(256) void sqnorm_ranges_kernel(const float* __restrict__ g, const long* __restrict__ ranges, int nr,
                                                            float* __restrict__ partial) {
  __shared__ int sb[kMaxRanges], se[kMaxRanges], pre[kMaxRanges + 1];
  __shared__ int wsum[4];
  __shared__ float red[4];
  for (int r = threadIdx.x; r < nr; r += 256) {
    sb[r] = (int)(ranges[2 * r] >> 2);
    se[r] = (int)(ranges[2 * r + 1] >> 2);
  }
  __syncthreads();
  range_prefix(sb, se, nr, pre, wsum);
  const long total4 = pre[nr];
  float s = 0.f;
  int r = 0;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total4; j += (long)gridDim.x * 256) {
    int hi = nr;                       // the last range r with pre[r] <= j (j grows: the search starts at the previous one)
    while (hi - r > 1) {
      const int mid = (r + hi) >> 1;
      if (pre[mid] <= j) r = mid; else hi = mid;
    }
    const long i = (long)sb[r] + (j - pre[r]);
    f32x4 v = *(const f32x4*)(g + i * 4);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// adamw_ema_kernel with the AdamW update only on the vectors inside a range; base4 = the arena offset of p[0] in vectors (the
// pointers of a call on one update chunk are offset, the table is not).  The EMA lerp and the shadow cover [0, n4_total) as before.
__global__ __launch_bounds__(256) void adamw_ema_ranges_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               float* __restrict__ ema, bf16* __restrict__ shadow, long n4_train,
                                                               long n4_total, const float* __restrict__ norm_clip,
                                                               const float* __restrict__ scaler, AdamArgs a,
                                                               const long* __restrict__ ranges, int nr, long base4) {
  __shared__ int sb[kMaxRanges], se[kMaxRanges];
  for (int r = threadIdx.x; r < nr; r += 256) {
    sb[r] = (int)(ranges[2 * r] >> 2);
    se[r] = (int)(ranges[2 * r + 1] >> 2);
  }
  __syncthreads();
  const AdamStep s = adam_step(norm_clip, scaler, a);
  int r = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4_total; i += (long)gridDim.x * 256) {
    f32x4 pv = OPT_LD(p + i * 4);
    const long at = base4 + i;
    int hi = nr;                       // the first range that ends behind `at` (i grows: the search starts at the previous one)
    while (r < hi) {
      const int mid = (r + hi) >> 1;
      if (se[mid] <= at) r = mid + 1; else hi = mid;
    }
    const bool in = r < nr && sb[r] <= at;
    if (in && i < n4_train && !s.skip) adam_update4(p, g, m, v, i, pv, s, a);
    ema_shadow4(ema, shadow, i, pv, a);
  }
}

// The caller's host copy of the table is what the entry points check (the device copy is read by the kernels only: no copy
// back, no synchronisation).
int check_ranges(const int64_t* h, int nr, int64_t limit, const char* who) {
  REED_CHECK_ARG(nr >= 0 && nr <= kMaxRanges, "%s: %d ranges, at most %d", who, nr, kMaxRanges);
  REED_CHECK_ARG(nr == 0 || h, "%s: null host copy of the ranges", who);
  int64_t prev = 0;
  for (int r = 0; r < nr; ++r) {
    const int64_t b = h[2 * r], e = h[2 * r + 1];
    REED_CHECK_ARG(b % 4 == 0 && e % 4 == 0, "%s: range %d [%ld, %ld) is misaligned: bounds must be multiples of 4", who, r,
                   (long)b, (long)e);
    REED_CHECK_ARG(b >= 0 && b < e, "%s: range %d [%ld, %ld) is empty or reversed", who, r, (long)b, (long)e);
    REED_CHECK_ARG(b >= prev, "%s: range %d [%ld, %ld) is unsorted or overlaps its predecessor (which ends at %ld)", who, r,
                   (long)b, (long)e, (long)prev);
    REED_CHECK_ARG(e <= limit, "%s: range %d [%ld, %ld) reaches past the end %ld", who, r, (long)b, (long)e, (long)limit);
    prev = e;
  }
  return REED_OK;
}

}  // namespace

extern "C" int reed_grad_sqnorm(const float* g, int64_t n, float* partial, int nblocks, void* stream) {
  REED_CHECK_ARG(g && partial && nblocks > 0 && n >= 0, "grad_sqnorm: bad args");
  REED_CHECK_ARG(((uintptr_t)g % 16) == 0, "grad_sqnorm: misaligned");
  REED_KLAUNCH(sqnorm_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, g, (long)(n >> 2), (long)n,
                     partial);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_clip_finalize(const float* partial, int nblocks, float max_norm, float* norm_clip,
                                  void* stream) {
  REED_CHECK_ARG(partial && norm_clip, "clip_finalize: null pointer");
  REED_KLAUNCH(clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblocks, max_norm,
                     norm_clip);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_clip_finalize_scaled(const float* partial, int nblocks, float max_norm, float* norm_clip,
                                         float* scaler_state, float growth_factor, float backoff_factor,
                                         float growth_interval, void* stream) {
  REED_CHECK_ARG(partial && norm_clip && scaler_state, "clip_finalize_scaled: null pointer");
  REED_KLAUNCH(clip_finalize_scaled_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblocks, max_norm,
               norm_clip, scaler_state, growth_factor, backoff_factor, growth_interval);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, void* shadow,
                              int64_t n_train, int64_t n_total, const float* norm_clip, const float* scaler_state,
                              float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2,
                              float ema_decay, void* stream) {
  REED_CHECK_ARG(p && (n_train == 0 || (g && m && v)), "adamw_ema: null pointer");
  REED_CHECK_ARG(n_train % 4 == 0 && n_total % 4 == 0 && n_train <= n_total,
                 "adamw_ema: n_train=%ld n_total=%ld must be multiples of 4 with n_train <= n_total", (long)n_train,
                 (long)n_total);
  AdamArgs a{lr, beta1, beta2, eps, weight_decay, bc1, bc2, ema_decay};
  long n4 = n_total >> 2;
  int blocks = (int)((n4 + 255) / 256);
  constexpr int cap = 8192;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  REED_KLAUNCH(adamw_ema_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                     (bf16*)shadow, (long)(n_train >> 2), n4, norm_clip, scaler_state, a);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_grad_sqnorm_ranges(const float* g, const int64_t* ranges, const int64_t* ranges_host, int nranges,
                                       int64_t n, float* partial, int nblocks, void* stream) {
  REED_CHECK_ARG(g && partial && nblocks > 0 && n >= 0 && (nranges == 0 || ranges), "grad_sqnorm_ranges: bad args");
  REED_CHECK_ARG(((uintptr_t)g % 16) == 0, "grad_sqnorm_ranges: misaligned");
  REED_CHECK_ARG(n < ((int64_t)1 << 33), "grad_sqnorm_ranges: n=%ld is past 2^33", (long)n);
  if (int rc = check_ranges(ranges_host, nranges, n, "grad_sqnorm_ranges")) return rc;
  REED_KLAUNCH(sqnorm_ranges_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, g, (const long*)ranges, nranges, partial);
  REED_LAUNCH_CHECK();
  return REED_OK;
}

extern "C" int reed_adamw_ema_ranges(float* p, const float* g, float* m, float* v, float* ema, void* shadow,
                                     int64_t n_train, int64_t n_total, const float* norm_clip, const float* scaler_state,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2,
                                     float ema_decay, const int64_t* ranges, const int64_t* ranges_host, int nranges,
                                     int64_t offset, void* stream) {
  REED_CHECK_ARG(p && (n_train == 0 || (g && m && v)) && (nranges == 0 || ranges), "adamw_ema_ranges: null pointer");
  REED_CHECK_ARG(n_train % 4 == 0 && n_total % 4 == 0 && n_train <= n_total && n_train >= 0,
                 "adamw_ema_ranges: n_train=%ld n_total=%ld must be multiples of 4 with n_train <= n_total", (long)n_train,
                 (long)n_total);
  REED_CHECK_ARG(offset >= 0 && offset % 4 == 0 && offset + n_total < ((int64_t)1 << 33),
                 "adamw_ema_ranges: offset=%ld must be a multiple of 4 with offset + n_total below 2^33", (long)offset);
  if (int rc = check_ranges(ranges_host, nranges, offset + n_total, "adamw_ema_ranges")) return rc;
  AdamArgs a{lr, beta1, beta2, eps, weight_decay, bc1, bc2, ema_decay};
  long n4 = n_total >> 2;
  int blocks = (int)((n4 + 255) / 256);
  constexpr int cap = 8192;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  REED_KLAUNCH(adamw_ema_ranges_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, (bf16*)shadow,
               (long)(n_train >> 2), n4, norm_clip, scaler_state, a, (const long*)ranges, nranges, (long)(offset >> 2));
  REED_LAUNCH_CHECK();
  return REED_OK;
}
