// Pillow's 8-bit resampler (ImagingResample: `Image.resize` on uint8) for a ragged batch of differently sized RGB images: the
// crop / resize of the reference's `dataset_tools.py convert` (image/preprocessing/dataset_tools.py:131-200), bit for bit.
// The arithmetic is integer: out = clip_0_255((2^21 + sum_t in[first + t] * k[t]) >> 22) with int32 coefficients that the host
// planner (reed_amd/resample.py) rebuilds exactly as Pillow does; a resize is a horizontal pass, then a vertical pass, each
// uint8 -> uint8, so the passes run as separate launches ("levels") over ping-pong arenas.
//
// One launch = one level of every image that has one.  An item (include/reed_hip.h: reed_resample_u8) describes one pass of
// one image; a workgroup finds its item by bisecting the prefix table of tile counts (TILE work items per workgroup).
// Images are interleaved RGB with 16-byte aligned rows, so
//   vertical    the filter is the same for every byte of a row: a lane owns one aligned dword of the row's bytes, four
//               accumulators, dword loads and a dword store (byte stores on the window's two ragged dwords);
//   horizontal  a lane owns the 4 output pixels of an aligned group of 4: twelve accumulators, three dword stores (byte stores
//               on the window's ragged groups).  The taps are byte loads straight from global memory: neighbouring lanes read
//               neighbouring segments of one row, which the vector L1 serves; no LDS staging;
//   planar      the last (vertical) pass of an image writes the R x R crop as u8 [3, R, R]: a lane owns 4 pixels = 12 source
//               bytes at any byte alignment (three or four aligned dword loads, funnel-shifted), one dword store per plane.
// Nothing outside an item's window is written: neither pitch padding nor the columns / rows later passes do not read.
// Tap indices are clamped into the source extent: the tables come from the host.
#include "../../include/reed_hip.h"
#include "common.hpp"

namespace {

constexpr int RS_TILE = 256;       // work items per workgroup (reed_amd/resample.py: TILE)
constexpr int RS_BITS = 22;        // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_HALF = 1 << (RS_BITS - 1);

struct RsItem {                    // 16 int32 words
  int64_t src_off, dst_off;
  int32_t src_pitch, dst_pitch, src_extent, out0, nout, oth0, noth, coef_off, bounds_off, ksize, kind, plane;
};
static_assert(sizeof(RsItem) == 64, "item layout");

// clip_0_255(acc >> 22), written as a clamp of the accumulator in front of a logical shift.  The direct form, clamp(acc >> 22, 0,
// 255), is selected in pairs as v_ashr_pk_u8_i32, whose result on the MI355X kept the upper half of its destination register where
// the compiler counts on zeros: the packed dword of one plane came out OR-ed with the previous plane's pixels 2 and 3.
__device__ __forceinline__ uint32_t rs_clip(int acc) {
  constexpr int top = (255 << RS_BITS) | ((1 << RS_BITS) - 1);
  const int v = acc < 0 ? 0 : (acc > top ? top : acc);
  return (uint32_t)v >> RS_BITS;
}

__device__ __forceinline__ int rs_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ void rs_horizontal(const RsItem& it, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                              const int* __restrict__ coefs, const int* __restrict__ bounds, long u) {
  const int g0 = it.out0 >> 2, ng = ((it.out0 + it.nout + 3) >> 2) - g0;
  if (u >= (long)it.noth * ng) return;
  const int row = it.oth0 + (int)(u / ng), g = g0 + (int)(u % ng);
  const uint8_t* srow = src + it.src_off + (long)row * it.src_pitch;
  uint8_t* drow = dst + it.dst_off + (long)row * it.dst_pitch;
  const int xend = it.out0 + it.nout;
  uint32_t o[12];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int x = 4 * g + p;
    int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF;
    if (x >= it.out0 && x < xend) {
      const int i = x - it.out0;
      const int first = bounds[2 * (it.bounds_off + i)], taps = min(bounds[2 * (it.bounds_off + i) + 1], it.ksize);
      const int* k = coefs + it.coef_off + (long)i * it.ksize;
      for (int t = 0; t < taps; ++t) {
        const uint8_t* s = srow + 3 * rs_clamp(first + t, it.src_extent);
        const int kt = k[t];
        a0 += (int)s[0] * kt;
        a1 += (int)s[1] * kt;
        a2 += (int)s[2] * kt;
      }
    }
    o[3 * p] = rs_clip(a0);
    o[3 * p + 1] = rs_clip(a1);
    o[3 * p + 2] = rs_clip(a2);
  }
  if (4 * g >= it.out0 && 4 * g + 4 <= xend) {
    uint32_t* d = (uint32_t*)(drow + 12 * g);   // rows are 16-byte aligned
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = o[4 * j] | (o[4 * j + 1] << 8) | (o[4 * j + 2] << 16) | (o[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int x = 4 * g + p;
      if (x >= it.out0 && x < xend) {
        drow[3 * x] = (uint8_t)o[3 * p];
        drow[3 * x + 1] = (uint8_t)o[3 * p + 1];
        drow[3 * x + 2] = (uint8_t)o[3 * p + 2];
      }
    }
  }
}

__device__ __forceinline__ void rs_vertical(const RsItem& it, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                            const int* __restrict__ coefs, const int* __restrict__ bounds, long u) {
  const int b0 = 3 * it.oth0, b1 = 3 * (it.oth0 + it.noth);       // the window's bytes of a row
  const int d0 = b0 >> 2, nd = ((b1 + 3) >> 2) - d0;
  if (u >= (long)it.nout * nd) return;
  const int i = (int)(u / nd), d = d0 + (int)(u % nd);
  const int first = bounds[2 * (it.bounds_off + i)], taps = min(bounds[2 * (it.bounds_off + i) + 1], it.ksize);
  const int* k = coefs + it.coef_off + (long)i * it.ksize;
  const uint8_t* scol = src + it.src_off + 4 * (long)d;
  int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF, a3 = RS_HALF;
  for (int t = 0; t < taps; ++t) {
    const uint32_t v = *(const uint32_t*)(scol + (long)rs_clamp(first + t, it.src_extent) * it.src_pitch);
    const int kt = k[t];
    a0 += (int)(v & 255u) * kt;
    a1 += (int)((v >> 8) & 255u) * kt;
    a2 += (int)((v >> 16) & 255u) * kt;
    a3 += (int)(v >> 24) * kt;
  }
  const uint32_t o0 = rs_clip(a0), o1 = rs_clip(a1), o2 = rs_clip(a2), o3 = rs_clip(a3);
  uint8_t* dp = dst + it.dst_off + (long)(it.out0 + i) * it.dst_pitch + 4 * (long)d;
  if (4 * d >= b0 && 4 * d + 4 <= b1) {
    *(uint32_t*)dp = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
  } else {
    const uint32_t o[4] = {o0, o1, o2, o3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * d + j >= b0 && 4 * d + j < b1) dp[j] = (uint8_t)o[j];
  }
}

__device__ __forceinline__ void rs_vertical_planar(const RsItem& it, const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                   const int* __restrict__ coefs, const int* __restrict__ bounds, long u) {
  const int ng = it.noth >> 2;                                     // noth % 4 == 0 (checked by the host planner)
  if (u >= (long)it.nout * ng) return;
  const int i = (int)(u / ng), g = (int)(u % ng);
  const int first = bounds[2 * (it.bounds_off + i)], taps = min(bounds[2 * (it.bounds_off + i) + 1], it.ksize);
  const int* k = coefs + it.coef_off + (long)i * it.ksize;
  const int byte0 = 3 * (it.oth0 + 4 * g), sh = 8 * (byte0 & 3);   // 12 bytes from byte0: within 3 * width <= pitch
  const uint8_t* scol = src + it.src_off + (byte0 & ~3);
  int acc[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = RS_HALF;
  for (int t = 0; t < taps; ++t) {
    const uint32_t* s = (const uint32_t*)(scol + (long)rs_clamp(first + t, it.src_extent) * it.src_pitch);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2], w3 = sh ? s[3] : 0u;   // sh != 0: the 4th dword still holds wanted bytes
    const uint64_t p01 = ((uint64_t)w1 << 32) | w0, p12 = ((uint64_t)w2 << 32) | w1, p23 = ((uint64_t)w3 << 32) | w2;
    const uint32_t v[3] = {(uint32_t)(p01 >> sh), (uint32_t)(p12 >> sh), (uint32_t)(p23 >> sh)};
    const int kt = k[t];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] += (int)((v[j >> 2] >> (8 * (j & 3))) & 255u) * kt;
  }
  uint8_t* dp = out + it.dst_off + (long)i * it.dst_pitch + 4 * g;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *(uint32_t*)(dp + (long)c * it.plane) =
        rs_clip(acc[c]) | (rs_clip(acc[3 + c]) << 8) | (rs_clip(acc[6 + c]) << 16) | (rs_clip(acc[9 + c]) << 24);
}

__global__ __launch_bounds__(RS_TILE) void resample_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              uint8_t* __restrict__ out, const RsItem* __restrict__ items,
                                                              const int* __restrict__ prefix, int n_items,
                                                              const int* __restrict__ coefs, const int* __restrict__ bounds) {
  const int tile = blockIdx.x;
  int lo = 0, hi = n_items;                  // the item with prefix[lo] <= tile < prefix[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= tile) lo = mid; else hi = mid;
  }
  if (tile < prefix[lo] || tile >= prefix[lo + 1]) return;
  const RsItem it = items[lo];
  const long u = (long)(tile - prefix[lo]) * RS_TILE + threadIdx.x;
  if (it.kind == 0) {
    if (dst) rs_horizontal(it, src, dst, coefs, bounds, u);
  } else if (it.kind == 1) {
    if (dst) rs_vertical(it, src, dst, coefs, bounds, u);
  } else if (it.kind == 2) {
    if (out) rs_vertical_planar(it, src, out, coefs, bounds, u);
  }
}

}  // namespace

extern "C" int reed_resample_u8(const uint8_t* src, uint8_t* dst, uint8_t* out, const void* items, const int32_t* tile_prefix,
                                int n_items, int total_tiles, const int32_t* coefs, const int32_t* bounds, void* stream) {
  REED_CHECK_ARG(n_items > 0 && total_tiles > 0, "resample_u8: n_items=%d total_tiles=%d must be positive", n_items, total_tiles);
  REED_CHECK_ARG(src && items && tile_prefix && coefs && bounds, "resample_u8: null source or table");
  REED_CHECK_ARG(dst || out, "resample_u8: neither a scratch destination nor an output");
  REED_CHECK_ARG(((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0 && ((uintptr_t)out % 4) == 0 &&
                     ((uintptr_t)items % 16) == 0 && ((uintptr_t)tile_prefix % 4) == 0 && ((uintptr_t)coefs % 4) == 0 &&
                     ((uintptr_t)bounds % 4) == 0,
                 "resample_u8: src, dst and items must be 16-byte aligned, out and the int32 tables 4-byte");
  REED_KLAUNCH(resample_u8_kernel, dim3(total_tiles), dim3(RS_TILE), 0, (hipStream_t)stream, src, dst, out, (const RsItem*)items,
               tile_prefix, n_items, coefs, bounds);
  REED_LAUNCH_CHECK();
  return REED_OK;
}
