// Lane map and scale operands of v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3), measured with one wave on exact data.
//   hipcc -O2 --offload-arch=gfx950 tools/micro/mx_mfma_probe.hip -o tools/micro/mx_mfma_probe && tools/micro/mx_mfma_probe
// 1. k pairing: A = a single 1.0 in (lane 16 ga, byte ja); B = f(lane group, byte) in every column: D[0][0] names the B element
//    the hardware multiplies it with.
// 2. scale source: A = ones in ONE half register (16 bytes) of ONE lane, B = ones everywhere, every lane's scale_a register a
//    different power of two in each of its four bytes: D names the lane and, per op_sel, the byte whose scale was applied.  The
//    same for B.
// 3. accumulation unit: one large and K - 1 tiny exact terms against fp64 (what the tests' u' has to cover).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// a, b: [64 lanes][32 bytes]; sa, sb: [64] scale registers; out: [64 lanes][4]
template <int OA, int OB>
__global__ void one_mfma(const unsigned char* a, const unsigned char* b, const int* sa, const int* sb, float* out) {
  const int lane = threadIdx.x;
  const i32x8 av = *(const i32x8*)(a + lane * 32), bv = *(const i32x8*)(b + lane * 32);
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 0, 0, OA, sa[lane], OB, sb[lane]);
  *(f32x4*)(out + lane * 4) = c;
}

static unsigned char *dA, *dB;
static int *dSa, *dSb;
static float* dOut;
static unsigned char hA[64 * 32], hB[64 * 32];
static int hSa[64], hSb[64];
static float hOut[256];

template <int OA, int OB>
static int run() {
  CK(hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice));
  CK(hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice));
  CK(hipMemcpy(dSa, hSa, sizeof(hSa), hipMemcpyHostToDevice));
  CK(hipMemcpy(dSb, hSb, sizeof(hSb), hipMemcpyHostToDevice));
  hipLaunchKernelGGL((one_mfma<OA, OB>), dim3(1), dim3(64), 0, 0, dA, dB, dSa, dSb, dOut);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(hOut, dOut, sizeof(hOut), hipMemcpyDeviceToHost));
  return 0;
}
// D[row][col] in the 16x16 C/D map: lane = col + 16 (row / 4), register row % 4
static float D(int row, int col) { return hOut[(col + 16 * (row / 4)) * 4 + row % 4]; }
static unsigned char code_of_int(int v) {   // e4m3 code of an integer 0..16
  if (v == 0) return 0;
  int e = 0;
  while ((v >> (e + 1)) != 0) ++e;
  return (unsigned char)(((e + 7) << 3) | (((v << 3) >> e) & 7));
}

int main() {
  CK(hipMalloc(&dA, sizeof(hA)));
  CK(hipMalloc(&dB, sizeof(hB)));
  CK(hipMalloc(&dSa, sizeof(hSa)));
  CK(hipMalloc(&dSb, sizeof(hSb)));
  CK(hipMalloc(&dOut, sizeof(hOut)));
  for (int l = 0; l < 64; ++l) hSa[l] = hSb[l] = 127;
  // ---- 1. k pairing -------------------------------------------------------------------------------------------------
  printf("1. k pairing: A (lane group ga, byte ja) x B (lane group gb, byte jb); rows ga, 32 entries 'gb:jb'\n");
  int natural = 1;
  for (int ga = 0; ga < 4; ++ga) {
    printf("  ga=%d:", ga);
    for (int ja = 0; ja < 32; ++ja) {
      int id[2];
      for (int pass = 0; pass < 2; ++pass) {
        memset(hA, 0, sizeof(hA));
        hA[(16 * ga) * 32 + ja] = 0x38;   // 1.0 in row 0
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 32; ++j) hB[l * 32 + j] = code_of_int(pass == 0 ? (l >> 4) * 4 + j / 8 + 1 : j % 8 + 1);
        if (run<0, 0>()) return 1;
        id[pass] = (int)D(0, 0);
      }
      const int gb = (id[0] - 1) / 4, jb = ((id[0] - 1) % 4) * 8 + id[1] - 1;
      printf(" %d:%d", gb, jb);
      natural &= gb == ga && jb == ja;
    }
    printf("\n");
  }
  printf("  => %s\n", natural ? "equal lane group and byte pair up (operands loaded alike sum over equal k)" : "NOT the identity pairing");
  // ---- 2. scale source ----------------------------------------------------------------------------------------------
  // data = ones in ONE lane's bytes 0..15 (half 0) or 16..31 (half 1): D = 16 x the one scale that was applied (else "mixed").
  // Two runs name the lane (l % 16, then l / 16) and the byte: byte s of lane l holds 127 + (l % 16) + 16 s - 32, then 127 + l / 16 + 4 s - 8.
  for (int which = 0; which < 2; ++which) {
    printf("2%c. scale_%c: data of (lane L0, half) -> the scale register lane and byte applied to it, per op_sel\n", which ? 'b' : 'a', which ? 'b' : 'a');
    for (int sel = 0; sel < 4; ++sel) {
      int ok = 1, src_group[4][2], src_byte = -1;
      for (int L0 = 0; L0 < 64; ++L0)
        for (int half = 0; half < 2; ++half) {
          unsigned char* data = which ? hB : hA;
          unsigned char* other = which ? hA : hB;
          int* sc = which ? hSb : hSa;
          int* so = which ? hSa : hSb;
          memset(data, 0, 64 * 32);
          memset(data + L0 * 32 + 16 * half, 0x38, 16);
          memset(other, 0x38, 64 * 32);
          int e[2];
          for (int pass = 0; pass < 2; ++pass) {
            for (int l = 0; l < 64; ++l) {
              so[l] = 127;
              sc[l] = 0;
              for (int s = 0; s < 4; ++s) sc[l] |= (pass == 0 ? 127 + (l % 16) + 16 * s - 32 : 127 + (l / 16) + 4 * s - 8) << (8 * s);
            }
            if (sel == 0 ? run<0, 0>() : sel == 1 ? (which ? run<0, 1>() : run<1, 0>()) : sel == 2 ? (which ? run<0, 2>() : run<2, 0>()) : (which ? run<0, 3>() : run<3, 0>())) return 1;
            const float v = (which ? D(0, L0 & 15) : D(L0 & 15, 0)) / 16.f;
            e[pass] = (int)lrintf(log2f(v));
            if (ldexpf(1.f, e[pass]) != v) { printf("  op_sel=%d L0=%d half=%d: mixed scales (D / 16 = %g)\n", sel, L0, half, v); ok = 0; }
            e[pass] += pass == 0 ? 32 : 8;
          }
          const int lane = e[0] % 16 + 16 * (e[1] % 4), byte = e[0] / 16;
          if (byte != e[1] / 4 || (lane & 15) != (L0 & 15)) { printf("  op_sel=%d L0=%d half=%d: lane %d byte %d / %d ?\n", sel, L0, half, lane, byte, e[1] / 4); ok = 0; }
          if ((L0 & 15) == 0) src_group[L0 >> 4][half] = lane >> 4;
          else if (src_group[L0 >> 4][half] != lane >> 4) { printf("  op_sel=%d L0=%d half=%d: lane group %d differs from row 0's\n", sel, L0, half, lane >> 4); ok = 0; }
          if (src_byte < 0) src_byte = byte;
          else if (src_byte != byte) ok = 0;
        }
      printf("  op_sel=%d: byte %d of the register of lane (same row / column) + 16 x:", sel, src_byte);
      for (int g = 0; g < 4; ++g) printf("  data group %d: bytes 0-15 <- %d, bytes 16-31 <- %d;", g, src_group[g][0], src_group[g][1]);
      printf(" %s\n", ok ? "consistent over all 16 rows" : "INCONSISTENT");
    }
  }
  // ---- 3. accumulation unit -----------------------------------------------------------------------------------------
  // big = 256 * 256 = 2^16 (one term), tiny = 2^-6 * 2^-6 = 2^-12 (127 terms): exact sum 2^16 + 127 * 2^-12; fp32 ulp at 2^16 is 2^-7.
  for (int l = 0; l < 64; ++l) hSa[l] = hSb[l] = 127;
  memset(hA, 0x08, sizeof(hA));   // 2^-6
  memset(hB, 0x08, sizeof(hB));
  hA[0] = hB[0] = 0x78;           // 256 (lane 0 = row / column 0, k-group 0, byte 0)
  if (run<0, 0>()) return 1;
  const double exact = 65536.0 + 127.0 / 4096.0, tiny_only = 128.0 / 4096.0;
  printf("3. accumulation: D[0][0] = %.9g (exact %.9g, error %.3g = %.3f ulp of fp32 at 2^16); D[1][1] = %.9g (exact %.9g)\n", D(0, 0), exact,
         D(0, 0) - exact, (D(0, 0) - exact) / 0.0078125, D(1, 1), tiny_only);
  // the same with tiny terms of 2^-8 each (127 of them = 0.496 < half an ulp of 2^16 in sum, each far below it)
  memset(hA, 0x18, sizeof(hA));   // 2^-4
  memset(hB, 0x18, sizeof(hB));
  hA[0] = hB[0] = 0x78;
  if (run<0, 0>()) return 1;
  const double exact2 = 65536.0 + 127.0 / 256.0;
  printf("   D[0][0] = %.9g (exact %.9g, error %.3g = %.3f ulp)\n", D(0, 0), exact2, D(0, 0) - exact2, (D(0, 0) - exact2) / 0.0078125);
  return 0;
}
