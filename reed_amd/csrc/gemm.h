// Internal GEMM interface (see gemm.hip). Public C ABI is in include/reed_hip.h.
#pragma once
#include <type_traits>
#include <utility>

#include "common.hpp"

enum { LAY_NT = 0, LAY_NN = 1, LAY_TN = 2,
       LAY_TN_TALL = 3, LAY_TN_WIDE = 4 };   // TN on gemm_tn.hip's 256x128 / 128x256 tile (fp32 epilogue only)
enum {
  EPI_BF16 = 0,       // C bf16 = bf16(acc [+bias])
  EPI_GELU = 1,       // C bf16 = pre = bf16(acc+bias) (optional), C2 bf16 = gelu_tanh(pre)
  EPI_SILU = 2,       // same with SiLU
  EPI_GATE_RES = 3,   // C f32 = R f32 + bf16(gate[m/rows_per_gate] * bf16(acc+bias)); C2 bf16 = y (optional)
  EPI_DGELU = 4,      // C bf16 = bf16(bf16(acc) * gelu_tanh'(R bf16))
  EPI_DSILU = 5,      // C bf16 = bf16(bf16(acc) * silu'(R bf16))
  EPI_F32 = 6,        // C f32 (+)= acc [+bias]; split-K writes slabs C + z*slab_stride
  EPI_ADDF32_RB = 7,  // C f32 += float(bf16(acc))
  EPI_ATOMIC_F32 = 8, // atomicAdd(C f32, acc)   (split-K into a pre-zeroed / accumulating buffer)
  // inference-only epilogues of the frozen CLIP image encoder (bf16 residual stream):
  EPI_QGELU = 9,      // C2 bf16 = QuickGELU(pre) = bf16(pre * bf16(sigmoid(bf16(1.702 pre)))), pre = bf16(acc+bias) (C optional)
  EPI_RES_BF16 = 10,  // C bf16 = bf16(bf16(acc+bias) + R bf16)
  EPI_LS_RES = 12,    // C f32 = R f32 + gamma f32[n] * float(bf16(acc+bias)): LayerScale + fp32 residual (DINOv2 blocks); `gate`
                      //   points at the fp32 gamma vector; NT only
  EPI_BF16_DOT = 13,  // C bf16 = bf16(acc [+ bias]) and dpart f32 [N / hd, S, M] (C2) = per row and head of hd = rows_per_gate columns
                      //   (64: S = 1, 72: S = 2) the partial dot products of the stored row with R bf16 [M, N]: slot s of head h is the
                      //   part inside the (s + 1)-th 64-column strip the head touches.  NN, 256^2 four-wave kernel only: the attention
                      //   backward's delta = rowsum(dO * O) formed where dO is produced (reed_attention_bwd_dp adds the slots)
  EPI_GELU_ERF = 11,  // C2 bf16 = GELU(erf)(pre): nn.GELU() of the timm / I-JEPA towers' Mlp (its own instantiation since round 4;
                      //   the fp32-operand build folds it into EPI_QGELU with GemmArgs::act_variant = 1)
  // Round 5: the activation's DERIVATIVE is formed where the activation is (the forward epilogue holds sigmoid(2u) already) and
  // saved in the array the pre-activation used to occupy — the pre-activation of fc1 / the projector layers was kept for the
  // backward's dGELU / dSiLU epilogue only — so that epilogue becomes one multiply per element (EPI_MUL):
  EPI_GELU_G = 14,    // C bf16 = bf16(gelu_tanh'(pre)) (optional), C2 bf16 = gelu_tanh(pre), pre = bf16(acc+bias)
  EPI_SILU_G = 15,    // same with SiLU
  EPI_MUL = 16,       // C bf16 = bf16(bf16(acc) * R bf16)
  // the SwiGLU feed-forward of DINOv2 ViT-g (SwiGLUFFNFused: w3(silu(x1) * x2), x1 | x2 = w12(x)), inference only:
  EPI_SWIGLU = 17     // C bf16 [M, N / 2] = bf16(bf16(silu(x1)) * x2), x12 = bf16(acc+bias) never stored.  NT only, on a weight (and
                      //   bias) whose rows are interleaved in groups of SWIGLU_GROUP: packed rows 2 g k .. 2 g k + g - 1 are the x1 rows
                      //   g k .. g k + g - 1, the next g their x2 partners (ops.swiglu_pack); output column g k + j
};
constexpr int SWIGLU_GROUP = 8;   // = the 8 columns a lane of tile_epilogue owns: the partner sits in the neighbouring lane

// Sets of epilogues as bit masks over the EPI_* values: every "which epilogues" question has its one answer here, for the
// selection (gemm_plan.cpp) and for the launchers alike.
template <class... E>
constexpr unsigned epi_set(E... e) { return ((1u << e) | ...); }
constexpr bool epi_in(unsigned set, int epi) { return epi >= 0 && epi < 32 && ((set >> epi) & 1u) != 0; }
// -- per kernel and layout: the epilogues the kernel is INSTANTIATED for.  Each launcher hands its set to epi_dispatch (below), so
// a kernel exists for exactly the members; the selection reads the same constants, so it cannot plan a launch that is not built.
// the bf16-output epilogues, all built for the 256x144 tile (NT and NN)
constexpr unsigned EPIS_144 = epi_set(EPI_BF16, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_DGELU, EPI_DSILU, EPI_QGELU, EPI_GELU_ERF,
                                      EPI_RES_BF16, EPI_GELU_G, EPI_SILU_G, EPI_MUL);
// the 256x288 tile: the epilogues of the two 4608-wide GEMMs it was built for (fc1 forward, fc2 input gradient)
constexpr unsigned EPIS_288 = epi_set(EPI_BF16, EPI_GELU, EPI_GELU_G, EPI_DGELU, EPI_MUL);
// the skinny tiles: the row-free bf16 / fp32-residual epilogues of a frozen tower's forward (NT).  Against EPIS_144: + LS_RES,
// SWIGLU (tower epilogues); - DGELU, DSILU, MUL: as found (a forward has none of them)
constexpr unsigned EPIS_SKINNY = epi_set(EPI_BF16, EPI_GELU, EPI_SILU, EPI_QGELU, EPI_GELU_ERF, EPI_GELU_G, EPI_SILU_G, EPI_RES_BF16,
                                         EPI_LS_RES, EPI_GATE_RES, EPI_SWIGLU);
// the four-wave 256^2 kernel.  QuickGELU / exact-GELU are not eligible and no longer built for it: they stay on the 8-wave
// kernel — their VALU work (erff, two roundings per element) needs two waves per SIMD to hide its own latency; measured 0.93 vs
// 0.64 ms on the ViT-L fc1 shape.  DSILU is missing from the NT set as found.
constexpr unsigned EPIS_256W_NT = epi_set(EPI_BF16, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_GELU_G, EPI_SILU_G, EPI_RES_BF16, EPI_LS_RES,
                                          EPI_BF16_DOT, EPI_DGELU, EPI_MUL, EPI_SWIGLU);
// input gradients on the weights as they are: the backward's epilogues only
constexpr unsigned EPIS_256W_NN = epi_set(EPI_BF16, EPI_BF16_DOT, EPI_DGELU, EPI_DSILU, EPI_MUL);
constexpr unsigned epis_256w(int layout) { return layout == LAY_NT ? EPIS_256W_NT : EPIS_256W_NN; }
// epilogue 13 is asked for as the plain store's kernel plus the dot (reed_gemm_plan_shape): wherever one is built, both are
static_assert(epi_in(EPIS_256W_NT, EPI_BF16) == epi_in(EPIS_256W_NT, EPI_BF16_DOT) &&
              epi_in(EPIS_256W_NN, EPI_BF16) == epi_in(EPIS_256W_NN, EPI_BF16_DOT), "four-wave 256^2: epilogues 0 and 13 go together");
// the 256^2 kernels' re-dealt ragged last column tile (<= 128 live columns) counts ~0.6 of a tile in the cost model for these:
// the bf16-output epilogues = EPIS_144, + LS_RES, SWIGLU as found
constexpr unsigned EPIS_RAGGED_COL = EPIS_144 | epi_set(EPI_LS_RES, EPI_SWIGLU);
// the 128^2 and eight-wave 256^2 kernels build every epilogue but 13; LS_RES and SWIGLU for NT only, and the eight-wave kernel
// on TN the fp32 outputs only (weight gradients)
constexpr unsigned EPIS_NT_ONLY = epi_set(EPI_LS_RES, EPI_SWIGLU);
// (reed_gemm refuses them elsewhere, with split-K, and SWIGLU for N not a multiple of 128, before any selection: api.cpp)
constexpr bool epi_layout_ok(int layout, int epi, int N, int split_k) {
  return !epi_in(EPIS_NT_ONLY, epi) || (layout == LAY_NT && split_k <= 1 && (epi != EPI_SWIGLU || N % 128 == 0));
}
constexpr int EPI_COUNT = 18;   // one past the largest EPI_* value
constexpr unsigned EPIS_128_NT = (1u << EPI_COUNT) - 1u - epi_set(EPI_BF16_DOT);
constexpr unsigned EPIS_256X8_TN = epi_set(EPI_F32, EPI_ADDF32_RB, EPI_ATOMIC_F32);
constexpr unsigned epis_128(int layout) { return layout == LAY_NT ? EPIS_128_NT : EPIS_128_NT & ~EPIS_NT_ONLY; }
constexpr unsigned epis_256x8(int layout) { return layout == LAY_TN ? EPIS_256X8_TN : epis_128(layout); }
// the MX-fp8 block GEMM (gemm_mxfp8.hip): the three epilogues of the inference forward's block linears
constexpr unsigned EPIS_MXFP8 = epi_set(EPI_BF16, EPI_GELU, EPI_GATE_RES);
// the fp32-operand build's one kernel (gemm_f32.hip; its epilogue is a run-time switch): every layout.  GELU_ERF arrives as QGELU
// with GemmArgs::act_variant = 1, SWIGLU is not part of that build
constexpr unsigned EPIS_F32 = epi_set(EPI_BF16, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_DGELU, EPI_DSILU, EPI_F32, EPI_ADDF32_RB,
                                      EPI_ATOMIC_F32, EPI_QGELU, EPI_RES_BF16, EPI_LS_RES, EPI_GELU_G, EPI_SILU_G, EPI_MUL);
// the 128^2 kernel is where the selection ends when nothing else applies: what any other kernel builds on a layout, it builds too
// (13 aside: a shape whose plain store lands there is answered with REED_ERR_UNSUPPORTED), and so does the fp32-operand build
static_assert(((EPIS_144 | EPIS_288 | EPIS_SKINNY | EPIS_256W_NT) & ~(EPIS_128_NT | epi_set(EPI_BF16_DOT))) == 0 &&
                  ((EPIS_144 | EPIS_256W_NN) & ~(epis_128(LAY_NN) | epi_set(EPI_BF16_DOT))) == 0 &&
                  (EPIS_256X8_TN & ~epis_128(LAY_TN)) == 0 && (EPIS_F32 & ~EPIS_128_NT) == 0,
              "a kernel builds an epilogue that the 128^2 kernel lacks on that layout");
// the sets the cost model and the splits read describe epilogues that exist
static_assert(((EPIS_RAGGED_COL | EPIS_NT_ONLY) & ~EPIS_128_NT) == 0, "the cost model names an epilogue that no kernel builds");

// -- semantic
// the row index carries no meaning (rows may go out as two launches): EPIS_RAGGED_COL - GATE_RES (the gate is per sample =
// per block of rows); the head-dot slots of epilogue 13 and the fp32 outputs are left alone
constexpr unsigned EPIS_ROWS_FREE = EPIS_RAGGED_COL & ~epi_set(EPI_GATE_RES);
// the column index carries no meaning beyond the offsets the launcher applies to Q / C / C2 / R / bias / gate (columns may go
// out as two launches): = EPIS_144.  Against EPIS_ROWS_FREE: + GATE_RES (its gate is per row block, not per column); - LS_RES,
// SWIGLU: as found (the launcher offsets `gate` as 16-bit elements, LS_RES's is an fp32 vector; SWIGLU's output has N / 2 columns)
constexpr unsigned EPIS_COLS_FREE = EPIS_144;
// bytes per element of C and of R: the two fp32-residual epilogues have fp32 outputs; the splits take bf16 for everything else
// in their sets
constexpr int epi_out_bytes(int epi) { return epi == EPI_GATE_RES || epi == EPI_LS_RES ? 4 : 2; }

// Launch-side reading of a set: calls f(std::integral_constant<int, E>{}) for the one member E of SET equal to `epi` and returns
// true; for any other value calls nothing and returns false.  f's body is instantiated for the members only, so a launcher that
// dispatches over its set builds a kernel for exactly that set.  (A chain of at most EPI_COUNT compares on the host.)
template <unsigned SET, int E, class F>
bool epi_dispatch_one(int epi, F& f) {
  if constexpr (epi_in(SET, E)) {
    if (epi == E) {
      f(std::integral_constant<int, E>{});
      return true;
    }
  }
  return false;
}
template <unsigned SET, class F, int... E>
bool epi_dispatch_seq(int epi, F& f, std::integer_sequence<int, E...>) { return (epi_dispatch_one<SET, E>(epi, f) || ...); }
template <unsigned SET, class F>
bool epi_dispatch(int epi, F&& f) {
  static_assert((SET >> EPI_COUNT) == 0, "epi_dispatch: the set has a member that is no epilogue");
  return epi_dispatch_seq<SET>(epi, f, std::make_integer_sequence<int, EPI_COUNT>{});
}

struct GemmArgs {
  const bf16* P;
  const bf16* Q;
  long ldp, ldq;
  int M, N, K;
  void* C;
  long ldc;
  void* C2;
  long ldc2;
  const void* R;
  long ldr;
  const bf16* bias;
  const bf16* gate;
  long ldgate;
  int rows_per_gate;
  float* dbias;  // TN only: dbias[m] (+)= sum_k P[k][m]
  int accumulate;
  int ksplit_len;
  long slab_stride;
  int act_variant;   // fp32-operand build only: EPI_QGELU as 0 = QuickGELU (CLIP), 1 = GELU(erf) (timm / I-JEPA Mlp, nn.GELU)
  int tile_gm;   // gemm256: tile rows per XCD-local group of the workgroup -> tile map (set by launch256)
};

int reed_gemm_launch(int layout, int epi, GemmArgs a, int splits, hipStream_t stream);
