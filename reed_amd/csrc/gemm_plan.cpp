// Kernel selection for reed_gemm: the knobs, the round-count cost models, the persistent-form decision and the plan itself.
// Host arithmetic only — no kernel, no launch, no pointer; the one HIP call is the device-property query of reed_num_cus.
// Compiled into every build of the library (the fp32-operand build uses the knobs; its one kernel needs no selection).
//
// Time is counted in units of "one CU, one 128^2 tile".  The models were fitted to A/B timing at the SiT-XL/2 shapes for b = 32 ..
// 256 per GPU (tools/stagger_sweep.py, tools/tile_ab.py): a kernel's cost is its rounds on `ncu` CUs times its
// tile's area over its rate per flop relative to the 128^2 kernel.
#include "gemm_plan.h"

#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

// ---- the knobs -------------------------------------------------------------------------------------------------------------
static int g_force_tile = 0;
extern "C" int reed_gemm_force_tile(int tile) { g_force_tile = tile; return 0; }
int reed_gemm_forced_tile() { return g_force_tile; }

// fp32-operand build: 0 = exact fp32 products (v_mfma_f32_32x32x2_f32, the default), 1 = each fp32 product as three bf16 MFMA
// products (csrc/gemm_f32.hip: the reference's --allow-tf32).  The 16-bit builds have nothing to switch.
static int g_f32_split = 0;
extern "C" int reed_gemm_f32_split(int on) {
#if defined(REED_FP32)
  g_f32_split = on ? 1 : 0;
  return REED_OK;
#else
  if (on) {
    reed_set_error("reed_gemm_f32_split: this library's operands are 16-bit already (the mode belongs to the fp32-operand build)");
    return REED_ERR_UNSUPPORTED;
  }
  return REED_OK;
#endif
}
int reed_gemm_f32_split_on() { return g_f32_split; }

// CUs the tile heuristics plan for = the device's count minus a reserve (reed_set_cu_reserve).  While a
// gradient bucket is in flight RCCL's channels hold CUs, and a grid planned as exactly one round of the 256 CUs — the 256x144
// tile at b = 32 per GPU, the grouped weight gradients' 512 slots — turns into two rounds on what is left.  The data-parallel
// train step measures a few reserves during its first steps and keeps the fastest (reed_amd/trainer.py).
static int g_cu_reserve = 0;
extern "C" int reed_set_cu_reserve(int n) { g_cu_reserve = n > 0 ? n : 0; return 0; }
int reed_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n - g_cu_reserve > 32 ? n - g_cu_reserve : 32;
}
extern "C" int reed_planning_cus(void) { return reed_num_cus(); }

// Collectives run beside the GEMMs (a data-parallel step): kernels that need a whole CU per workgroup for their whole run
// (the persistent form of gemm256w.hip) lose more than they gain when RCCL's channels hold some CUs — the workgroups that
// find no CU start when another finishes its entire list.  The one-shot kernels degrade gracefully; they are used then.
static int g_concurrent_comm = 0;
extern "C" int reed_set_concurrent_comm(int on) { g_concurrent_comm = on ? 1 : 0; return 0; }
int reed_concurrent_comm() { return g_concurrent_comm; }

static bool env_on(const char* name) { return getenv(name) && atoi(getenv(name)) != 0; }
// read once, at load.  REED_GEMM_COLSPLIT=1: the column split (measured equal in the b = 32 step: off by default);
// REED_GEMM288=1: the heuristic may take the 256x288 kernel (measured equal to the 256x144 kernel: off by default)
static const bool g_colsplit = env_on("REED_GEMM_COLSPLIT"), g_use288 = env_on("REED_GEMM288");

GemmKnobs reed_gemm_knobs() { return GemmKnobs{reed_num_cus(), g_force_tile, g_colsplit, g_use288, g_concurrent_comm != 0}; }

namespace {

long cdivl(long a, long b) { return (a + b - 1) / b; }
bool nt_or_nn(int layout) { return layout == LAY_NT || layout == LAY_NN; }

// ---- eligibility: the shapes each kernel can take --------------------------------------------------------------------------
// 256x144: NT / NN, bf16-output epilogue, N a multiple of 144, no split-K
bool eligible144(const GemmShape& s) {
  return nt_or_nn(s.layout) && epi_in(EPIS_144, s.epi) && s.splits <= 1 && s.N % 144 == 0 && s.K % 64 == 0 && s.K >= 64;
}
// 256x288: NT, N a multiple of 288, K of 64 and >= 4 k-steps of 32 (the prologue stages three), no split-K
bool eligible288(const GemmShape& s) {
  return s.layout == LAY_NT && epi_in(EPIS_288, s.epi) && s.splits <= 1 && s.N % 288 == 0 && s.K % 64 == 0 && s.K >= 128;
}
// four-wave 256^2
bool eligible256w(const GemmShape& s) {
  return nt_or_nn(s.layout) && s.splits <= 1 && s.K % 64 == 0 && s.K >= 128 && s.N % 128 == 0 &&
         epi_in(epis_256w(s.layout), s.epi);
}
// skinny: NT, K a multiple of 64, N of 64, no split-K
bool eligible_skinny(const GemmShape& s) {
  return s.layout == LAY_NT && epi_in(EPIS_SKINNY, s.epi) && s.splits <= 1 && s.K % 64 == 0 && s.K >= 64 && s.N % 64 == 0 && s.M >= 1 &&
         cdivl(s.M, 16) * (s.N / 64) < (1l << 30);
}

// ---- cost: one function per tile shape --------------------------------------------------------------------------------------
// 128^2: two tiles per CU in flight, which quantises better when the 256^2 grid is only one or two rounds
double cost128(int M, int N, int ncu) { return (double)cdivl(cdivl(M, 128) * cdivl(N, 128), 2L * ncu) * 2.0; }

// 256^2 (both kernels): one tile per CU at a time, ~1.18x faster per flop than 128^2 (half the global->LDS bytes, deeper pipeline).
// A ragged last column tile (<= 128 live columns) runs the re-dealt two-phase body: ~0.6 of a full tile, and such tiles fill the
// tail of the last round (A/B at b = 128: fc2 forward 0.407 -> 0.362 ms, fc1 / qkv dgrads 0.385 -> 0.322 / 0.285 -> 0.237 ms).
// How the rounds of a grid with such tiles are counted differs by call site:
enum RaggedRounds {
  RAGGED_HALF_ROUNDS,           // in halves always: prefer256 (256^2 against 128^2), for the epilogues of EPIS_RAGGED_COL
  RAGGED_HALF_FROM_TWO_ROUNDS,  // in halves from two rounds of work on, whole rounds below (at 1.25 rounds — b = 64, N = 1152 —
                                //   the second, quarter-full round costs a full tile time): prefer144 and prefer288
  RAGGED_WHOLE_ROUNDS           // ragged tiles as full ones: the column split (its N is a multiple of 256 anyway), and
                                //   prefer256 for the epilogues outside EPIS_RAGGED_COL
};
double cost256(int M, int N, int ncu, RaggedRounds ragged) {
  const long tm = cdivl(M, 256), tn = cdivl(N, 256);
  double rounds = (double)cdivl(tm * tn, ncu);
  if (ragged != RAGGED_WHOLE_ROUNDS && (N % 256) != 0 && (N % 256) <= 128) {
    const double w = (double)tm * (tn - 1) + 0.6 * tm;
    if (ragged == RAGGED_HALF_ROUNDS || w >= 2.0 * ncu) rounds = ceil(2.0 * w / ncu) / 2.0;
  }
  return rounds * 4.0 / 1.18;
}

// 256x144: 0.5625 of a 256^2 tile; with the loader waves its main loop runs at the chip's dense-MFMA ceiling when all CUs are
// busy, but per round it exposes the same epilogue as the 256^2 kernel on 0.56 of the work, so over the block shapes it is worth
// ~0.92 of the 128^2 kernel's unit per flop (a sweep of the threshold inside the step, b = 32 .. 256, round 2).  N % 144 == 0.
double cost144(int M, int N, int ncu) { return (double)cdivl(cdivl(M, 256) * (N / 144), ncu) * 2.25 / 0.92; }

// 256x288: 4.5 of area.  MEASURED equal to the 256x144 kernel (profiles/r6_gemm288.txt), so the heuristic takes it only under
// REED_GEMM288=1; the rate is a build-time knob for that A/B.  N % 288 == 0.
#ifndef REED_GEMM288_ETA
#define REED_GEMM288_ETA 1.10
#endif
double cost288(int M, int N, int ncu) { return (double)cdivl(cdivl(M, 256) * (N / 288), ncu) * 4.5 / REED_GEMM288_ETA; }

// Outcome of prefer144 on SiT-XL/2: the five 1152-wide outputs (proj / fc2 forward, dgrads of qkv / proj / fc1) at b <= 64 per
// GPU and the two 4608-wide ones (fc1 forward, fc2 dgrad) at b = 32; everything else stays on the square tiles.
bool prefer144(const GemmShape& s, int ncu) {
  if (!eligible144(s) || s.K < 256) return false;
  const double c144 = cost144(s.M, s.N, ncu);
  return c144 < cost256(s.M, s.N, ncu, RAGGED_HALF_FROM_TWO_ROUNDS) && c144 < cost128(s.M, s.N, ncu);
}
bool prefer288(const GemmShape& s, int ncu) {
  if (!eligible288(s) || s.K < 256) return false;
  double best = fmin(cost256(s.M, s.N, ncu, RAGGED_HALF_FROM_TWO_ROUNDS), cost128(s.M, s.N, ncu));
  if (s.N % 144 == 0) best = fmin(best, cost144(s.M, s.N, ncu));
  return cost288(s.M, s.N, ncu) < best;
}
// NT forward / NN dgrad.  TN (wgrad) stays on the 128^2 kernel with wave-quantised split-K (ops.plan_wgrad); its 256^2 variant
// is reachable through the forced tile only.
bool prefer256(const GemmShape& s, int ncu) {
  if (s.layout == LAY_TN || s.splits > 1 || s.K < 256) return false;
  const RaggedRounds ragged = epi_in(EPIS_RAGGED_COL, s.epi) ? RAGGED_HALF_ROUNDS : RAGGED_WHOLE_ROUNDS;
  return cost256(s.M, s.N, ncu, ragged) < cost128(s.M, s.N, ncu);
}

// ---- the four-wave 256^2 kernel: tile walk and one-shot / persistent form ---------------------------------------------------
// Tile rows per XCD-local group of the workgroup -> tile map.
// Measured at b = 256 (tools/_ab/gm_w4.sh): the 1152-wide outputs (4.5 column tiles) prefer groups of 2 rows — fc2 forward
// 0.637 -> 0.618 ms, fc1 / qkv dgrads 0.564 -> 0.546 / 0.430 -> 0.417 —, the 3456- / 4608-wide ones groups of 4 (fc1 forward
// 0.684 vs 0.720 with 2).
int w_tile_group_rows(int M, int N) {
#ifdef REED_TILE_GM_ENV   // diagnostic build only (tools/r6/gm_sweep.sh): the tile rows per XCD-local group from the environment
  if (const char* e = getenv("REED_TILE_GM")) return atoi(e) > 0 ? atoi(e) : 4;
#endif
  if (cdivl(M, 256) < 192) return 4;   // b = 128: 1157 (4 everywhere) vs 1151 images/s with the per-shape choice
  const long ntn = cdivl(N, 256);
  return ntn <= 6 ? 2 : ntn >= 16 ? 5 : 4;   // (4608-wide: fc1 forward 0.688 -> 0.675, fc2 dgrad 0.727 -> 0.721 with 5)
}

// Static deal of the persistent form: the heaviest workgroup's load in full-tile units (a ragged tile counts RAG_COST) when
// wpx workgroups per XCD take positions s, s + wpx, ... of their XCD's run.
constexpr double RAG_COST = 0.58;
double w_static_max_load(int ntm, int ntn, bool rag, int GM, int wpx) {
  const int nwg = ntm * ntn, q = nwg >> 3, r = nwg & 7;
  double worst = 0;
  for (int xcd = 0; xcd < 8; ++xcd) {
    const int run0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, runlen = q + (xcd < r ? 1 : 0);
    for (int s = 0; s < wpx && s < runlen; ++s) {
      double load = 0;
      for (int p = s; p < runlen; p += wpx) {
        const int b = run0 + p, per_group = GM * ntn, group = b / per_group, first_m = group * GM;
        const int gs = std::min(ntm - first_m, GM), tn = (b % per_group) / gs;
        load += (rag && tn == ntn - 1) ? RAG_COST : 1.0;
      }
      worst = std::max(worst, load);
    }
  }
  return worst;
}

// The persistent form (one workgroup per CU, the next tile's first K-tiles staged under this tile's epilogue) or the one-shot
// grid.  forced 257: never, 258: wherever the form applies (tests), else never beside a collective and otherwise where the
// static deal is balanced.
bool w_persistent(int M, int N, int K, int GM, const GemmKnobs& k, int forced) {
  const int mode = forced == 257 ? 0 : forced == 258 ? 2 : k.concurrent_comm ? 0 : 1;
  const int nt = (int)cdivl(K, 64), ntm = (int)cdivl(M, 256), ntn = (int)cdivl(N, 256), wpx = k.ncu / 8;
  if (mode == 0 || (nt & 1) || nt < 4 || wpx < 1 || (K % 64) != 0) return false;
  if (mode == 2) return true;
  const bool rag = (N % 256) != 0;
  const double total = (double)ntm * ((ntn - (rag ? 1 : 0)) + (rag ? RAG_COST : 0.0));
  const double ideal = total / (8.0 * wpx);
  if (ideal < 3.0) return false;       // too few tiles per workgroup for the hand-over to matter
  // the verdict per (tile grid, group rows, workgroups per XCD) is remembered: the walk is ~5 k steps on the host
  static thread_local struct { int ntm, ntn, gm, wpx, ok; } memo[8];   // ntn carries the ragged flag in its sign
  static thread_local int memo_n = 0;
  for (int i = 0; i < memo_n; ++i)
    if (memo[i].ntm == ntm && memo[i].ntn == (rag ? -ntn : ntn) && memo[i].gm == GM && memo[i].wpx == wpx) return memo[i].ok != 0;
  const double worst = w_static_max_load(ntm, ntn, rag, GM, wpx);
  // the greedy hand-out of the one-shot kernel ends about half a tile after the balanced time when ragged tiles are mixed in
  const double greedy = ideal + (rag ? 0.45 : 0.0);
  const int ok = worst > greedy + 0.05 ? 0 : 1;
  memo[memo_n % 8] = {ntm, rag ? -ntn : ntn, GM, wpx, ok};
  if (memo_n < 8) ++memo_n;
  return ok != 0;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
int unsupported_dot() {
  reed_set_error("reed_gemm(epilogue 13): this shape runs on a kernel without it (use epilogue 0)");
  return REED_ERR_UNSUPPORTED;
}

// the instantiations of the two kernels that take every layout: gemm.hip's 128^2 and gemm256.hip's eight-wave 256^2
int square_built(const GemmShape& s, bool eight_wave) {
  if (s.layout != LAY_NT && s.layout != LAY_NN && s.layout != LAY_TN) {
    reed_set_error("reed_gemm: unknown layout %d", s.layout);
    return REED_ERR_ARG;
  }
  if (epi_in(eight_wave ? epis_256x8(s.layout) : epis_128(s.layout), s.epi)) return REED_OK;
  if (eight_wave) reed_set_error("reed_gemm(256^2): epilogue %d is not built for layout %d", s.epi, s.layout);
  else reed_set_error("reed_gemm: unknown epilogue %d", s.epi);
  return REED_ERR_ARG;
}

int push(GemmPlan* plan, int kernel, const GemmShape& s, int row0, int col0, int ksplit_len, int tile_gm, long grid) {
  if (plan->n >= 3) {   // (cannot happen: a row split's parts and a column split's tail are too small to split again)
    reed_set_error("reed_gemm: more than 3 launches planned");
    return REED_ERR_ARG;
  }
  plan->launch[plan->n++] = GemmLaunch{kernel, row0, s.M, col0, s.N, s.splits, ksplit_len, tile_gm, (int)grid};
  return REED_OK;
}
int push256w(GemmPlan* plan, const GemmShape& s, const GemmKnobs& k, int forced, int row0, int col0, int ksplit_len) {
  const int gm = w_tile_group_rows(s.M, s.N);
  if (w_persistent(s.M, s.N, s.K, gm, k, forced)) return push(plan, GK_256WP, s, row0, col0, ksplit_len, gm, 8 * (k.ncu / 8));
  return push(plan, GK_256W, s, row0, col0, ksplit_len, gm, cdivl(s.M, 256) * cdivl(s.N, 256));
}

// One validated problem (s.epi is the plain store where dot = epilogue 13 was asked for: the kernel is selected as for the plain
// store, and where that selection is a kernel without epilogue 13 the answer is REED_ERR_UNSUPPORTED) whose output starts at
// (row0, col0) of the caller's: split it, or select its kernel.  `forced` is explicit: a split's parts that go "through the
// ordinary selection" are calls with forced = 0.
int plan_part(const GemmShape& s, bool dot, const GemmKnobs& k, int forced, int row0, int col0, int ksplit_len, GemmPlan* plan) {
  const int ncu = k.ncu;
  // Ragged-M split (round 4).  M = B * 257 tokens of a ViT tower (256 patches + CLS) is 64.25 tile rows at B = 64: the 65th row
  // tile (64 live rows) costs every GEMM of the tower a whole extra round of the chip — 65 x 16 = 1040 tiles of the fc1 GEMM are
  // 5 rounds of 256 CUs where 64 x 16 = 1024 are exactly 4 (qkv 4 -> 3, proj and fc2 2 -> 1).  Where dropping the ragged row
  // tile saves a round, the full rows go out as one launch and the <= 128 tail rows as a second, small one (the same kernels
  // on offset pointers: bit-identical results; epilogues whose row index carries meaning are left alone).
  {
    const int r = s.M % 256, mfull = s.M - r;
    if (forced == 0 && !dot && epi_in(EPIS_ROWS_FREE, s.epi) && s.splits <= 1 && nt_or_nn(s.layout) && r > 0 && r <= 128 &&
        mfull >= 2048) {
      const long ntn = cdivl(s.N, 256), rows = mfull / 256;
      if (cdivl(rows * ntn, ncu) < cdivl((rows + 1) * ntn, ncu)) {
        GemmShape m = s, t = s;
        m.M = mfull;
        t.M = r;
        const int rc = plan_part(m, dot, k, 0, row0, col0, ksplit_len, plan);
        if (rc != REED_OK) return rc;
        // the tail: a few rows against the whole weight matrix — bound by how many CUs stream it (gemm_skinny.hip)
        if (eligible_skinny(t)) return push(plan, GK_SKINNY, t, row0 + mfull, col0, ksplit_len, 0, cdivl(t.M, 16) * (t.N / 64));
        return plan_part(t, dot, k, 0, row0 + mfull, col0, ksplit_len, plan);
      }
    }
  }
  // Column split (round 6; OFF by default: REED_GEMM_COLSPLIT=1 or forced tile 259).  M = 8192 tokens (b = 32 per GPU) x N = 4608
  // (fc1 forward, the fc2 input gradient) is 32 x 18 = 576 tiles of 256^2 = 2.25 rounds of 256 CUs: three rounds on the 256^2
  // kernels, four on 256x144 tiles (what the selection below takes).  Where a leading block of tile COLUMNS fills whole rounds
  // exactly, that block goes out on the four-wave 256^2 kernel and the remaining columns as a second launch through the ordinary
  // selection (here 512 columns = 256 tiles of 128^2, one per CU): the same kernels on offset pointers, every element formed by
  // the same products in the same order (bit-identical: tests/test_gemm_gpu.py).  Measured (profiles/r6_column_split.txt): fc1
  // forward alone 98 -> 94 us, the fc2 input gradient 98 -> 96, and the b = 32 step EQUAL (957.4 / 959.0 / 954.5 against 959.0 /
  // 953.2 / 958.1 images/s, alternating on one box) — the second launch's prologue and epilogue eat what the saved round gives.
  // Kept as a switch, not as the default: it is the cheap stand-in for the 256x288 tile (two rounds of one kernel), and it bounds
  // what that tile could give from below.
  if (((forced == 0 && k.colsplit) || forced == 259) && !dot && epi_in(EPIS_COLS_FREE, s.epi) && s.splits <= 1 &&
      nt_or_nn(s.layout) && s.N % 256 == 0 && s.K >= 256) {
    const long tm = cdivl(s.M, 256), tn = s.N / 256;
    const long full = tm * tn / ncu, rem = tm * tn % ncu;
    if (full >= 1 && rem > 0 && (full * ncu) % tm == 0) {
      GemmShape h = s, t = s;
      h.N = (int)(full * ncu / tm * 256);
      t.N = s.N - h.N;
      if (eligible256w(h)) {
        // the head in whole rounds; the tail and the unsplit problem through the selection's own models (the 256x144 term asks
        // for N % 144 == 0 and nothing else)
        auto best = [&](const GemmShape& g) {
          double c = fmin(cost128(g.M, g.N, ncu), cost256(g.M, g.N, ncu, RAGGED_WHOLE_ROUNDS));
          if (g.N % 144 == 0) c = fmin(c, cost144(g.M, g.N, ncu));
          return c;
        };
        if (cost256(h.M, h.N, ncu, RAGGED_WHOLE_ROUNDS) + best(t) < 0.97 * best(s)) {
          const int rc = push256w(plan, h, k, forced, row0, col0, ksplit_len);
          if (rc != REED_OK) return rc;
          return plan_part(t, dot, k, 0, row0, col0 + h.N, ksplit_len, plan);
        }
      }
    }
  }
  if (forced == 259) return plan_part(s, dot, k, 0, row0, col0, ksplit_len, plan);   // no split for this shape

  // ---- one kernel ----
  const bool can144 = eligible144(s);
  if (forced == 64 && !dot && eligible_skinny(s))   // tests: the skinny kernel on any shape it accepts
    return push(plan, GK_SKINNY, s, row0, col0, ksplit_len, 0, cdivl(s.M, 16) * (s.N / 64));
  if ((forced == 257 || forced == 258) && eligible256w(s)) return push256w(plan, s, k, forced, row0, col0, ksplit_len);
  if ((forced == 288 && eligible288(s)) || (forced == 0 && k.use288 && prefer288(s, ncu))) {
    if (dot) return unsupported_dot();
    return push(plan, GK_288, s, row0, col0, ksplit_len, 0, cdivl(s.M, 256) * (s.N / 288));
  }
  if (can144 && (forced == 144 || s.N % 128 != 0 || (forced == 0 && prefer144(s, ncu)))) {
    if (dot) return unsupported_dot();
    return push(plan, GK_144, s, row0, col0, ksplit_len, 0, cdivl(s.M, 256) * (s.N / 144));
  }
  if (forced != 128 && (forced == 256 || prefer256(s, ncu)) && !(s.layout == LAY_TN && s.has_dbias)) {
    // the 256^2 tile: four waves of 128x128 where that kernel is built, else eight of 128x64; forced tile 256 keeps the
    // eight-wave kernel (tests, A/B timing)
    if (forced != 256 && eligible256w(s)) return push256w(plan, s, k, forced, row0, col0, ksplit_len);
    if (dot) return unsupported_dot();
    if (const int rc = square_built(s, true)) return rc;
    return push(plan, GK_256X8, s, row0, col0, ksplit_len, 4, cdivl(s.M, 256) * cdivl(s.N, 256));
  }
  if (dot) return unsupported_dot();
  if (const int rc = square_built(s, false)) return rc;
  return push(plan, GK_128, s, row0, col0, ksplit_len, 0, cdivl(s.M, 128) * (s.N / 128));
}

}  // namespace

int reed_gemm_check_dims(const GemmShape& s) {
  REED_CHECK_ARG(s.M > 0 && s.N > 0 && s.K > 0, "reed_gemm: empty problem M=%d N=%d K=%d", s.M, s.N, s.K);
  GemmShape plain = s;
  if (s.epi == EPI_BF16_DOT) {
    REED_CHECK_ARG(nt_or_nn(s.layout) && s.has_dot_operands && (s.rows_per_gate == 64 || s.rows_per_gate == 72) &&
                       s.N % s.rows_per_gate == 0 && s.N % 64 == 0 && s.splits <= 1,
                   "reed_gemm(epilogue 13): NN or NT, R and C2 given, rows_per_gate = head_dim 64 or 72 dividing N");
    plain.epi = EPI_BF16;
  }
  REED_CHECK_ARG(s.N % 128 == 0 || eligible144(plain), "reed_gemm: N=%d must be a multiple of %d (or, NT / NN with a bf16-output epilogue, of 144)",
                 s.N, 128);
  return REED_OK;
}

int reed_gemm_plan_shape(const GemmShape& in, const GemmKnobs& k, GemmPlan* plan) {
  GemmShape s = in;
  plan->n = 0;
  if (const int rc = reed_gemm_check_dims(s)) return rc;
  // epilogue 13 (store + per-head dot products with R) exists in the four-wave 256^2 kernel only: the kernel is selected as for
  // the plain store (the caller of a refused call stores plainly and lets reed_attention_bwd_ws form delta itself)
  const bool dot = s.epi == EPI_BF16_DOT;
  if (dot) s.epi = EPI_BF16;
  const int tn_tile = s.layout == LAY_TN_TALL ? GK_TN_TALL : s.layout == LAY_TN_WIDE ? GK_TN_WIDE : 0;   // gemm_tn.hip's tiles
  if (tn_tile) {
    REED_CHECK_ARG(s.epi == EPI_F32, "reed_gemm(TN 256x128 / 128x256): fp32 (weight-gradient) epilogue only");
    s.layout = LAY_TN;
  }
  if (s.layout == LAY_TN) {
    REED_CHECK_ARG(s.M % 128 == 0, "reed_gemm(TN): M=%d must be a multiple of %d", s.M, 128);
  } else {
    REED_CHECK_ARG(s.K % 64 == 0, "reed_gemm(NT/NN): K=%d must be a multiple of %d", s.K, 64);
  }
  if (s.splits < 1) s.splits = 1;
  // K per split: a multiple of 64
  const long ksteps = cdivl(s.K, 64), per = cdivl(ksteps, s.splits);
  s.splits = (int)cdivl(ksteps, per);
  const int ksplit_len = (int)std::min(per * 64, (long)INT_MAX);   // (>= K where one slice takes it all)
  if (s.splits > 1) {
    REED_CHECK_ARG(s.epi == EPI_ATOMIC_F32 || (s.epi == EPI_F32 && s.has_slab), "reed_gemm: split-K needs the atomic or slab fp32 epilogue");
  }
  if (tn_tile == GK_TN_WIDE) {
    REED_CHECK_ARG(s.N % 256 == 0, "reed_gemm(TN 128x256): N=%d must be a multiple of 256", s.N);
    return push(plan, GK_TN_WIDE, s, 0, 0, ksplit_len, 0, cdivl(s.M, 128) * (s.N / 256));
  }
  if (tn_tile) return push(plan, GK_TN_TALL, s, 0, 0, ksplit_len, 0, cdivl(s.M, 256) * (s.N / 128));
  const int rc = plan_part(s, dot, k, k.forced, 0, 0, ksplit_len, plan);
  if (rc != REED_OK) plan->n = 0;
  return rc;
}

#if !defined(REED_FP32)
// the dry run of include/reed_hip.h (the fp32-operand build has its own in gemm_f32.hip: one kernel)
extern "C" int reed_gemm_plan(int layout, int epilogue, int M, int N, int K, int split_k, int flags, int rows_per_gate, int ncu,
                              int forced_tile, int colsplit, int use288, int concurrent_comm, int* launches) {
  GemmKnobs k = reed_gemm_knobs();
  if (ncu > 0) k.ncu = ncu;
  k.forced = forced_tile;
  if (colsplit >= 0) k.colsplit = colsplit != 0;
  if (use288 >= 0) k.use288 = use288 != 0;
  k.concurrent_comm = concurrent_comm != 0;
  const GemmShape s{layout, epilogue, M, N, K, split_k, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, rows_per_gate > 0 ? rows_per_gate : 1};
  GemmPlan plan;
  if (!epi_layout_ok(layout, epilogue, N, split_k)) {
    reed_set_error("reed_gemm: epilogue %d: NT only, no split-K (17: N a multiple of 128)", epilogue);
    return -REED_ERR_ARG;
  }
  const int rc = reed_gemm_plan_shape(s, k, &plan);
  if (rc != REED_OK) return -rc;
  if (!launches) return plan.n;
  for (int i = 0; i < plan.n; ++i) {
    const GemmLaunch& l = plan.launch[i];
    const int v[GEMM_LAUNCH_INTS] = {l.kernel, l.row0, l.rows, l.col0, l.cols, l.splits, l.ksplit_len, l.tile_gm, l.grid};
    std::copy(v, v + GEMM_LAUNCH_INTS, launches + GEMM_LAUNCH_INTS * i);
  }
  return plan.n;
}
#endif

// Where the MX-fp8 block GEMM (gemm_mxfp8.hip: 128 x 128 tiles, a 128-code K step) applies: the three epilogues of the inference
// forward's block linears, whole column tiles and K steps, ragged rows.  The fp32-operand build has no such kernel: every
// entry of the family answers with the argument error there.
extern "C" int reed_gemm_mxfp8_plan(int epilogue, int M, int N, int K) {
#if defined(REED_FP32)
  (void)M; (void)N; (void)K;
  REED_CHECK_ARG(false, "reed_gemm_mxfp8: epilogue %d: not part of the fp32-operand build (use the bf16 / fp16 library)", epilogue);
#else
  REED_CHECK_ARG(epi_in(EPIS_MXFP8, epilogue), "reed_gemm_mxfp8: epilogue %d: 0, 1 or 3", epilogue);
  REED_CHECK_ARG(M >= 1 && N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0,
                 "reed_gemm_mxfp8: M=%d >= 1, N=%d and K=%d positive multiples of 128", M, N, K);
#endif
  return REED_OK;
}
#if defined(REED_FP32)
extern "C" int reed_mx_quantize(const void*, int64_t, void*, int64_t, void*, int64_t, int, int, void*) {
  REED_CHECK_ARG(false, "reed_mx_quantize: not part of the fp32-operand build (use the bf16 / fp16 library)");
  return REED_OK;
}
extern "C" int reed_gemm_mxfp8(int epilogue, const void*, int64_t, const void*, int64_t, const void*, int64_t, const void*, int64_t,
                               int M, int N, int K, void*, int64_t, void*, int64_t, const void*, int64_t, const void*, const void*,
                               int64_t, int, void*) {
  return reed_gemm_mxfp8_plan(epilogue, M, N, K);
}
#endif
