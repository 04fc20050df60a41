// Which kernels a reed_gemm call runs, and on which part of the problem: host arithmetic only (gemm_plan.cpp).
// reed_gemm_launch (gemm.hip) validates the pointers, asks for a plan and launches it; reed_gemm_plan (include/reed_hip.h) hands
// the same plan to the planning side and to the CPU tests.
#pragma once
#include "gemm.h"

enum GemmKernel {
  GK_128 = 0,     // gemm.hip: 128^2 tiles, two workgroups per CU
  GK_144 = 1,     // gemm144.hip: 256x144 tiles
  GK_288 = 2,     // gemm288.hip: 256x288 tiles
  GK_256X8 = 3,   // gemm256.hip: 256^2 tiles, eight waves
  GK_256W = 4,    // gemm256w.hip: 256^2 tiles, four waves, one tile per workgroup
  GK_256WP = 5,   // gemm256w.hip: the same, persistent (one workgroup per CU walks a static list of tiles)
  GK_SKINNY = 6,  // gemm_skinny.hip: 16 x 64 tiles, one wave each
  GK_TN_TALL = 7, // gemm_tn.hip: 256x128 tiles
  GK_TN_WIDE = 8, // gemm_tn.hip: 128x256 tiles
  GK_F32 = 9,     // gemm_f32.hip: the fp32-operand build's exact kernel (fp32 MFMA)
  GK_F32_SPLIT = 10   // gemm_f32.hip: the same build under reed_gemm_f32_split(1): three bf16 MFMA products per fp32 product
};

// What the selection reads of a call.  No pointers: only whether the optional ones were given.
struct GemmShape {
  int layout, epi, M, N, K, splits;
  bool has_dbias;          // TN: the fused bias gradient is asked for
  bool has_slab;           // slab_stride > 0 (split-K into slabs)
  bool has_dot_operands;   // R and C2 given (epilogue 13)
  int rows_per_gate;
};
// Forced tile: 0 = heuristic; 64 / 128 / 144 / 256 (eight waves) / 257 (four waves, one-shot) / 258 (four waves, persistent
// wherever the form applies) / 288 = that kernel where the shape allows; 259 = heuristic plus the column split.
struct GemmKnobs {
  int ncu, forced;
  bool colsplit, use288, concurrent_comm;
};
struct GemmLaunch {
  int kernel;              // GemmKernel
  int row0, rows;          // the rows [row0, row0 + rows) of the output ...
  int col0, cols;          // ... and its columns [col0, col0 + cols)
  int splits, ksplit_len;  // split-K: grid.y and the K range of one slice
  int tile_gm;             // 256^2 kernels: tile rows per XCD-local group of the workgroup -> tile map; 0 elsewhere
  int grid;                // grid.x
};
struct GemmPlan {
  int n;
  GemmLaunch launch[3];
};
constexpr int GEMM_LAUNCH_INTS = 9;

// REED_OK and the launches in order, or REED_ERR_ARG / REED_ERR_UNSUPPORTED with the reason in reed_last_error() and no launch.
// A function of its arguments alone.
int reed_gemm_plan_shape(const GemmShape& s, const GemmKnobs& k, GemmPlan* plan);

// The first of reed_gemm's checks — empty problem, epilogue 13's conditions, N's multiple —, which reed_gemm_launch reports before
// it looks at leading dimensions and alignment; reed_gemm_plan_shape begins with them too.
int reed_gemm_check_dims(const GemmShape& s);

// The knobs the process has set (reed_gemm_force_tile, reed_gemm_f32_split, reed_set_cu_reserve, reed_set_concurrent_comm,
// REED_GEMM_COLSPLIT, REED_GEMM288) — their one definition, in every build of the library.
int reed_num_cus();            // the device's CUs minus the reserve, at least 32; 256 without a device
int reed_gemm_forced_tile();
int reed_concurrent_comm();
int reed_gemm_f32_split_on();   // reed_gemm_f32_split: always 0 in the 16-bit builds
GemmKnobs reed_gemm_knobs();
