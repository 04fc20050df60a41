"""The cell table, fp64 references, error budgets and fp32 restatements for the nine 16-bit GEMM kernels and their 18 epilogues
(csrc/gemm.hip, gemm144.hip, gemm288.hip, gemm256.hip, gemm256w.hip, gemm_skinny.hip, gemm_tn.hip; the epilogues in
csrc/gemm_common.hpp, their contract in csrc/gemm.h).  A plain module, not a test file, after the pattern of tests/embed_ref.py:
tests/test_gemm_budgets_cpu.py proves the budgets on the CPU (each restatement stays at or below 0.6 of them, every realistic bug
leaves them by more than 20 times) and holds the table to the planner (ops.gemm_plan) both ways; tests/test_gemm_epilogues_gpu.py
holds every kernel x layout x epilogue of the bf16 and the IEEE-half build to them.

THE TABLE (ROWS): one row per (kernel, layout, epilogue set, shapes, knobs); a CELL is (row, epilogue).  `forced` is the value
of ops.gemm_force_tile that reaches the row's kernel, `reserve` the CU reserve (ops.set_cu_reserve) it runs under.  Every shape
carries the feature it is there for.  Every operand has its own leading dimension (lds()), larger than the row it strides; every
buffer is NaN outside its live elements (inputs too: a MFMA row / column that was loaded from a gap poisons exactly the outputs
that must not depend on it).

INPUTS (inputs()): seeded on the CPU, rounded to the build's operand type before the reference sees them.  A has per-row scales
exp(0.5 N), W ~ N(0, 1 / K): outputs are O(1).  bias, gate, gamma are distinct per column.  The LAST row of A is zero (M >= 2): its
accumulator is exactly 0, its pre-activation exactly the bias, which the rounding to the operand type leaves alone (delta = 0
below): that row holds the activations to their own error terms alone, at the values of SPECIAL (embed_ref.C_SPECIAL: both tails
of the fast_exp2 / fast_rcp sigmoid up to exp2 -> inf; and +-1, +-2, +-3, where a wrong polynomial coefficient shows most).  The
same values sit in row 0 of the 16-bit R (the DGELU / DSILU / MUL operand).

BUDGETS: bounds derived from the arithmetic (u = 2**-24 = rowpass_ref.U), never from what a kernel returns.
  * accumulator: e_acc = n u' sum|terms|, n = K + 1 (the K products' additions and the bias), u' = 2 u.  How a 16-bit MFMA rounds
    its internal sums is not documented where this project could read it; u' = 2 u is safe under truncation of every partial sum
    and is UNMEASURED.  (The products themselves are exact in fp32: 8 + 8 resp. 11 + 11 significand bits.)  Against a 16-bit
    output's ulp the term is negligible; it decides the fp32 outputs only.
  * one whole ulp_out per rounding to a 16-bit type, taken at |reference| + the rest of the budget where a chain precedes the
    rounding (_rounded: the computed value is what is rounded, and the chain may have carried it into the next binade).  delta = ulp_out(pre) + e_acc is how far the rounded pre-activation can be
    from the exact one (0 on a row whose products are all zero, see above).
  * chained epilogues f(r(pre)): the delta goes through a bound on |f'| over the interval it can move in,
    |f'(pre)| + F2 delta with F2 >= sup|f''| (and |f''(pre)| + F3 delta for the saved derivative); F2 = F3 = 1 holds for all four
    activations (test_gemm_budgets_cpu.py samples them).  The error terms of f are evaluated at pre and doubled (they vary by
    O(delta) relative over the interval).
  * v_exp_f32 / v_rcp_f32: 1 ulp each, treated as embed_ref.label_reference does: s = rcp(1 + exp2(e)) has the relative error
    eps_s = (3 + (2 + k |y|) (1 - s)) u, y the natural exponent and k the roundings that form e (2 for the sigmoid, 6 for the
    GELU polynomial), and the floor 2**-126 (1 + |x|) where a result is flushed.
  * gelu_erf_f (16-bit builds): the 1.5e-7 of Abramowitz & Stegun 7.1.26 on Phi, times |x|, and 12 u for the Horner chain.
  * a stored pre-activation (EPI_GELU / SILU / QGELU / GELU_ERF with C, GATE_RES with y): the stored array is held to
    ulp_out + e_acc, and the activation to f OF THE KERNEL'S OWN STORED VALUE: one transcendental term and one ulp, no chain.
  * fp32 outputs: one u |value| per fp32 operation of the epilogue (the prior value's addition, a slab reduce of `splits` terms,
    an atomic per split).

MUTATIONS of the fp32 restatement are the realistic bugs of exactly this code (MUTATIONS).  Bugs that only REMOVE a rounding (a
missing bfround) stay inside any sound budget — they make the result more accurate — and are not listed: the bit-equality tests
of tests/test_gemm_gpu.py (288 == 144, 259 == 144 == 257, 64 == 256) and the tower parity tests cover them.
"""
import math
from collections import namedtuple

import torch

from reed_amd import ops
from tests.embed_ref import C_SPECIAL, TINY
from tests.rowpass_ref import DTYPE, U, ulp_out, worst

KINDS16 = ("bf16", "fp16")
NT, NN, TN, TN_TALL, TN_WIDE = 0, 1, 2, 3, 4
LAYOUTS = (NT, NN, TN, TN_TALL, TN_WIDE)
LAY_NAME = {NT: "NT", NN: "NN", TN: "TN", TN_TALL: "TNtall", TN_WIDE: "TNwide"}
(BF16, GELU, SILU, GATE_RES, DGELU, DSILU, F32, ADDF32_RB, ATOMIC_F32, QGELU, RES_BF16, GELU_ERF, LS_RES, BF16_DOT, GELU_G, SILU_G,
 MUL, SWIGLU) = range(18)
EPI_NAME = ("bf16", "gelu", "silu", "gate_res", "dgelu", "dsilu", "f32", "addf32_rb", "atomic_f32", "qgelu", "res_bf16", "gelu_erf",
            "ls_res", "bf16_dot", "gelu_g", "silu_g", "mul", "swiglu")
assert (ops.EPI_BF16_DOT, ops.EPI_SWIGLU, ops.EPI_LS_RES, ops.EPI_GELU_ERF) == (BF16_DOT, SWIGLU, LS_RES, GELU_ERF)
SPECIAL = C_SPECIAL + (1.0, -1.0, 2.0, -2.0, 3.0, -3.0)
F2 = F3 = 1.0                                       # >= sup|f''|, sup|f'''| of gelu_tanh, gelu_erf, silu, QuickGELU
GUARD = 3                                           # NaN rows behind every 2-D buffer
PAD = 8                                             # NaN elements behind every 1-D buffer

# the epilogue sets of csrc/gemm.h restated (the table test holds them to the planner)
_ALL = set(range(18))
E_128_NT = _ALL - {BF16_DOT}
E_128_NN = E_128_NT - {LS_RES, SWIGLU}
E_144 = {BF16, GELU, SILU, GATE_RES, DGELU, DSILU, QGELU, GELU_ERF, RES_BF16, GELU_G, SILU_G, MUL}
E_288 = {BF16, GELU, GELU_G, DGELU, MUL}
E_SKINNY = {BF16, GELU, SILU, QGELU, GELU_ERF, GELU_G, SILU_G, RES_BF16, LS_RES, GATE_RES, SWIGLU}
E_W_NT = {BF16, GELU, SILU, GATE_RES, GELU_G, SILU_G, RES_BF16, LS_RES, DGELU, MUL, SWIGLU}      # + BF16_DOT: rows of its own
E_W_NN = {BF16, DGELU, DSILU, MUL}
E_F32 = {F32, ADDF32_RB, ATOMIC_F32}
E_WALK_NT, E_WALK_NN = {BF16, GATE_RES, GELU_G}, {BF16, MUL}

Row = namedtuple("Row", "kernel layout epis shapes forced reserve")
S = namedtuple("S", "M N K what")


def _row(kernel, layout, epis, shapes, forced, reserve=0):
    return Row(kernel, layout, tuple(sorted(epis)), tuple(S(*s) for s in shapes), forced, reserve)


# K-tiles of 64: one, two, three and five wherever the kernel takes them (256w, 288: K >= 128; 256wp: an even count >= 4)
_SH_128 = ((9, 128, 64, "M < 16: one partial row group; one K-tile"), (300, 256, 128, "three row tiles, the last ragged; two K-tiles"),
           (520, 128, 192, "five row tiles; three K-tiles"), (130, 384, 320, "two rows in the second tile; five K-tiles"))
_SH_256 = ((9, 256, 64, "M < 16; N % 256 == 0; one K-tile"), (300, 384, 128, "ragged second row tile; N % 256 == 128: the re-dealt last column tile"),
           (520, 640, 192, "three row tiles; N = 640: two full column tiles and the re-dealt one; three K-tiles"),
           (260, 256, 320, "four rows in the second tile; N % 256 == 0; five K-tiles"))
_SH_256W = ((9, 256, 128, "M < 16; N % 256 == 0; two K-tiles"), (300, 384, 192, "ragged second row tile; re-dealt last column tile; three K-tiles"),
            (520, 640, 320, "three row tiles; N = 640; five K-tiles"), (260, 256, 128, "four rows in the second tile; N % 256 == 0"))
_SH_256WP = ((9, 256, 256, "M < 16: 239 idle workgroups; four K-tiles"), (300, 384, 384, "ragged rows, re-dealt last column tile; six K-tiles"),
             (520, 640, 256, "three row tiles; N = 640"))
# the persistent walk at N = 1152 (4.5 column tiles): the smallest M with more tiles than workgroups, under the reserves
# tests/test_gemm_gpu.py::test_persistent_form_with_cu_reserve runs (240 / 216 workgroups; 49 x 5 = 245 / 44 x 5 = 220 tiles)
_SH_WALK = {16: ((12300, 1152, 256, "245 tiles on 240 workgroups: five walk two tiles; the last row tile has 12 rows"),),
            40: ((11020, 1152, 256, "220 tiles on 216 workgroups: four walk two tiles; the last row tile has 12 rows"),)}
_SH_144 = ((9, 144, 64, "M < 16; one tile column; one K-tile"), (300, 288, 128, "ragged second row tile; two tile columns"),
           (520, 432, 192, "three row tiles; three tile columns; three K-tiles"), (260, 144, 320, "five K-tiles"))
_SH_288 = ((9, 288, 128, "M < 16; one tile column; two K-tiles"), (300, 576, 192, "ragged second row tile; two tile columns; three K-tiles"),
           (520, 288, 320, "three row tiles; five K-tiles"), (260, 576, 128, "two tile columns"))
# (reed_gemm takes N % 128 == 0 or, on the 256x144 kernel, % 144: the skinny kernel's 64-wide tiles come in pairs)
_SH_SKINNY = ((1, 128, 64, "M = 1; one K-tile"), (17, 384, 128, "one row in the second 16-row tile; six tile columns"),
              (130, 640, 192, "nine row tiles, the last with two rows; ten tile columns; three K-tiles"), (17, 128, 320, "five K-tiles"))
_SH_TN = ((128, 128, 8, "8 tokens: one ragged K-tile"), (256, 128, 40, "40 tokens; two row tiles"),
          (128, 256, 1000, "1000 tokens: 15 K-tiles and 40 rows; split-K 3; two column tiles"))
_SH_TN_TALL = ((256, 128, 8, "8 tokens"), (128, 128, 40, "40 tokens; half a 256-row tile"), (384, 256, 1000, "1000 tokens; split-K 3; a ragged second row tile"))
_SH_TN_WIDE = ((128, 256, 8, "8 tokens"), (128, 512, 40, "40 tokens; two column tiles"), (256, 256, 1000, "1000 tokens; split-K 3"))
# EPI_BF16_DOT: head dim 64 (one slot) at N = 256; at N = 1152 (the one width % 128 == 0 that 72 divides below 2304: 16 heads)
# both 64 and 72: heads straddle the 64-column strips; ragged M
_SH_DOT = ((300, 256, 128, "4 heads of 64; ragged M"), (300, 1152, 128, "16 heads of 72 across the strips (and 18 of 64); ragged M; re-dealt last column tile"))
_SH_DOT_P = ((300, 256, 256, "4 heads of 64; ragged M"), (300, 1152, 256, "16 heads of 72 across the strips (and 18 of 64); ragged M"))

ROWS = (
    _row("128", NT, E_128_NT, _SH_128, 128), _row("128", NN, E_128_NN, _SH_128, 128), _row("128", TN, E_128_NN, _SH_TN, 128),
    _row("144", NT, E_144, _SH_144, 144), _row("144", NN, E_144, _SH_144, 144),
    _row("288", NT, E_288, _SH_288, 288),
    _row("256x8", NT, E_128_NT, _SH_256, 256), _row("256x8", NN, E_128_NN, _SH_256, 256), _row("256x8", TN, E_F32, _SH_TN, 256),
    _row("256w", NT, E_W_NT, _SH_256W, 257), _row("256w", NN, E_W_NN, _SH_256W, 257),
    _row("256w", NT, {BF16_DOT}, _SH_DOT, 257), _row("256w", NN, {BF16_DOT}, _SH_DOT, 257),
    _row("256wp", NT, E_W_NT, _SH_256WP, 258), _row("256wp", NN, E_W_NN, _SH_256WP, 258),
    _row("256wp", NT, {BF16_DOT}, _SH_DOT_P, 258), _row("256wp", NN, {BF16_DOT}, _SH_DOT_P, 258),
    _row("256wp", NT, E_WALK_NT, _SH_WALK[16], 258, 16), _row("256wp", NN, E_WALK_NN, _SH_WALK[16], 258, 16),
    _row("256wp", NT, E_WALK_NT, _SH_WALK[40], 258, 40), _row("256wp", NN, E_WALK_NN, _SH_WALK[40], 258, 40),
    _row("skinny", NT, E_SKINNY, _SH_SKINNY, 64),
    _row("tn_tall", TN_TALL, {F32}, _SH_TN_TALL, 0), _row("tn_wide", TN_WIDE, {F32}, _SH_TN_WIDE, 0),
)
KERNELS = tuple(k for k in ops.GEMM_KERNELS if k != "f32")
FORCED = {"128": 128, "144": 144, "288": 288, "256x8": 256, "256w": 257, "256wp": 258, "skinny": 64, "tn_tall": 0, "tn_wide": 0}
TILE = {"128": (128, 128), "144": (256, 144), "288": (256, 288), "256x8": (256, 256), "256w": (256, 256), "256wp": (256, 256),
        "skinny": (16, 64), "tn_tall": (256, 128), "tn_wide": (128, 256)}             # rows, columns of a workgroup's tile
CELLS = tuple((i, e) for i, r in enumerate(ROWS) for e in r.epis)


def cell_id(cell):
    r = ROWS[cell[0]]
    return f"{r.kernel}-{LAY_NAME[r.layout]}-{EPI_NAME[cell[1]]}" + (f"-reserve{r.reserve}" if r.reserve else "")


def table_cells():
    """{(kernel, layout, epilogue)} of the table."""
    return {(r.kernel, r.layout, e) for r in ROWS for e in r.epis}


ACT = (GELU, SILU, QGELU, GELU_ERF)                  # C = pre (optional), C2 = f(pre)
ACT_G = (GELU_G, SILU_G)                            # C = f'(pre) (optional), C2 = f(pre)
BWD = (DGELU, DSILU, MUL)                           # C = r(acc) * g(R)
FP32_OUT = (GATE_RES, LS_RES, F32, ADDF32_RB, ATOMIC_F32)


def variants(row, epi, sh):
    """The calls one (cell, shape) makes: dicts of store (the optional output given), rpg, hd, accumulate, dbias, split."""
    tn = row.layout in (TN, TN_TALL, TN_WIDE)
    if row.reserve:                                   # the walk rows (14 M elements): one call, the form the shape runs in training
        return [dict(rpg=256, store=True)] if epi == GATE_RES else [dict(store=True)] if epi in ACT_G else [dict()]
    if epi in ACT or epi in ACT_G:
        return [dict(store=True), dict(store=False)]
    if epi == GATE_RES:
        # 64: the scalar walk over gate rows (a boundary inside every tile of 128 rows or more); 40: not a multiple of 16, the
        # per-lane division; 256: one gate row per strip, the hoisted load (SiT's own form).  No M of the table is a multiple of 64
        # or 40 but 520 = 13 x 40.
        return [dict(rpg=64, store=True), dict(rpg=40, store=False), dict(rpg=256, store=True)]
    if epi == BF16_DOT:
        return [dict(hd=h) for h in (64, 72) if sh.N % h == 0]
    if epi == F32:
        v = [dict(), dict(accumulate=True)]
        if tn:
            db = row.kernel != "256x8"                # (the eight-wave kernel has no bias gradient: the planner sends it to 128)
            v = [dict(dbias=db), dict(dbias=db, accumulate=True)] + ([dict()] if db else [])
            if sh.K >= 3 * 64:
                v.append(dict(dbias=db, split=3))     # slabs with the bias slice in the slab
        return v
    if epi == ATOMIC_F32:
        return [dict(split=2 if sh.K >= 128 else 1)]
    return [dict()]


def eff_splits(K, split):
    """The split count reed_gemm runs (csrc/gemm_plan.cpp: K per split a multiple of 64)."""
    ksteps = -(-K // 64)
    per = -(-ksteps // max(split, 1))
    return -(-ksteps // per), per * 64


def has_bias(layout, epi):
    """Forward epilogues carry a bias; the backward's (acc only in csrc/gemm.h), the weight gradients and the atomic one do not."""
    if epi in BWD or epi == ATOMIC_F32:
        return False
    return not (epi in E_F32 and layout in (TN, TN_TALL, TN_WIDE))


def ncols(epi, N):
    return N // 2 if epi == SWIGLU else N


def lds(layout, epi, sh):
    """Leading dimensions, all different, each a multiple of 8 (reed_gemm's rule) above the row it strides."""
    prow = sh.M if layout >= TN else sh.K
    qrow = sh.K if layout == NT else sh.N
    out, used = {}, set()
    for i, (name, rowlen) in enumerate((("ldp", prow), ("ldq", qrow), ("ldc", ncols(epi, sh.N)), ("ldc2", sh.N), ("ldr", sh.N),
                                        ("ldgate", sh.N))):
        ld = -(-rowlen // 8) * 8 + 8 * (i + 1)
        while ld in used:
            ld += 8
        used.add(ld)
        out[name] = ld
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(sh, kind):
    """Everything any epilogue reads at this shape, logical (A [M, K], W [N, K]: pre = A W^T + bias), in the operand type where
    the kernels read 16 bits.  The fp64 products are cached in the dict on first use (products())."""
    M, N, K = sh.M, sh.N, sh.K
    g = torch.Generator().manual_seed(4242 + 7 * M + 3 * N + K)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    dt = DTYPE[kind]
    A = rn(M, K) * torch.exp(0.5 * rn(M, 1))
    zero_row = M - 1 if M >= 2 else None
    if zero_row is not None:
        A[zero_row] = 0
    W = rn(N, K) / math.sqrt(K)
    bias = 1.5 * rn(N)
    bias[:len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.float64)
    R16 = 1.5 * rn(M, N)
    R16[0, :len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.float64)
    return dict(sh=sh, kind=kind, A=A.to(dt), W=W.to(dt), bias=bias.to(dt), R16=R16.to(dt), gate=rn(-(-M // 40) + 1, N).to(dt),
                gamma=(1 + 0.5 * rn(N)).float(), R32=(2 * rn(M, N)).float(), prior=rn(M, N).float(), prior_db=rn(M).float(),
                zero_row=zero_row)


def subset(inp, idx):
    """The same inputs restricted to the output rows idx (absolute row numbers, kept in "rows"): every budget and every restatement
    is a per-element function of its row of A, so the CPU conditions of a 12 k-row shape are proven on the rows of its first and
    last tiles at a hundredth of the cost.  The GPU test never uses this: it compares every element."""
    sh = inp["sh"]
    out = dict(inp, sh=S(len(idx), sh.N, sh.K, sh.what), rows=idx, M_full=sh.M)
    for k in ("A", "R16", "R32", "prior"):
        out[k] = inp[k][idx]
    out["prior_db"] = inp["prior_db"][idx]
    out.pop("acc", None), out.pop("mag", None)
    return out


def _rows(inp):
    """Absolute row number of each output row."""
    return inp["rows"] if "rows" in inp else torch.arange(inp["sh"].M)


def products(inp):
    """fp64 A W^T and |A| |W|^T, once per shape and kind, shared by every epilogue; never modified."""
    if "acc" not in inp:
        A, W = inp["A"].double(), inp["W"].double()
        inp["acc"], inp["mag"] = A @ W.T, A.abs() @ W.abs().T
    return inp["acc"], inp["mag"]


# ------------------------------------------------------------------------------------------------- activations in fp64
_C = 2.0 * 0.7978845608028654


def _f_gelu(x):
    y = _C * (x + 0.044715 * x ** 3)
    s, om, G = torch.sigmoid(y), torch.sigmoid(-y), _C * (1 + 3 * 0.044715 * x * x)
    return dict(f=x * s, d=s + x * s * om * G, s=s, om=om, G=G, y=y, k=6.0)


def _f_silu(x):
    s, om = torch.sigmoid(x), torch.sigmoid(-x)
    return dict(f=x * s, d=s * (1 + x * om), s=s, om=om, G=torch.ones_like(x), y=x, k=2.0)


def _f_qgelu(x):
    y = 1.702 * x
    s, om = torch.sigmoid(y), torch.sigmoid(-y)
    return dict(f=x * s, d=s + y * s * om, s=s, om=om, G=torch.full_like(x, 1.702), y=y, k=2.0)


def _f_erf(x):
    z = x / math.sqrt(2.0)
    phi = torch.where(x < 0, 0.5 * torch.special.erfc(-z), 1 - 0.5 * torch.special.erfc(z))
    return dict(f=x * phi, d=phi + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi))


FN = {GELU: _f_gelu, GELU_G: _f_gelu, DGELU: _f_gelu, SILU: _f_silu, SILU_G: _f_silu, DSILU: _f_silu, SWIGLU: _f_silu, QGELU: _f_qgelu,
      GELU_ERF: _f_erf}


def _d2(fn, x, h=1e-5):
    """f'' by a central difference of the analytic f' (fp64: good to 1e-9, against budgets of 1e-4 and more)."""
    return (fn(x + h)["d"] - fn(x - h)["d"]) / (2 * h)


def _eps_s(p):
    return 3 + (2 + p["k"] * p["y"].abs()) * p["om"]


def e_act(epi, x, kind):
    """Bound on the error of the kernel's fp32 activation of an EXACT fp32 x, before the rounding to the output type."""
    p = FN[epi](x)
    if epi == GELU_ERF:
        return x.abs() * (1.5e-7 + 12 * U)
    if epi == QGELU:
        # a = r(1.702 x); s~ = r(sigmoid(a)); f = x s~: sigma' <= sigma'(|1.702 x| - da) over the interval a can lie in
        y = p["y"]
        da = ulp_out(y, kind) + 2 * U * y.abs()
        lo = (y.abs() - da).clamp(min=0)
        ds = torch.sigmoid(lo) * torch.sigmoid(-lo) * da + _eps_s(p) * U * p["s"] + ulp_out(p["s"], kind) + TINY
        return x.abs() * ds + U * p["f"].abs()
    return (_eps_s(p) + 1) * U * p["f"].abs() + TINY * (1 + x.abs())


def e_grad(epi, x):
    """The same for the derivative s + x s (1 - s) G (G = 2u' for GELU, 1 for SiLU): s's error eps_s u goes through the
    cancellation 1 - s with the weight s, |x| G s^2 eps_s u, and through everything else with the size S = s + |x| G s (1 - s) of
    the two terms; six more roundings (x s, its product with s, the difference, G's two and the final fma)."""
    p = FN[epi](x)
    xg = x.abs() * p["G"]
    size = p["s"] + xg * p["s"] * p["om"] + xg * p["s"] * p["s"]
    return (_eps_s(p) + 8) * U * size + TINY * (1 + x.abs()) * (1 + xg)


# -------------------------------------------------------------------------------------------------------- fp64 reference
def _rounded(ref, rest, kind):
    """Budget of an output rounded to the operand type whose unrounded value is within `rest` of ref: the rounding happens at the
    COMPUTED value, which `rest` may have carried across a binade edge, so the whole ulp is taken at |ref| + rest."""
    return rest + ulp_out(ref.abs() + rest, kind)


def reference(inp, epi, var, got):
    """{output: (fp64 reference, budget)} of one call.  `got` holds the outputs under test (fp64, logical): the stored
    pre-activation / y / C that the next output is held to where csrc/gemm.h makes the kernel's own stored value its input."""
    sh, kind = inp["sh"], inp["kind"]
    M, N, K = sh[:3]
    acc, mag = products(inp)
    lay_bias = var["_bias"]
    b64 = inp["bias"].double() if lay_bias else torch.zeros(N, dtype=torch.float64)
    pre = acc + b64
    e_acc = (K + 1) * 2 * U * (mag + b64.abs())
    delta = torch.where(mag == 0, torch.zeros_like(pre), ulp_out(pre, kind) + e_acc)          # r(pre) against pre
    b_pre = ulp_out(pre, kind) + e_acc
    out = {}
    if epi in (BF16, BF16_DOT):
        out["C"] = (pre, b_pre)
        if epi == BF16_DOT:
            hd = var["hd"]
            cr = got["C"] * inp["R16"].double()
            out["dsum"] = (cr.reshape(M, N // hd, hd).sum(2).T, (hd + 4) * U * cr.abs().reshape(M, N // hd, hd).sum(2).T)
    elif epi in ACT:
        if var["store"]:
            x = got["C"]
            out["C"] = (pre, b_pre)
            f = FN[epi](x)["f"]
            out["C2"] = (f, _rounded(f, e_act(epi, x, kind), kind))
        else:
            p = FN[epi](pre)
            out["C2"] = (p["f"], _rounded(p["f"], (p["d"].abs() + F2 * delta) * delta + 2 * e_act(epi, pre, kind), kind))
    elif epi in ACT_G:
        p = FN[epi](pre)
        out["C2"] = (p["f"], _rounded(p["f"], (p["d"].abs() + F2 * delta) * delta + 2 * e_act(epi, pre, kind), kind))
        if var["store"]:
            out["C"] = (p["d"], _rounded(p["d"], (_d2(FN[epi], pre).abs() + F3 * delta) * delta + 2 * e_grad(epi, pre), kind))
    elif epi == SWIGLU:
        H = N // 2
        x1, x2, d1, d2 = pre[:, :H], pre[:, H:], delta[:, :H], delta[:, H:]
        p = _f_silu(x1)
        eh = _rounded(p["f"], (p["d"].abs() + F2 * d1) * d1 + 2 * e_act(SILU, x1, kind), kind)
        o = p["f"] * x2
        out["C"] = (o, _rounded(o, x2.abs() * eh + p["f"].abs() * d2 + eh * d2 + U * o.abs(), kind))
    elif epi == GATE_RES:
        gt = inp["gate"].double()[_rows(inp) // var["rpg"]]
        R = inp["R32"].double()
        if var["store"]:
            out["C2"] = (pre, b_pre)
            gy = gt * got["C2"]
            c = R + gy
            out["C"] = (c, ulp_out(gy, kind) + 2 * U * c.abs())
        else:
            gy = gt * pre
            c = R + gy
            out["C"] = (c, _rounded(gy, gt.abs() * delta, kind) + 2 * U * c.abs())
    elif epi == LS_RES:
        gy = inp["gamma"].double() * pre
        c = inp["R32"].double() + gy
        out["C"] = (c, inp["gamma"].double().abs() * delta + 2 * U * (gy.abs() + c.abs()))
    elif epi == RES_BF16:
        c = pre + inp["R16"].double()
        out["C"] = (c, _rounded(c, delta + U * c.abs(), kind))
    elif epi in (DGELU, DSILU):
        x = inp["R16"].double()
        d = FN[epi](x)["d"]
        o = pre * d
        out["C"] = (o, _rounded(o, d.abs() * delta + (pre.abs() + delta) * e_grad(epi, x) + U * o.abs(), kind))
    elif epi == MUL:
        x = inp["R16"].double()
        o = pre * x
        out["C"] = (o, _rounded(o, x.abs() * delta, kind))
    elif epi == ADDF32_RB:
        c = inp["prior"].double() + pre
        out["C"] = (c, b_pre + 2 * U * c.abs())
    elif epi == ATOMIC_F32:
        ns = eff_splits(K, var.get("split", 1))[0]
        c = inp["prior"].double() + pre
        out["C"] = (c, e_acc + (ns + 1) * U * (inp["prior"].double().abs() + mag))
    elif epi == F32:
        ns = eff_splits(K, var.get("split", 1))[0]
        A = inp["A"].double()
        c, db = pre, A.sum(1)
        bc, bd = e_acc + U * c.abs(), (K + 1) * 2 * U * A.abs().sum(1) + U * db.abs()
        if ns > 1:
            bc, bd = bc + ns * U * (mag + b64.abs()), bd + ns * U * A.abs().sum(1)
        if var.get("accumulate"):
            c, db = c + inp["prior"].double(), db + inp["prior_db"].double()
            bc, bd = bc + U * (inp["prior"].double().abs() + c.abs()), bd + U * (inp["prior_db"].double().abs() + db.abs())
        out["C"] = (c, bc)
        if var.get("dbias"):
            out["dbias"] = (db, bd)
    else:
        raise ValueError(epi)
    return out


def ratios(got, ref):
    """{output: (worst error / budget, flat index)}; every element counts."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {k: worst((got[k].double().flatten() - ref[k][0].flatten()).abs(), ref[k][1].flatten()) for k in ref}


# -------------------------------------------------------------------------------------------------------- fp32 restatement
MUTATIONS = ("bias_plus8", "bias_dropped", "gate_plus8", "gate_dropped", "gamma_plus8", "drop_last_ktile", "ktile_twice", "gelu_d1_no3",
             "gelu_c1_dropped", "silu_grad_sign", "qgelu_1702_to_1", "r_with_ldc", "c2_with_ldc", "gate_row_tile_local",
             "gate_row_off_by_one", "ragged_halves_swapped", "strip_from_neighbour", "accumulate_overwrite",
             "dbias_first_split_only", "dot_slot_at_72", "swiglu_wrong_partner")
_USES_R = (GATE_RES, LS_RES, RES_BF16, BF16_DOT) + BWD


def mutation_applies(m, row, epi, sh, var):
    """Whether mutation m is a bug this (cell, shape, call) can have at all: the code it breaks runs here."""
    if m in ("bias_plus8", "bias_dropped"):
        return has_bias(row.layout, epi)
    if m in ("gate_plus8", "gate_dropped"):
        return epi == GATE_RES
    if m == "gamma_plus8":
        return epi == LS_RES
    if m in ("drop_last_ktile", "ktile_twice"):
        return True
    if m == "gelu_d1_no3":
        return epi == DGELU or (epi == GELU_G and var["store"])
    if m == "gelu_c1_dropped":
        return epi in (GELU, GELU_G, DGELU)
    if m == "silu_grad_sign":
        return epi == DSILU or (epi == SILU_G and var["store"])
    if m == "qgelu_1702_to_1":
        return epi == QGELU
    if m == "r_with_ldc":
        return epi in _USES_R and sh.M >= 2
    if m == "c2_with_ldc":
        return (epi in ACT or epi in ACT_G or (epi == GATE_RES and var["store"])) and sh.M >= 2
    if m == "gate_row_tile_local":                    # the first row tile is right either way
        return epi == GATE_RES and sh.M > TILE[row.kernel][0] and TILE[row.kernel][0] % var["rpg"] != 0
    if m == "gate_row_off_by_one":
        return epi == GATE_RES and sh.M >= var["rpg"]
    if m == "ragged_halves_swapped":
        return row.kernel in ("256x8", "256w", "256wp") and row.layout in (NT, NN) and sh.N % 256 == 128
    if m == "strip_from_neighbour":
        return row.kernel in ("144", "288")
    if m == "accumulate_overwrite":
        return epi == ADDF32_RB or (epi == F32 and bool(var.get("accumulate")))
    if m == "dbias_first_split_only":
        return epi == F32 and bool(var.get("dbias")) and eff_splits(sh.K, var.get("split", 1))[0] > 1
    if m == "dot_slot_at_72":
        return epi == BF16_DOT and var["hd"] == 72
    if m == "swiglu_wrong_partner":
        return epi == SWIGLU
    raise ValueError(m)


def _sig(t):
    return 1.0 / (1.0 + torch.exp2(t))


def _c32(v):
    return torch.tensor(v, dtype=torch.float32)


def _gelu32(x, mutation):
    c0 = _c32(-2.0) * _c32(0.7978845608028654) * _c32(1.4426950408889634)
    c1 = c0 * _c32(0.0 if mutation == "gelu_c1_dropped" else 0.044715)
    d0 = _c32(2.0) * _c32(0.7978845608028654)
    d1 = d0 * (_c32(1.0) if mutation == "gelu_d1_no3" else _c32(3.0)) * _c32(0.044715)
    s = _sig(x * (c1 * (x * x) + c0))
    act = x * s
    return act, (act - act * s) * (d1 * (x * x) + d0) + s


def _silu32(x, mutation):
    s = _sig(_c32(-1.4426950408889634) * x)
    return x * s, s * (1.0 + x * (1.0 - s)) if mutation != "silu_grad_sign" else s * (1.0 - x * (1.0 - s))


def _erf32(x):
    z = x.abs() * _c32(0.7071067811865476)
    t = 1.0 / (_c32(0.3275911) * z + 1.0)
    q = t * _c32(0.5 * 1.061405429) + _c32(0.5 * -1.453152027)
    for a in (1.421413741, -0.284496736, 0.254829592):
        q = q * t + _c32(0.5 * a)
    q = q * t * torch.exp2(z * z * _c32(-1.4426950408889634))
    return x * torch.where(x < 0, q, 1.0 - q)


def _strided(vals, ld_write, ld_read, rows, nrows):
    """vals [M, n] (absolute rows `rows` of nrows) written with one leading dimension into a NaN buffer and read back with another."""
    M, n = vals.shape
    flat = torch.full(((nrows + GUARD) * max(ld_write, ld_read) + n,), float("nan"), dtype=vals.dtype)
    r, c = rows[:, None], torch.arange(n)[None, :]
    flat[r * ld_write + c] = vals
    return flat[r * ld_read + c]


def accumulate32(inp, var, mutation=None):
    """The K loop in fp32: 64-wide K-tiles in order, one fp32 matmul each, per K-split a slab.  Returns ([slab acc], [slab dbias])."""
    sh = inp["sh"]
    A, W = inp["A"].float(), inp["W"].float()
    ns, per = eff_splits(sh.K, var.get("split", 1))
    tiles = [(k0, min(k0 + 64, sh.K)) for k0 in range(0, sh.K, 64)]
    if mutation == "drop_last_ktile":
        tiles = tiles[:-1]
    accs, dbs = [], []
    for z in range(ns):
        acc, db = torch.zeros(sh.M, sh.N), torch.zeros(sh.M)
        mine = [t for t in tiles if z * per <= t[0] < (z + 1) * per]
        if mutation == "ktile_twice" and z == 0:
            mine = mine[:1] + mine
        for k0, k1 in mine:
            acc = acc + A[:, k0:k1] @ W[:, k0:k1].T
            db = db + A[:, k0:k1].sum(1)
        accs.append(acc)
        dbs.append(db)
    return accs, dbs


def restatement(inp, row, epi, var, mutation=None, acc=None):
    """The kernel's own order of operations in fp32 torch -> the logical outputs (float tensors).  `acc` = accumulate32's result
    where the caller shares it between epilogues.  mutation: one of MUTATIONS, see mutation_applies and the comments below."""
    assert mutation is None or mutation in MUTATIONS
    sh, kind = inp["sh"], inp["kind"]
    M, N, K = sh[:3]
    dt = DTYPE[kind]
    r = lambda v: v.to(dt).float()  # noqa: E731
    ld = lds(row.layout, epi, sh)
    Mf = inp.get("M_full", M)
    accs, dbs = acc if acc is not None else accumulate32(inp, var, mutation)
    bias = inp["bias"].float() if var["_bias"] else torch.zeros(N)
    if mutation == "bias_plus8":
        bias = torch.roll(bias, -8)                  # the neighbouring lane's 8 columns
    if mutation == "bias_dropped":
        bias = torch.zeros(N)
    pre = accs[0] + bias
    R16 = inp["R16"].float()
    if mutation == "r_with_ldc" and epi != GATE_RES and epi != LS_RES:
        R16 = _strided(R16, ld["ldr"], ld["ldc"], _rows(inp), Mf)
    R32 = inp["R32"] if mutation != "r_with_ldc" else _strided(inp["R32"], ld["ldr"], ld["ldc"], _rows(inp), Mf)
    out = {}
    if epi in (BF16, BF16_DOT):
        out["C"] = r(pre)
        if epi == BF16_DOT:
            hd = var["hd"]
            Sl = 1 if hd == 64 else 2
            dp = torch.full((N // hd, Sl, M), float("nan"))
            cr = out["C"] * R16
            for q in range(N // 64):                 # strip by strip, as the waves write: tail of head hA, start of hA + 1
                hA = 64 * q // hd
                slot = q - (hA * hd) // 64 if mutation != "dot_slot_at_72" else (64 * q - hA * hd) // 64
                cols = torch.arange(64 * q, 64 * q + 64)
                inA = cols // hd == hA
                dp[hA, slot] = cr[:, cols[inA]].sum(1)
                if (64 * q + 63) // hd != hA:
                    dp[hA + 1, 0] = cr[:, cols[~inA]].sum(1)
            out["dsum"] = dp.sum(1)
    elif epi in ACT or epi in ACT_G:
        x = r(pre)
        if epi in (GELU, GELU_G):
            a, g = _gelu32(x, mutation)
        elif epi in (SILU, SILU_G):
            a, g = _silu32(x, mutation)
        elif epi == QGELU:
            a, g = x * r(_sig(_c32(-1.4426950408889634) * r(_c32(1.0 if mutation == "qgelu_1702_to_1" else 1.702) * x))), None
        else:
            a, g = _erf32(x), None
        out["C2"] = r(a)
        if var["store"]:
            out["C"] = r(g) if epi in ACT_G else x
    elif epi == SWIGLU:
        x = r(pre)
        x1, x2 = x[:, :N // 2], x[:, N // 2:]
        if mutation == "swiglu_wrong_partner":
            x2 = torch.roll(x2, -8, 1)               # the x2 group of the next lane pair
        out["C"] = r(r(_silu32(x1, None)[0]) * x2)
    elif epi == GATE_RES:
        rpg, bm = var["rpg"], TILE[row.kernel][0]
        m = _rows(inp)
        grow = m // rpg
        if mutation == "gate_row_tile_local":
            grow = (m % bm) // rpg
        if mutation == "gate_row_off_by_one":
            grow = (m + 1) // rpg
        gate = inp["gate"].float()
        gate = torch.cat([gate[:-(-Mf // rpg)], torch.full((gate.shape[0], N), float("nan"))])[grow]   # NaN behind the last gate row
        if mutation == "gate_plus8":
            gate = torch.roll(gate, -8, 1)
        if mutation == "gate_dropped":
            gate = torch.ones_like(gate)
        y = r(pre)
        out["C"] = R32 + r(gate * y)
        if var["store"]:
            out["C2"] = y
    elif epi == LS_RES:
        gamma = inp["gamma"] if mutation != "gamma_plus8" else torch.roll(inp["gamma"], -8)
        out["C"] = R32 + gamma * r(pre)
    elif epi == RES_BF16:
        out["C"] = r(r(pre) + R16)
    elif epi == DGELU:
        out["C"] = r(r(pre) * _gelu32(R16, mutation)[1])
    elif epi == DSILU:
        out["C"] = r(r(pre) * _silu32(R16, mutation)[1])
    elif epi == MUL:
        out["C"] = r(r(pre) * R16)
    elif epi == ADDF32_RB:
        out["C"] = (inp["prior"] if mutation != "accumulate_overwrite" else 0) + r(pre)
    elif epi == ATOMIC_F32:
        c = inp["prior"].clone()
        for a in accs:
            c = c + a
        out["C"] = c
    elif epi == F32:
        keep = bool(var.get("accumulate")) and mutation != "accumulate_overwrite"
        c, db = (inp["prior"].clone(), inp["prior_db"].clone()) if keep else (torch.zeros(M, N), torch.zeros(M))
        for z, (a, d) in enumerate(zip(accs, dbs)):
            c = c + (a + bias)
            if z == 0 or mutation != "dbias_first_split_only":
                db = db + d
        out["C"] = c
        if var.get("dbias"):
            out["dbias"] = db
    else:
        raise ValueError(epi)
    if mutation == "c2_with_ldc" and "C2" in out:
        out["C2"] = _strided(out["C2"], ld["ldc"], ld["ldc2"], _rows(inp), Mf)
    if mutation == "ragged_halves_swapped":           # the re-dealt last column tile: its two 64-column halves
        for k in ("C", "C2"):
            if k in out:
                w = 64 * out[k].shape[1] // N
                n0 = out[k].shape[1] - 2 * w
                out[k] = torch.cat([out[k][:, :n0], out[k][:, n0 + w:], out[k][:, n0:n0 + w]], 1)
    if mutation == "strip_from_neighbour":            # 144: columns 64..79 of a tile from the wave column at 80; 288: the two strips
        for k in ("C", "C2"):
            if k in out:
                o = out[k].clone()
                for t0 in range(0, N, TILE[row.kernel][1]):
                    if row.kernel == "144":
                        o[:, t0 + 64:t0 + 80] = out[k][:, t0 + 80:t0 + 96]
                    else:
                        o[:, t0 + 128:t0 + 144], o[:, t0 + 272:t0 + 288] = out[k][:, t0 + 272:t0 + 288], out[k][:, t0 + 128:t0 + 144]
                out[k] = o
    return out


def with_bias(row, epi, var):
    """The call's dict with `_bias` (whether a bias vector is passed) filled in."""
    return dict(var, _bias=has_bias(row.layout, epi))


# ------------------------------------------------------------------------------------------------- buffers of the GPU run
def _buf2(vals, ld, dtype, rows=None):
    """[rows + GUARD, ld] of NaN with vals in its top left corner."""
    rows = vals.shape[0] if rows is None else rows
    b = torch.full((rows + GUARD, ld), float("nan"), dtype=dtype)
    b[:vals.shape[0], :vals.shape[1]] = vals.to(dtype)
    return b


def _buf1(n, vals=None):
    b = torch.full((n + PAD,), float("nan"), dtype=torch.float32)
    if vals is not None:
        b[:n] = vals
    return b


def call_buffers(inp, row, epi, var):
    """CPU tensors of one reed_gemm call (physical layout, NaN outside the live elements) and its keyword arguments.
    Returns (bufs, kw, live) with live = {buffer name: (rows, columns) | count} of the OUTPUT buffers."""
    sh, kind = inp["sh"], inp["kind"]
    M, N, K = sh[:3]
    dt, f32 = DTYPE[kind], torch.float32
    lay, ld = row.layout, lds(row.layout, epi, sh)
    A, W, bias = inp["A"], inp["W"], inp["bias"]
    if epi == SWIGLU:
        W, bias = ops.swiglu_pack(W, bias)           # the kernel's row order; the references keep SwiGLUFFNFused's chunk(2)
    b = dict(P=_buf2(A if lay < TN else A.T, ld["ldp"], dt), Q=_buf2(W if lay == NT else W.T, ld["ldq"], dt))
    kw = dict(ldp=ld["ldp"], ldq=ld["ldq"], ldc=ld["ldc"])
    live = {}
    if var["_bias"]:
        b["bias"] = torch.cat([bias, torch.full((PAD,), float("nan"), dtype=dt)])
    out32 = epi in FP32_OUT
    nc = ncols(epi, N)
    want_c = not ((epi in ACT or epi in ACT_G) and not var["store"])
    ns, _ = eff_splits(K, var.get("split", 1))
    slab = epi == F32 and var.get("split", 1) > 1
    if slab:
        stride = M * ld["ldc"] + M + PAD              # slab z = [dW slice z | dbias slice z | pad]
        b["ws"] = torch.full((ns * stride,), float("nan"), dtype=f32)
        b["C"] = torch.full((stride,), float("nan"), dtype=f32)   # reduce_slabs' output, the slab's own layout
        kw.update(split_k=var["split"], slab_stride=stride)
        live["C"] = (M, nc)
    elif want_c:
        prior = (epi == F32 and var.get("accumulate")) or epi in (ADDF32_RB, ATOMIC_F32)
        c0 = inp["prior"] if prior else torch.full((0, nc), float("nan"))
        b["C"] = _buf2(c0, ld["ldc"], f32 if out32 else dt, rows=M)
        live["C"] = (M, nc)
        if epi == ATOMIC_F32:
            kw["split_k"] = var["split"]
    if epi in ACT or epi in ACT_G or (epi == GATE_RES and var["store"]):
        b["C2"] = _buf2(torch.zeros(0, N), ld["ldc2"], dt, rows=M)
        b["C2"][:] = float("nan")
        kw["ldc2"] = ld["ldc2"]
        live["C2"] = (M, N)
    if epi == BF16_DOT:
        hd = var["hd"]
        b["C2"] = _buf1((N // hd) * (1 if hd == 64 else 2) * M)
        kw.update(rows_per_gate=hd)
        live["C2"] = b["C2"].numel() - PAD
    if epi in _USES_R:
        b["R"] = _buf2(inp["R32"] if epi in (GATE_RES, LS_RES) else inp["R16"], ld["ldr"], f32 if epi in (GATE_RES, LS_RES) else dt)
        kw["ldr"] = ld["ldr"]
    if epi == GATE_RES:
        b["gate"] = _buf2(inp["gate"][:-(-M // var["rpg"])], ld["ldgate"], dt)
        kw.update(ldgate=ld["ldgate"], rows_per_gate=var["rpg"])
    if epi == LS_RES:
        b["gate"] = torch.cat([inp["gamma"], torch.full((PAD,), float("nan"))])
    if var.get("dbias") and not slab:
        b["dbias"] = _buf1(M, inp["prior_db"] if var.get("accumulate") else None)
        live["dbias"] = M
    if var.get("accumulate"):
        kw["accumulate"] = True
    return b, kw, live


def plan_args(row, epi, sh, var):
    """Arguments of ops.gemm_plan for this call (everything but the knobs)."""
    return dict(lay=row.layout, epi=epi, M=sh.M, N=sh.N, K=sh.K, split_k=var.get("split", 1), dbias=bool(var.get("dbias")),
                slab=epi == F32 and var.get("split", 1) > 1, dot_operands=True,
                rows_per_gate=var.get("rpg", var.get("hd", 1)))
