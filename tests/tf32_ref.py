"""The fp64 reference, the fp32 restatement and the error budget of the fp32 build's split GEMM (csrc/gemm_f32.hip,
gemm_f32_split_kernel; ops.f32_split): every fp32 product as three bf16 MFMA products.  A plain module, not a test file, after
tests/gemm_ref.py, whose inputs, buffers, epilogue references and epilogue restatements it reuses at kind "fp32" (there every
rounding to "the operand type" is the identity, and gemm_ref charges it one fp32 ulp).  tests/test_tf32_budgets_cpu.py proves the
budget on the CPU; tests/test_tf32_gemm_gpu.py holds the kernel to it.

THE SPLIT: hi = bf16_rne(x), lo = bf16_rne(x - float(hi)) (the subtraction is exact in fp32: hi has x's leading 8 bits), and
a b ~ a_hi b_lo + a_lo b_hi + a_hi b_hi.  Each of the three products is exact in fp32 (8 + 8 significand bits).

THE BUDGET, from the arithmetic alone (u = 2**-24):
  * x = hi + lo + r with |x - hi| <= 2**-9 |x| and |r| <= 2**-9 |x - hi| <= 2**-18 |x| (bf16 rounds to nearest at 8 bits).  So
    a b - (a_hi b_hi + a_hi b_lo + a_lo b_hi) = a_lo b_lo + a r_b + r_a b - r_a r_b, at most (2**-18 + 2 * 2**-18 + ...) |a||b|
    < 3 * 2**-16 |a||b| with room to spare: the issue's figure, kept as it states it.
  * the accumulator adds 3 K products and the bias: (3 K + 1) u' sum|a||b| with u' = 2 u — the same assumption on how the MFMA
    rounds its partial sums as gemm_ref.py's (safe under truncation of every partial sum; UNMEASURED).
  so |err of acc + bias| <= (3 * 2**-16 + (3 K + 1) u') (sum_k |a||b| + |bias|)        (the bias term as gemm_ref charges it)
  * every epilogue's own terms on top, as gemm_ref.reference derives them ("fp32 outputs": one u |value| per fp32 operation).
  * the TN bias gradient is a plain fp32 column sum of K values in some order: (K - 1) u sum|a| to first order, taken as K u sum|a|,
    plus gemm_ref's terms for the slab reduce and the prior value.
HOW gemm_ref.reference IS REUSED: it takes the accumulator's error as (K + 1) u' (mag + |bias|) from the cached mag = |A||W|^T;
scaled(inp) hands it that matrix times SCALE(K) = (3 * 2**-16 + (3 K + 1) u') / ((K + 1) u'), which turns the accumulator term on
the products into this module's and leaves every epilogue term as gemm_ref has it.  The two epilogues that read `mag` again for
their own fp32 additions (F32, ATOMIC_F32) are restated here with the true mag.

INPUTS: gemm_ref.inputs(sh, "fp32") — seeded on the CPU, per-row scales exp(0.5 N), W ~ N(0, 1 / K), the last row of A zero, the
SPECIAL values in the bias; gemm_ref.call_buffers puts them in buffers with their own leading dimensions, NaN outside the live
elements and behind each.  No element is anywhere near 2**-118, where `lo` would become a bf16 subnormal (how the MFMA reads those
is unmeasured: the kernel's header).
"""
import torch

from tests import gemm_ref as G
from tests.rowpass_ref import U

KIND = "fp32"
NT, NN, TN = G.NT, G.NN, G.TN
BK = 32                                             # the kernel's K step: the order of the restatement's sums
SPLIT_TERM = 3 * 2.0 ** -16

# M x N x K of reed_gemm.  NT / NN:
SHAPES = (G.S(9, 128, 64, "M < 16; two K steps"), G.S(200, 132, 36, "ragged M; N % 128 != 0; K % 8 == 4: the K range ends inside a packed group"),
          G.S(300, 256, 128, "three row tiles, the last ragged"), G.S(130, 384, 320, "two rows in the second row tile; ten K steps"),
          G.S(64, 384, 8, "K smaller than one K step"))
EPIS_NT = (G.BF16, G.GELU, G.SILU, G.GATE_RES, G.F32, G.QGELU, G.RES_BF16, G.LS_RES, G.GELU_G, G.SILU_G)
EPIS_NN = (G.BF16, G.DGELU, G.DSILU, G.MUL)
# TN (weight gradients; tokens x n_out x k_in in the issue's words): M = n_out, N = k_in, K = tokens; the calls of each
TN_CASES = ((G.S(768, 128, 8, "8 tokens: a quarter of a K step"), (dict(dbias=True), dict(dbias=True, accumulate=True), dict())),
            (G.S(132, 64, 40, "40 tokens; ragged second row tile; half a column tile"), (dict(dbias=True),)),
            (G.S(132, 64, 1000, "1000 tokens; split-K 3 into slabs, the bias slice in the slab"), (dict(dbias=True, split=3),)),
            (G.S(256, 384, 1000, "1000 tokens; split-K 4, atomic (the atomic epilogue carries no bias gradient)"), (dict(split=4),)))


def row(layout):
    """The gemm_ref.Row of the split kernel at this layout.  (Its tile is 128 x 128, the "128" kernel's: gemm_ref.TILE is keyed by
    that name; nothing else of the row's kernel is read at kind "fp32".)"""
    return G.Row("128", layout, EPIS_NT if layout == NT else EPIS_NN if layout == NN else (G.F32, G.ATOMIC_F32), SHAPES, 0, 0)


def calls(layout, epi, sh):
    """The variants of one (layout, epilogue, shape), with `_bias` filled in."""
    r = row(layout)
    if layout == TN:
        return [G.with_bias(r, epi, v) for s, vs in TN_CASES if s == sh for v in vs]
    return [G.with_bias(r, epi, v) for v in G.variants(r, epi, sh)]


def scale(K):
    return (SPLIT_TERM + (3 * K + 1) * 2 * U) / ((K + 1) * 2 * U)


def scaled(inp):
    """inp with the cached |A||W|^T times scale(K): see the module docstring."""
    acc, mag = G.products(inp)
    return dict(inp, acc=acc, mag=mag * scale(inp["sh"].K))


def reference(inp, epi, var, got):
    """{output: (fp64 reference, budget)} of one call in split mode."""
    sh = inp["sh"]
    M, N, K = sh[:3]
    if epi not in (G.F32, G.ATOMIC_F32):
        return G.reference(scaled(inp), epi, var, got)
    acc, mag = G.products(inp)
    b64 = inp["bias"].double() if var["_bias"] else torch.zeros(N, dtype=torch.float64)
    pre = acc + b64
    e_acc = (SPLIT_TERM + (3 * K + 1) * 2 * U) * (mag + b64.abs())
    ns = G.eff_splits(K, var.get("split", 1))[0]
    prior = inp["prior"].double()
    if epi == G.ATOMIC_F32:                           # one atomic per split onto the prior value
        return {"C": (prior + pre, e_acc + (ns + 1) * U * (prior.abs() + mag))}
    A = inp["A"].double()
    c, db = pre, A.sum(1)
    bc, bd = e_acc + U * c.abs(), K * U * A.abs().sum(1) + U * db.abs()
    if ns > 1:                                        # the slab reduce: ns fp32 additions
        bc, bd = bc + ns * U * (mag + b64.abs()), bd + ns * U * A.abs().sum(1)
    if var.get("accumulate"):
        c, db = c + prior, db + inp["prior_db"].double()
        bc, bd = bc + U * (prior.abs() + c.abs()), bd + U * (inp["prior_db"].double().abs() + db.abs())
    out = {"C": (c, bc)}
    if var.get("dbias"):
        out["dbias"] = (db, bd)
    return out


# ------------------------------------------------------------------------------------------------------- the restatement
MUTATIONS = ("drop_a_lo_b_hi", "drop_a_hi_b_lo", "lo_from_x", "hi_for_both", "lo_not_zero_filled")


def mutation_applies(m, sh):
    return sh.K % 8 == 4 if m == "lo_not_zero_filled" else True


def split(x, mutation=None):
    """(hi, lo) of an fp32 tensor, as float tensors holding bf16 values."""
    hi = x.bfloat16().float()
    if mutation == "lo_from_x":
        return hi, x.bfloat16().float()
    if mutation == "hi_for_both":
        return hi, hi.clone()
    return hi, (x - hi).bfloat16().float()


def accumulate_split(inp, var, mutation=None):
    """The split kernel's K loop in fp32: per K step of 32 the two cross products, then the main one, each an fp32 matmul of bf16
    values; per K-split a slab; the bias gradient from the fp32 operand.  Returns ([slab acc], [slab dbias]) as
    gemm_ref.accumulate32 does, so gemm_ref.restatement finishes the epilogue (restatement(..., acc=this)).
    lo_not_zero_filled: K is padded to the 8-element group the kernel packs; past K the hi half is zero and the lo half is what
    lies behind the row in memory — NaN in every buffer of these tests."""
    sh = inp["sh"]
    A, W = inp["A"].float(), inp["W"].float()
    (Ah, Al), (Wh, Wl) = split(A, mutation), split(W, mutation)
    K = sh.K
    if K % 8:
        pad = 8 - K % 8
        z = lambda t, v: torch.cat([t, torch.full((t.shape[0], pad), v)], 1)  # noqa: E731
        fill = float("nan") if mutation == "lo_not_zero_filled" else 0.0
        A, Ah, Al, Wh, Wl = z(A, 0.0), z(Ah, 0.0), z(Al, fill), z(Wh, 0.0), z(Wl, fill)
        K += pad
    ns, per = G.eff_splits(sh.K, var.get("split", 1))
    accs, dbs = [], []
    for s in range(ns):
        acc, db = torch.zeros(sh.M, sh.N), torch.zeros(sh.M)
        for k0 in range(s * per, min((s + 1) * per, K), BK):
            k = slice(k0, min(k0 + BK, K))
            if mutation != "drop_a_hi_b_lo":
                acc = acc + Ah[:, k] @ Wl[:, k].T
            if mutation != "drop_a_lo_b_hi":
                acc = acc + Al[:, k] @ Wh[:, k].T
            acc = acc + Ah[:, k] @ Wh[:, k].T
            db = db + A[:, k].sum(1)
        accs.append(acc)
        dbs.append(db)
    return accs, dbs


def restatement(inp, layout, epi, var, mutation=None):
    """The logical outputs of the split kernel + epilogue in fp32 torch."""
    return G.restatement(inp, row(layout), epi, var, acc=accumulate_split(inp, var, mutation))


def tf32_round(x):
    """fp32 -> TF32 (10 explicit mantissa bits, round to nearest even), as an fp32 tensor."""
    i = x.contiguous().view(torch.int32)
    i = (i + 0x0FFF + ((i >> 13) & 1)) & ~0x1FFF
    return i.view(torch.float32)


def rounded_operands(inp, how):
    """acc = r(A) r(W)^T in fp64 with both operands rounded once: how = "tf32" or "fp16" — the modes the split stands in for."""
    r = tf32_round if how == "tf32" else (lambda t: t.half().float())
    return r(inp["A"].float()).double() @ r(inp["W"].float()).double().T
