"""fp64 references, error budgets and fp32 restatements for the LoRA kernels (csrc/lora.hip: reed_lora_merge, reed_lora_grads).
A plain module, not a test file, after the pattern of tests/gemm_ref.py: tests/test_lora_budgets_cpu.py proves the budgets on the
CPU (each restatement stays at or below 0.6 of them, every listed mutation leaves them), tests/test_lora_gpu.py holds the kernels
of the three builds to them.

WHAT THE KERNELS COMPUTE (include/reed_hip.h), r = rounding to the build's operand type (the identity in the fp32 build):
    u = r(s (x a^T)) [M, R]     v = r(s (dy b)) [M, R]     db [N, R] (+)= dy^T u     da [R, K] (+)= v^T x
    w' = fma(s, acc, w), acc = sum_j b[n, j] a[j, k] by fma in ascending j;  w_op = r(w')

BUDGETS: bounds derived from the arithmetic (u = 2**-24 = rowpass_ref.U), never from what a kernel returns.
  * a MFMA (or fp32 FMA / tree) sum of n terms: n u' sum|terms| with u' = 2 u (gemm_ref.py: safe under truncation of every
    partial sum);
  * e_u = the distance of the stored u from the exact s (x a^T): the first product's sum (K terms) and the scale's rounding,
    then one whole ulp_out taken at |u| + that;
  * that e_u carried through the second product: sum_m |dy[m, n]| e_u[m, j]; the second product's own sum over the M terms, the
    <= 32 slab partials and the prior value: (M + 34) u' sum_m |dy| (|u| + e_u); one u for the fp32 add of the prior value.
  * the merge: (R + 1) u s sum_j |b a| for the fma chain and one u |w'| for the last fma.

INPUTS (grads_inputs): seeded on the CPU and rounded to the operand type before the reference sees them; x ~ N(0, 1) with per-row
scales, dy ~ 0.05 N, a ~ N / sqrt(K), b ~ 0.1 N, all entries distinct, so a transposed index or a row taken from the wrong operand
moves every output; s = 1.5 (not a power of two: its rounding is exercised, and s, 1 and s^2 are far apart); the prior values of
da / db are O(1), far above the budget, so an `accumulate` that drops them shows.
"""
import math

import torch

from tests.rowpass_ref import DTYPE, U, ulp_out, worst  # noqa: F401

KINDS = ("bf16", "fp16", "fp32")
UP = 2.0 * U
SCALE = 1.5
SLAB = 64                                                   # ops.LORA_UV_ROWS: rows of x | dy per workgroup of the u / v pass
MS = (16, SLAB - 1, SLAB, 2 * SLAB + 16)
NKS = ((128, 128), (384, 128), (128, 512))
RS = (8, 16, 64)
SHAPES = tuple((M, N, K, R) for M in MS for (N, K) in NKS for R in RS)
MUTATIONS = ("scale_missing", "scale_twice", "u_from_dy", "drop_last_slab", "pad_as_data", "acc_ignores_prior", "a_transposed",
             "b_transposed")


def applies(mut, M, N, K, R, accumulate):
    return {"u_from_dy": N == K, "drop_last_slab": M % SLAB != 0, "pad_as_data": R == 8,
            "acc_ignores_prior": bool(accumulate)}.get(mut, True)


def grads_inputs(M, N, K, R, kind, seed=0):
    g = torch.Generator().manual_seed(4321 + seed + 7 * M + N + 3 * K + R)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    dt = DTYPE[kind]
    x = (rn(M, K) * torch.exp(0.5 * rn(M, 1))).to(dt)
    dy = (0.05 * rn(M, N)).to(dt)
    a = (rn(R, K) / math.sqrt(K)).to(dt)
    b = (0.1 * rn(N, R)).to(dt)
    return dict(x=x, dy=dy, a=a, b=b, da0=rn(R, K).float(), db0=rn(N, R).float(), scale=SCALE, M=M, N=N, K=K, R=R, kind=kind)


def grads_reference(inp, accumulate):
    """fp64 (da, db) from the operand-type inputs, and the budget of each."""
    x, dy, a, b = (inp[k].double() for k in ("x", "dy", "a", "b"))
    s, M, N, K, kind = inp["scale"], inp["M"], inp["N"], inp["K"], inp["kind"]

    def stored(p, q, n):        # s (p q^T) and how far the kernel's stored, rounded value can be from it
        val = s * (p @ q.T)
        e_acc = s * (n + 1) * UP * (p.abs() @ q.abs().T) + U * val.abs()
        return val, e_acc + ulp_out(val.abs() + e_acc, kind)

    u, e_u = stored(x, a, K)
    v, e_v = stored(dy, b.T, N)
    db, da = dy.T @ u, v.T @ x
    e_db = dy.abs().T @ e_u + (M + 34) * UP * (dy.abs().T @ (u.abs() + e_u))
    e_da = e_v.T @ x.abs() + (M + 34) * UP * ((v.abs() + e_v).T @ x.abs())
    if accumulate:
        db, da = db + inp["db0"].double(), da + inp["da0"].double()
        e_db = e_db + U * (db.abs() + e_db)
        e_da = e_da + U * (da.abs() + e_da)
    return dict(da=da, db=db, e_da=e_da, e_db=e_db)


def grads_restatement(inp, accumulate, mutation=None):
    """The kernels' arithmetic in fp32 torch on the CPU (sums in torch's order: the budgets do not depend on it)."""
    dt = DTYPE[inp["kind"]]
    x, dy, a, b = (inp[k].float() for k in ("x", "dy", "a", "b"))
    s, M, N, K, R = inp["scale"], inp["M"], inp["N"], inp["K"], inp["R"]
    if mutation == "a_transposed":
        a = a.reshape(K, R).T.contiguous()
    if mutation == "b_transposed":
        b = b.reshape(R, N).T.contiguous()
    su = {"scale_missing": 1.0, "scale_twice": s * s}.get(mutation, s)
    rows = M // SLAB * SLAB if mutation == "drop_last_slab" else M
    u = (torch.tensor(su, dtype=torch.float32) * ((dy if mutation == "u_from_dy" else x) @ a.T)).to(dt).float()
    v = (torch.tensor(su, dtype=torch.float32) * (dy @ b)).to(dt).float()
    if mutation == "pad_as_data":       # R = 8 on a 16-wide tile: columns 8..15 loaded from what lies behind, stored at the pitch R
        g = torch.Generator().manual_seed(99)
        u = torch.cat([u, torch.randn(M, 8, generator=g)], 1)
        v = torch.cat([v, torch.randn(M, 8, generator=g)], 1)
        db = (dy[:rows].T @ u[:rows]).flatten()[:N * R].view(N, R)
        da = (v[:rows].T @ x[:rows])[:R]    # (its rows 8..15 would land behind da: the NaN guards of the GPU test see those)
    else:
        db, da = dy[:rows].T @ u[:rows], v[:rows].T @ x[:rows]
    if accumulate and mutation != "acc_ignores_prior":
        db, da = inp["db0"] + db, inp["da0"] + da
    return dict(da=da, db=db)


def grads_ratio(got, ref):
    """The largest error / budget over da and db."""
    return max(worst((got["da"].double() - ref["da"]).abs(), ref["e_da"])[0],
               worst((got["db"].double() - ref["db"]).abs(), ref["e_db"])[0])


# ------------------------------------------------------------------------------------------------------------------ merge
MERGE_SHAPES = ((5, 12, 8), (64, 256, 16), (130, 516, 64), (384, 128, 32))     # (N, K, R): ragged rows and column chunks


def merge_inputs(N, K, R, seed=0):
    g = torch.Generator().manual_seed(777 + seed + N + K + R)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return dict(w=(rn(N, K) / math.sqrt(K)).float(), a=(rn(R, K) / math.sqrt(K)).float(), b=(0.1 * rn(N, R)).float(), scale=SCALE,
                N=N, K=K, R=R)


def merge_reference(inp):
    w, a, b = (inp[k].double() for k in ("w", "a", "b"))
    s, R = inp["scale"], inp["R"]
    ref = w + s * (b @ a)
    return ref, (R + 1) * U * s * (b.abs() @ a.abs()) + U * ref.abs()


def merge_restatement(inp, mutation=None):
    w, a, b = inp["w"], inp["a"], inp["b"]
    s = {"scale_missing": 1.0, "scale_twice": inp["scale"] ** 2}.get(mutation, inp["scale"])
    if mutation == "a_transposed":
        a = a.reshape(inp["K"], inp["R"]).T.contiguous()
    if mutation == "b_transposed":
        b = b.reshape(inp["R"], inp["N"]).T.contiguous()
    return w + torch.tensor(s, dtype=torch.float32) * (b @ a)


MERGE_MUTATIONS = ("scale_missing", "scale_twice", "a_transposed", "b_transposed")
