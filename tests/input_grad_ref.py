"""fp64 references, error budgets and fp32 restatements for the two input-gradient kernels of csrc/embed.hip:
reed_patch_embed_bwd_x (dL/dx: the patch-embed convolution's input gradient) and reed_timestep_sinusoid_bwd (dL/dt through the
sinusoid table).  A plain module, not a test file, after tests/embed_ref.py: tests/test_input_grad_budgets_cpu.py proves the budgets
on the CPU (each restatement stays at or below 0.6 of them, every realistic bug leaves them by 20 times or more),
tests/test_input_grad_gpu.py holds the kernels to them.

Every fp64 reference starts from the inputs ROUNDED AS THE KERNEL READS THEM (dtok, an fp32 array, through rnd(); the weight in the
operand type as it is), fp64 from there on.  Budgets are bounds derived from the arithmetic (u = 2**-24), never from what a kernel
delivers: n u sum|terms| for an fp32 summation tree of depth n (Higham 4.2: each term passes through at most n additions), the
products' own rounding counted as one more level, and for the sinusoid the argument and transcendental terms of
embed_ref.sin_reference.
"""
import math

import torch

from tests import embed_ref as E
from tests.adaln_ref import rnd
from tests.rowpass_ref import DTYPE, U

# (B, C, HW, P, D): embed_ref.PATCH_SHAPES and one shape for the streaming form's own tail — 18 tokens (9 pairs in one block, waves
# 1 .. 3 with two pairs and wave 0 with three), D = 328: 82 16-byte loads per row, the second group of 64 with 18 live lanes
PATCH_SHAPES = E.PATCH_SHAPES + ((2, 4, 6, 2, 328),)
STREAM_K, STREAM_MAX_D, STREAM_GROUP, GENERIC_GROUP = 16, 1280, 256, 64
LEVELS = 6                                        # the halves 32 + 32, 16 + 16, ..., 1 + 1 over the 64 lanes


def _gen(seed):
    g = torch.Generator().manual_seed(24680 + seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


# ----------------------------------------------------------------------------------------------- patch embed, dL/dx
def bwdx_form(K, D, aligned):
    """'stream16' (patch_embed_bwd_x16_kernel) or 'generic' (patch_embed_bwd_x_kernel): the rule of reed_patch_embed_bwd_x
    restated.  `aligned`: dtok and the weight at 16-byte addresses.  The same in every build."""
    return "stream16" if K == STREAM_K and D % 4 == 0 and D <= STREAM_MAX_D and aligned else "generic"


def lane_columns(form, D):
    """[64 lists]: the columns d a lane sums, in the order of its chain.  stream16: d = 4 (lane + 64 j) + e, j then e ascending;
    generic: d = lane + 64 i."""
    if form == "stream16":
        return [[4 * (lane + 64 * j) + e for j in range(-(-D // 256)) for e in range(4) if 4 * (lane + 64 * j) + e < D]
                for lane in range(64)]
    return [list(range(lane, D, 64)) for lane in range(64)]


def tree_depth(form, D):
    """Additions a term passes through at most: the longest lane chain and the six levels of halves."""
    return max(len(c) for c in lane_columns(form, D)) + LEVELS


def bwdx_inputs(B, C, HW, P, D, kind, seed=0):
    """dtok fp32 [B T, D] with a per-token scale exp(0.5 N); w = 0.2 N (operand type) [D, K].
    One probe, at the LAST token and k = K - 1 (embed_ref.patch_inputs turned round): dtok[d] = sgn_d 2**e_d (e_d = 3 d mod 5 - 2,
    the sign changing every second d), moved by 0.49 of the operand type's spacing AWAY from that power of two (up on the even d,
    down on the odd d: both round back; no offset in the fp32 build), and w[d, K - 1] = +-0.5 sgn_d 2**-e_d, + on the even and - on
    the odd d (D is even in every shape).  So the sum is 0 exactly, its budget the tree's own on D terms of size 0.5, and a dtok that
    is not rounded errs the same way in every term: 0.3675 D (half spacing) in all, 0.735 (half spacing) / (n u) budgets."""
    rn = _gen(seed + 3000 + D + HW)
    G = HW // P
    T, K = G * G, C * P * P
    assert D % 2 == 0
    dtok = (rn(B * T, D) * torch.exp(0.5 * rn(B * T, 1))).float()
    half_ulp = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}[kind]
    d = torch.arange(D)
    even = d % 2 == 0
    mag = torch.ldexp(torch.ones(D, dtype=torch.float64), (3 * d) % 5 - 2) * torch.where((d // 2) % 2 == 0, 1.0, -1.0)
    dtok[B * T - 1] = (mag * torch.where(even, 1.0 + 0.98 * half_ulp, 1.0 - 0.49 * half_ulp)).float()
    w = 0.2 * rn(D, K)
    w[:, K - 1] = torch.where(even, 0.5, -0.5) / mag
    return dict(dtok=dtok, w=w.to(DTYPE[kind]), B=B, C=C, HW=HW, P=P, D=D, T=T, K=K, kind=kind)


def _scatter(val, inp, order=0, swap_hw=False):
    """[B T, K] -> flat dx [B C HW HW] (NaN where nothing is written) through embed_ref.patch_src_index, the kernels' patch_src
    restated.  order 1 / swap_hw: the index bugs of BWDX_MUTATIONS."""
    B, C, HW, P, T, K = (inp[k] for k in ("B", "C", "HW", "P", "T", "K"))
    idx = E.patch_src_index(B, C, HW, P, order)
    if swap_hw:                                                     # token (ph, pw) lands where (pw, ph) belongs
        G = HW // P
        t = torch.arange(T)
        perm = (t % G) * G + t // G
        idx = idx.reshape(B, T, K)[:, perm].reshape(-1)
    out = torch.full((B * C * HW * HW,), float("nan"), dtype=val.dtype)
    out[idx] = val.reshape(-1)
    return out


def bwdx_reference(inp, form):
    """dx = r(dtok) @ w in fp64, scattered in patch order (c, pi, pj).  Budget: a term passes through tree_depth(form, D)
    additions, and its product rounds once in the fp32 build (exact in the 16-bit builds: counted all the same):
    (depth + 1) u sum_d |r(dtok) w|.  The output is fp32: no further rounding."""
    g = rnd(inp["dtok"].double(), inp["kind"])
    W = inp["w"].double()
    n = tree_depth(form, inp["D"]) + 1
    return dict(dx=_scatter(g @ W, inp), b_dx=_scatter(n * U * (g.abs() @ W.abs()), inp))


BWDX_MUTATIONS = ("order_pijc", "ph_pw_swapped", "last_token_dropped", "d_tail_dropped", "dtok_unrounded")


def bwdx_tail(form, D):
    """First column of the last, partly filled group of a row (256 columns per trip of the streaming form, 64 of the generic
    one), or None where D fills its groups exactly."""
    grp = STREAM_GROUP if form == "stream16" else GENERIC_GROUP
    return None if D % grp == 0 else D // grp * grp


def bwdx_restatement(inp, form, mutation=None):
    """Both kernels in fp32 torch: per lane one chain over its columns from 0.0f (lane_columns), then the halves
    p[:32] + p[32:], p[:16] + p[16:], ...: x + y has the same bits on both lanes of an exchange, so which lane keeps which half
    does not enter.  mutation: order_pijc = k written as (pi, pj, c); ph_pw_swapped; last_token_dropped = the last token of the
    last block is never written (stays NaN); d_tail_dropped = the partly filled last group of columns is skipped;
    dtok_unrounded."""
    assert mutation is None or mutation in BWDX_MUTATIONS
    D, K, kind = inp["D"], inp["K"], inp["kind"]
    g = inp["dtok"] if mutation == "dtok_unrounded" else inp["dtok"].to(DTYPE[kind]).float()
    w = inp["w"].float()
    cols = lane_columns(form, D)
    if mutation == "d_tail_dropped":
        cols = [[d for d in c if d < bwdx_tail(form, D)] for c in cols]
    depth = max(len(c) for c in cols)
    p = torch.zeros(g.shape[0], 64, K)
    for i in range(depth):
        live = torch.tensor([len(c) > i for c in cols])
        d = torch.tensor([c[i] if len(c) > i else 0 for c in cols])
        gi = torch.where(live, g[:, d], torch.zeros(()))            # a lane past the end of its chain adds nothing
        p = p + gi[:, :, None] * w[d][None]
    n = 64
    while n > 1:
        n //= 2
        p = p[:, :n] + p[:, n:2 * n]
    val = p[:, 0]
    if mutation == "last_token_dropped":
        val = val.clone()
        val[-1] = float("nan")
    return dict(dx=_scatter(val, inp, 1 if mutation == "order_pijc" else 0, mutation == "ph_pw_swapped"))


# ------------------------------------------------------------------------------------------------- sinusoid, dL/dt
def sinb_inputs(dim, seed=0):
    """t = embed_ref.SIN_T; dsin fp32 [7, dim] = N(0, 1), the padding column of an odd dim included (it must not count)."""
    rn = _gen(seed + 5000 + dim)
    return dict(t=torch.tensor(E.SIN_T, dtype=torch.float32), dsin=rn(len(E.SIN_T), dim).float(), dim=dim)


def sinb_reference(inp, max_period):
    """dt[b] = sum_k f_k (cos(arg) dS_k - sin(arg) dC_k), dC = dsin[:, :half], dS = dsin[:, half:2 half], f and arg = t f as in
    embed_ref.sin_reference, fp64 from the fp32 t and dsin.
    Per term, with eps_f = (4 + 3 ln max_period) u the relative error of the fp32 f and of arg (sin_reference):
      * cos and sin err by at most |arg| eps_f + 4 u each (slope at most 1; sinf / cosf themselves): f (|dS| + |dC|) times that;
      * f's own error and the four roundings of the expression (two products, the difference, the product with f):
        (eps_f + 4 u) f (|cos dS| + |sin dC|).
    The sum: ceil(half / 64) terms per lane chain, six levels of halves: (ceil(half / 64) + 6) u sum_k f (|cos dS| + |sin dC|)."""
    dim = inp["dim"]
    half = dim // 2
    f = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    arg = inp["t"].double()[:, None] * f
    g = inp["dsin"].double()
    dC, dS = g[:, :half], g[:, half:2 * half]
    c, s = torch.cos(arg), torch.sin(arg)
    eps_f = (4 + 3 * math.log(max_period)) * U
    mag = f * ((c * dS).abs() + (s * dC).abs())
    e = f * (dS.abs() + dC.abs()) * (arg.abs() * eps_f + 4 * U) + (eps_f + 4 * U) * mag
    n = -(-half // 64) + LEVELS
    return dict(dt=(f * (c * dS - s * dC)).sum(1), b_dt=e.sum(1) + n * U * mag.sum(1))


SINB_MUTATIONS = ("sin_sign", "swap_halves", "no_f", "pad_counted")


def sinb_restatement(inp, max_period, mutation=None):
    """sinusoid_bwd_kernel in fp32 torch (f and arg as embed_ref.sin_restatement forms them): a chain per lane over
    k = lane, lane + 64, ..., then the halves.  mutation: sin_sign = + for -; swap_halves = cos on dsin[:, :half] and sin on the
    other half; no_f = the factor f_k omitted; pad_counted = the last column of an odd dim added."""
    assert mutation is None or mutation in SINB_MUTATIONS
    dim = inp["dim"]
    half = dim // 2
    a = torch.tensor(-math.log(max_period), dtype=torch.float32) * torch.arange(half, dtype=torch.float32)
    f = torch.exp(a / torch.tensor(float(half)))
    arg = inp["t"][:, None] * f
    g = inp["dsin"]
    dC, dS = g[:, :half], g[:, half:2 * half]
    if mutation == "swap_halves":
        dC, dS = dS, dC
    c, s = torch.cos(arg), torch.sin(arg)
    v = c * dS + s * dC if mutation == "sin_sign" else c * dS - s * dC
    term = v if mutation == "no_f" else f * v
    per = -(-half // 64)
    term = torch.cat([term, torch.zeros(term.shape[0], 64 * per - half)], 1).reshape(-1, per, 64)
    p = torch.zeros(term.shape[0], 64)
    for i in range(per):
        p = p + term[:, i]
    n = 64
    while n > 1:
        n //= 2
        p = p[:, :n] + p[:, n:2 * n]
    dt = p[:, 0]
    if mutation == "pad_counted":
        dt = dt + g[:, dim - 1]
    return dict(dt=dt)
