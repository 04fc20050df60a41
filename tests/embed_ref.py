"""fp64 references, error budgets and fp32 restatements for the embedders, the conditioning kernels and the small-K weight gradient
of csrc/embed.hip (reed_smallk_wgrad, reed_patch_embed_fwd, reed_patchify_bf16, reed_timestep_sinusoid, reed_label_cond,
reed_label_cond_bwd).  A plain module, not a test file, after the pattern of tests/rowpass_ref.py and tests/adaln_ref.py:
tests/test_embed_budgets_cpu.py proves the budgets on the CPU (each restatement stays at or below 0.6 of them, every realistic bug
leaves them by more than 20 times), tests/test_embed_gpu.py holds the kernels to them.

Every fp64 reference starts from the inputs ROUNDED AS THE KERNEL READS THEM (the operand-type arrays as they are; an fp32 array
the kernel rounds on load through rnd()), fp64 from there on.  Budgets are bounds derived from the arithmetic (u = 2**-24,
rowpass_ref.U), never from what a kernel delivers:
  * ulp_out(ref, kind) per rounding to the output type (a whole ulp where half would do: a value whose own fp32 error carries it
    across a rounding boundary is covered);
  * n u sum|terms| for an fp32 chain of n additions (Higham 4.2), the products' own roundings counted as further additions;
  * for the transcendentals the terms derived in label_reference / sin_reference.
"""
import math

import torch

from tests.adaln_ref import rnd
from tests.rowpass_ref import DTYPE, U, ulp_out, worst

NSL = 256                                         # token slices of the two-stage small-K wgrad (csrc/embed.hip)
# (M, Dw, KS) of the small-K tests: see tests/test_embed_gpu.py for what each one reaches
SMALLK_SHAPES = ((1, 2, 8), (255, 130, 16), (257, 128, 32), (2309, 66, 16), (2309, 130, 40), (700, 34, 24), (320, 384, 64),
                 (80, 128, 256))
# (B, C, HW, P, D) of the patch-embed and patchify tests
PATCH_SHAPES = ((1, 4, 2, 2, 4), (5, 4, 18, 2, 1280), (5, 4, 18, 2, 1284), (3, 4, 12, 4, 260), (3, 2, 6, 2, 72), (1, 4, 16, 8, 128))
SIN_CASES = ((256, 10000.0), (2, 10000.0), (7, 100.0))                      # (dim, max_period)
SIN_T = (0.0, 1e-4, 0.37, 0.5, 1.0, 37.25, 999.0)
LABEL_SHAPES = ((6, 128, 10), (1, 4, 1), (3, 260, 5), (7, 1152, 1000))      # (B, D, num_classes)
C_SPECIAL = (0.0, 0.5, -0.5, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)      # values c takes in every label case (the first four at B D = 4)
TINY = 2.0 ** -126                                # the smallest normal fp32: v_exp_f32 / v_rcp_f32 return 0 below it


def _gen(seed):
    g = torch.Generator().manual_seed(9876 + seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def ratios(got, ref, outputs):
    """{output: (worst error / budget, flat index)} of a result dict (tensors of any float type) against a reference dict."""
    return {k: worst((got[k].double().cpu().flatten() - ref[k].flatten()).abs(), ref["b_" + k].flatten()) for k in outputs if k in got}


# ------------------------------------------------------------------------------------------------------- small-K wgrad
def smallk_rg(KS):
    """Rows per load group of smallk_wgrad_kernel: RG = 8 in the KSP = 16 instantiations (KS <= 16), 4 in the KSP = 32 ones."""
    return 8 if KS <= 16 else 4


def smallk_form(KS, wide_f32):
    """The instantiation reed_smallk_wgrad launches and its grid's z extent: the entry point's rule restated."""
    ksp = 16 if KS <= 16 else 32
    return f"smallk_wgrad_kernel<{'true' if wide_f32 else 'false'}, {ksp}>", (1 if ksp == 16 else -(-KS // 32))


def smallk_inputs(M, Dw, KS, kind, wide_f32, seed=0):
    """wide [M, Dw] (fp32, which the kernel rounds to the operand type on load, or the operand type), small [M, KS] (operand type):
    a per-row scale exp(0.5 N) on wide, an offset on both so that the column sums do not vanish; a non-zero prior value for each
    of the three outputs (the accumulate runs start from it)."""
    rn = _gen(seed + 17 * M + Dw + KS)
    wide = rn(M, Dw) * torch.exp(0.5 * rn(M, 1)) + 0.25
    small = rn(M, KS) + 0.1
    return dict(wide=wide.float() if wide_f32 else wide.to(DTYPE[kind]), small=small.to(DTYPE[kind]), prior_out=rn(Dw * KS).float(),
                prior_cw=rn(Dw).float(), prior_cs=rn(KS).float(), M=M, Dw=Dw, KS=KS, kind=kind, wide_f32=wide_f32)


def _lay(o, layout):
    """[..., Dw, KS] -> [..., Dw KS] flat in the output layout: 0 = d * KS + k, 1 = k * Dw + d."""
    return (o if layout == 0 else o.transpose(-1, -2)).reshape(*o.shape[:-2], -1)


def smallk_reference(inp, layout, accumulate):
    """out[d, k] = sum_m r(wide)[m, d] small[m, k], colsum_wide[d] = sum_m r(wide)[m, d], colsum_small[k] = sum_m small[m, k], on
    top of the prior value with `accumulate`.

    The kernel sums per = ceil(M / 256) rows in one fp32 chain per slice (an FMA per row: one rounding; a product and an addition
    where the compiler does not contract: the product of two operand-type numbers is exact in fp32 in the 16-bit builds and one
    more rounding in the fp32 build, counted in the slack of the 0.6 condition), then the 256 slice partials in one chain (on top
    of the prior value, which is the chain's start): (per + 256) u sum|terms|.  With accumulate the prior value takes part in every
    one of the 256 partial sums of that chain: 256 u |prior|, and u |ref| for the result's own last rounding.  (u (|prior| + |ref|)
    would be the prior value's share if it were added once at the end; the kernel starts from it, the same argument as for dtable
    in label_reference.)"""
    M, kind = inp["M"], inp["kind"]
    W = rnd(inp["wide"].double(), kind) if inp["wide_f32"] else inp["wide"].double()
    S = inp["small"].double()
    n = (-(-M // NSL) + NSL) * U
    res = {}
    for name, val, mag, prior in (("out", _lay(W.T @ S, layout), _lay(W.abs().T @ S.abs(), layout), inp["prior_out"]),
                                  ("cw", W.sum(0), W.abs().sum(0), inp["prior_cw"]), ("cs", S.sum(0), S.abs().sum(0), inp["prior_cs"])):
        b = n * mag
        if accumulate:
            val = val + prior.double()
            b = b + U * (NSL * prior.double().abs() + val.abs())
        res[name], res["b_" + name] = val, b
    return res


SMALLK_STAGE1_MUTATIONS = ("tail_unmasked", "drop_last_row", "ks_tail_zero")
SMALLK_MUTATIONS = SMALLK_STAGE1_MUTATIONS + ("drop_slice", "layout_swap", "accumulate_overwrite")
SMALLK_OUTPUTS = ("out", "cw", "cs")


def smallk_stage1(inp, mutation=None):
    """smallk_wgrad_kernel in fp32 torch: the per-slice partials (out [256, Dw, KS], colsum_wide [256, Dw], colsum_small [256, KS]),
    each one chain over the slice's rows in row order.  They depend neither on the layout nor on accumulate.
    mutation: tail_unmasked = the rows past the slice's end in its last group of RG are clamped to the last row but not zeroed
    (that row counts up to RG times in out and colsum_wide; colsum_small has a loop of its own); drop_last_row = every slice stops
    one row short; ks_tail_zero = the last 8-chunk of KS is never loaded."""
    assert mutation is None or mutation in SMALLK_STAGE1_MUTATIONS
    M, Dw, KS, kind = inp["M"], inp["Dw"], inp["KS"], inp["kind"]
    per = -(-M // NSL)
    w = inp["wide"].to(DTYPE[kind]).float()
    s = inp["small"].float()
    pad = NSL * per - M                                             # rows past M: zero terms, exact
    w = torch.cat([w, torch.zeros(pad, Dw)]).reshape(NSL, per, Dw)
    s = torch.cat([s, torch.zeros(pad, KS)]).reshape(NSL, per, KS)
    nz = (M - torch.arange(NSL) * per).clamp(0, per)                # rows of each slice
    if mutation == "ks_tail_zero":
        sk = s.clone()
        sk[:, :, KS - 8:] = 0
    else:
        sk = s
    acc, cw, cs = torch.zeros(NSL, Dw, KS), torch.zeros(NSL, Dw), torch.zeros(NSL, KS)
    for j in range(per):
        live = (j < (nz - 1 if mutation == "drop_last_row" else nz)).float()[:, None]
        wj = w[:, j] * live
        acc = acc + wj[:, :, None] * sk[:, j, None, :]
        cw = cw + wj
        cs = cs + s[:, j] * live
    if mutation == "tail_unmasked":
        rg = smallk_rg(KS)
        extra = torch.where(nz > 0, -(-nz // rg) * rg - nz, torch.zeros_like(nz))
        last = (nz - 1).clamp(min=0)
        wl, sl = w[torch.arange(NSL), last], sk[torch.arange(NSL), last]
        for e in range(int(extra.max())):
            live = (extra > e).float()[:, None]
            acc = acc + (wl * live)[:, :, None] * sl[:, None, :]
            cw = cw + wl * live
    return dict(out=acc, cw=cw, cs=cs)


def smallk_reduce(parts, inp, layout, accumulate, mutation=None):
    """smallk_reduce_kernel in fp32 torch on stage 1's partials: from the prior value (accumulate) or 0.0f, the 256 slices in order.
    mutation: drop_slice = the chain starts at slice 1; layout_swap = stage 1 wrote the other layout; accumulate_overwrite = the
    prior value is not read."""
    assert mutation is None or mutation in SMALLK_MUTATIONS
    lay = 1 - layout if mutation == "layout_swap" else layout
    res = {}
    for name, p, prior in (("out", _lay(parts["out"], lay), inp["prior_out"]), ("cw", parts["cw"], inp["prior_cw"]),
                           ("cs", parts["cs"], inp["prior_cs"])):
        tot = prior.clone() if accumulate and mutation != "accumulate_overwrite" else torch.zeros_like(prior)
        for z in range(1 if mutation == "drop_slice" else 0, NSL):
            tot = tot + p[z]
        res[name] = tot
    return res


def smallk_restatement(inp, layout, accumulate, mutation=None):
    return smallk_reduce(smallk_stage1(inp, mutation if mutation in SMALLK_STAGE1_MUTATIONS else None), inp, layout, accumulate,
                         mutation)


# ------------------------------------------------------------------------------------------- patchify and patch embed
def patch_src_index(B, C, HW, P, order):
    """The index map of csrc/embed.hip patch_src restated with plain integer arithmetic: out.flat[i] = x.flat[idx[i]] for
    i = (b T + t) K + k; order 0: k = (c, pi, pj), the conv's input; order 1: k = (pi, pj, c), the unpatchify order."""
    G = HW // P
    T, K = G * G, C * P * P
    i = torch.arange(B * T * K)
    k, bt = i % K, i // K
    b, t = bt // T, bt % T
    ph, pw = t // G, t % G
    if order == 0:
        c, r = k // (P * P), k % (P * P)
    else:
        c, r = k % C, k // C
    pi, pj = r // P, r % P
    return ((b * C + c) * HW + ph * P + pi) * HW + pw * P + pj


def patches(x, C, P, order=0):
    """[B, C, HW, HW] -> [B T, K] by reshape and permute (independent of patch_src_index: the CPU test holds one to the other)."""
    B, _, HW, _ = x.shape
    G = HW // P
    v = x.reshape(B, C, G, P, G, P)
    v = v.permute(0, 2, 4, 1, 3, 5) if order == 0 else v.permute(0, 2, 4, 3, 5, 1)
    return v.reshape(B * G * G, C * P * P)


def embed_form(kind, K, D, aligned):
    """'reg16' (patch_embed_fwd16_kernel: the weight rows of 4 columns in registers) or 'generic' (patch_embed_fwd_kernel): the
    rule of reed_patch_embed_fwd restated.  `aligned`: weight, pos and tokens at 16-byte addresses.  The same in every build."""
    assert kind in DTYPE
    return "reg16" if K == 16 and D % 4 == 0 and D <= 4 * 320 and aligned else "generic"


def patch_inputs(B, C, HW, P, D, kind, seed=0):
    """x fp32 with a per-token scale, w = 0.2 N (operand type), bias = N (operand type), pos = N (fp32).
    One probe, at the LAST token and column D - 1: the patch is x[k] = sgn_k 2**e_k (e_k = 3 k mod 5 - 2, the sign changing every
    second k), moved by 0.49 of the operand type's spacing AWAY from that power of two: up on the even k (0.49 ulp above), down on
    the odd k (0.49 of the half-sized ulp below); both round back to the power of two (no offset in the fp32 build).
    w[D - 1, k] = +-0.5 sgn_k 2**-e_k, + on the even and - on the odd k; no bias there and pos = 0.  So lin = 0 exactly and the
    budget there is the chain's own, while the terms differ in size and sign from k to k: an x that is not rounded to the operand
    type shows at full size (every term errs the same way: + 0.5 * 0.49 ulp on the even k, - 0.5 * -0.245 ulp on the odd k) instead
    of drowning in the output's own rounding, and a wrong patch order shows at the one-token shape, where this patch is the only
    one."""
    rn = _gen(seed + 1000 + D + HW)
    G = HW // P
    T, K = G * G, C * P * P
    pt = (rn(B * T, K) * torch.exp(0.5 * rn(B * T, 1))).float()
    half_ulp = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}[kind]
    k = torch.arange(K)
    even = k % 2 == 0
    mag = torch.ldexp(torch.ones(K, dtype=torch.float64), (3 * k) % 5 - 2) * torch.where((k // 2) % 2 == 0, 1.0, -1.0)
    pt[B * T - 1] = (mag * torch.where(even, 1.0 + 0.98 * half_ulp, 1.0 - 0.49 * half_ulp)).float()
    x = pt.reshape(B, G, G, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, HW, HW).contiguous()
    w, bias, pos = 0.2 * rn(D, K), rn(D), rn(T, D).float()
    w[D - 1] = torch.where(even, 0.5, -0.5) / mag
    bias[D - 1] = 0
    pos[T - 1, D - 1] = 0
    return dict(x=x, w=w.to(DTYPE[kind]), bias=bias.to(DTYPE[kind]), pos=pos, B=B, C=C, HW=HW, P=P, D=D, T=T, K=K, kind=kind)


def patch_reference(inp, bias=True):
    """tok = r(sum_k w[d, k] r(x)[k] + bias[d]) + pos[t, d], patch order (c, pi, pj).
    The fp32 chain over k has K additions, the bias is one more and the products one (fp32 build; exact in the 16-bit builds):
    (K + 2) u (sum|terms| + |bias|); one rounding to the operand type: ulp_out(lin); the addition of pos in fp32, and the
    rounding of r(lin) + pos as the fp32 output: 2 u |tok|.
    The fp64 reference leaves the r() out (tok = lin + pos), as rowpass_ref's references do: the kernel's one rounding moves a
    value by at most half of ulp_out(lin), and the whole ulp that is budgeted covers a sum whose own fp32 error carries it
    across a rounding boundary.  (Against r(lin) + pos such a flip is an error of a whole ulp: all of the budget or none.)"""
    kind, K, T, D, B = inp["kind"], inp["K"], inp["T"], inp["D"], inp["B"]
    X = rnd(patches(inp["x"], inp["C"], inp["P"]).double(), kind)
    W = inp["w"].double()
    bj = inp["bias"].double() if bias else torch.zeros(D, dtype=torch.float64)
    lin = X @ W.T + bj
    tok = lin + inp["pos"].double().repeat(B, 1)                    # unrounded, as rowpass_ref's outputs: see the docstring
    b = ulp_out(lin, kind) + (K + 2) * U * (X.abs() @ W.abs().T + bj.abs()) + 2 * U * tok.abs()
    return dict(tok=tok, b_tok=b, patches=[rnd(patches(inp["x"], inp["C"], inp["P"], o).double(), kind) for o in (0, 1)])


PATCH_MUTATIONS = ("order_pijc", "pos_neighbour", "no_bias", "x_unrounded")


def patch_restatement(inp, bias=True, mutation=None):
    """patch_embed_fwd_kernel / patch_embed_fwd16_kernel in fp32 torch: one chain over k from 0.0f in both.  mutation:
    order_pijc = the patch gathered in the (pi, pj, c) order; pos_neighbour = the positional row of token t + 1; no_bias;
    x_unrounded = x not rounded to the operand type."""
    assert mutation is None or mutation in PATCH_MUTATIONS
    kind, K, T, D, B = inp["kind"], inp["K"], inp["T"], inp["D"], inp["B"]
    dt = DTYPE[kind]
    x = patches(inp["x"], inp["C"], inp["P"], 1 if mutation == "order_pijc" else 0)
    if mutation != "x_unrounded":
        x = x.to(dt).float()
    w = inp["w"].float()
    acc = torch.zeros(B * T, D)
    for k in range(K):
        acc = acc + x[:, k:k + 1] * w[:, k]
    if bias and mutation != "no_bias":
        acc = acc + inp["bias"].float()
    t = torch.arange(B * T) % T
    if mutation == "pos_neighbour":
        t = (t + 1) % T
    return dict(tok=acc.to(dt).float() + inp["pos"][t])


# ------------------------------------------------------------------------------------------------------------ sinusoid
def sin_inputs(kind):
    return dict(t=torch.tensor(SIN_T, dtype=torch.float32), kind=kind)


def sin_reference(inp, dim, max_period):
    """out[b] = [cos(t f_k), sin(t f_k), (0 where dim is odd)], f_k = exp(-ln(max_period) k / half), half = dim // 2, in fp64 from the
    fp32 t.  The fp32 frequency: the exponent -ln(max_period) k / half, of size at most ln(max_period), takes three roundings (the
    constant, the product, the quotient): 3 ln(max_period) u relative in f; expf itself, the product t f and one spare: 4 u.
    cos and sin have slope at most 1, so that relative error times |arg| is the absolute error carried into the result; sinf /
    cosf themselves and the slack of the argument's last place: 4 u absolute on a result of size at most 1; the rounding to
    the operand type: ulp_out."""
    kind = inp["kind"]
    half = dim // 2
    B = len(inp["t"])
    f = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    arg = inp["t"].double()[:, None] * f
    out = torch.zeros(B, dim, dtype=torch.float64)
    out[:, :half], out[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
    e = arg.abs() * (4 + 3 * math.log(max_period)) * U + 4 * U
    b = ulp_out(out, kind)
    b[:, :half] += e
    b[:, half:2 * half] += e                                         # the odd column: an exact 0, budget = the subnormal spacing
    return dict(out=out, b_out=b)


SIN_MUTATIONS = ("swap_halves", "no_max_period", "half_minus_1", "odd_unwritten")


def sin_restatement(inp, dim, max_period, mutation=None):
    """sinusoid_kernel in fp32 torch.  mutation: swap_halves = sin first; no_max_period = max_period ignored, the exponent -k / half
    (as if it were e); half_minus_1 = the divisor half - 1; odd_unwritten = the last column of an odd dim left as it was (NaN)."""
    assert mutation is None or mutation in SIN_MUTATIONS
    half = dim // 2
    B = len(inp["t"])
    lg = torch.tensor(-1.0 if mutation == "no_max_period" else -math.log(max_period), dtype=torch.float32)
    a = lg * torch.arange(half, dtype=torch.float32)
    f = torch.exp(a / torch.tensor(float(half - 1 if mutation == "half_minus_1" else half)))
    arg = inp["t"][:, None] * f
    out = torch.full((B, dim), float("nan"))
    c, s = torch.cos(arg), torch.sin(arg)
    out[:, :half], out[:, half:2 * half] = (s, c) if mutation == "swap_halves" else (c, s)
    if dim % 2 and mutation != "odd_unwritten":
        out[:, dim - 1] = 0
    return dict(out=out.to(DTYPE[inp["kind"]]))


# -------------------------------------------------------------------------------------------------- label conditioning
def label_inputs(B, D, NC, kind, drop, seed=0):
    """labels with duplicates (label b = b // 2 mod NC: samples 0 and 1 share a row, 2 and 3, ...), a drop mask on every third
    sample from sample 2 on (or none; at B = 1 the one sample is dropped), a table of NC + 1 rows (the last one the null class), t_emb in the operand type, an upstream
    gradient dsilu (fp32) and a non-zero prior dtable.  c = t_emb + table[row] takes every value of C_SPECIAL: element j of the
    flat [B, D] array (as far as it reaches: 4 of them at B D = 4) has t_emb = the value and a zero table entry."""
    rn = _gen(seed + 2000 + D + B)
    labels = (torch.arange(B) // 2) % NC
    mask = (torch.arange(B) % 3 == (2 if B > 1 else 0)).to(torch.uint8) if drop else None    # B = 1: the one sample is dropped
    eff = torch.where(mask.bool(), torch.tensor(NC), labels) if drop else labels.clone()
    table, temb = rn(NC + 1, D).float(), rn(B, D)
    for j, v in enumerate(C_SPECIAL[:B * D]):
        b, d = j // D, j % D
        temb[b, d] = v
        table[eff[b], d] = 0
    return dict(labels=labels, drop=mask, eff=eff, table=table, t_emb=temb.to(DTYPE[kind]), dsilu=rn(B, D).float(),
                prior=rn(NC + 1, D).float(), B=B, D=D, NC=NC, kind=kind)


def _sig_terms(c):
    """fp64 sigmoid s of c and eps_s, the relative error bound of the kernel's s = rcp(1 + exp2(-log2(e) c)) in units of u:
    the exponent e = -log2(e) c carries the constant's rounding and the product's, 2 u relative, which is 2 u log2(e) |c| absolute
    and so 2 ln 2 log2(e) |c| u = 2 |c| u relative in E = 2**e; v_exp_f32 is good to 1 ulp = 2 u.  In 1 + E that error weighs
    E / (1 + E) = 1 - s; the addition rounds once (u) and v_rcp_f32 is good to 1 ulp (2 u):
        eps_s = (3 + (2 + 2 |c|) (1 - s)) u  <=  (5 + 2 |c|) u."""
    s = torch.sigmoid(c)
    one_minus = torch.sigmoid(-c)                                   # 1 - s without the cancellation
    return s, one_minus, 3 + (2 + 2 * c.abs()) * one_minus


def label_reference(inp):
    """labels_eff and c are exact (c is ONE fp32 addition of two fp32 values: the reference forms it the same way, budget 0).

    silu_c = r(c s):  eps_s (see _sig_terms) and the product's rounding, (6 + 2 |c|) u |silu|  [a = 6, b = 2, scale |silu(c)|];
        ulp_out for the rounding to the operand type.
    silu'(c) = s (1 + c (1 - s)):  1 - s is exact given s (Sterbenz for s >= 1/2, else one rounding u (1 - s)), so its error is s's
        own, eps_s s: the CANCELLATION, multiplied by c.  With S = s (1 + |c| (1 - s)) >= |silu'| (the sum of the two terms' sizes):
          |d silu'| <= (eps_s + 2 u) S               s's error through the outer product, the two roundings of 1 + . and s * .
                       + s |c| (eps_s s + 2 u (1 - s))  the cancellation and the roundings of 1 - s and c * .
                    <= ((7 + 2 |c|) + (3 |c| + 1.7) + 2) u S  =  (10.7 + 5 |c|) u S
        (s^2 <= S, and s (1 - s) |c| (2 + 2 |c|) <= 1.7 for every c: its maximum, at |c| = 1.62).  The product with r(dsilu) rounds
        once more:  (12 + 5 |c|) u |r(dsilu)| S  [a = 12, b = 5, scale |r(dsilu)| s (1 + |c| (1 - s))].
        dt_emb = r(g): ulp_out.
    The floor: v_exp_f32 and v_rcp_f32 return 0 for a result below 2**-126, an absolute error of up to 2**-126 in s (c = -88:
        s = e**-88 = 6.0e-39 comes out as 0; c = -100: exp2 overflows, rcp(inf) = 0, silu = -0).  silu multiplies it by |c|, silu'
        by at most 1 + |c| and the gradient by |r(dsilu)|; a product that is itself below 2**-126 may be flushed as well:
        floor = 2**-126 (1 + |c|) for silu_c and 2**-126 (1 + |c|) (1 + |r(dsilu)|) for the gradient.
    dtable[row] = prior + the g_b of the row's n samples in batch order, one fp32 chain that starts AT the prior value: every one of
        its n partial sums is bounded by |prior| + sum|g_b| and rounds by at most half an ulp of itself; a whole ulp is budgeted
        per addition (as for the rounding to the output type: the bound of a single rounding is attained), so
        2 n u (|prior| + sum|g_b|), plus each g_b's own error.  n <= B.
        A row that no sample selects is never touched: budget 0."""
    kind, B, D, NC = inp["kind"], inp["B"], inp["D"], inp["NC"]
    eff = inp["eff"]
    c32 = inp["t_emb"].float() + inp["table"][eff]
    c = c32.double()
    s, om, eps_s = _sig_terms(c)
    silu = c * s
    b_silu = ulp_out(silu, kind) + (6 + 2 * c.abs()) * U * silu.abs() + TINY * (1 + c.abs())
    dsr = rnd(inp["dsilu"].double(), kind)
    S = s * (1 + c.abs() * om)
    g = dsr * s * (1 + c * om)
    e_g = (12 + 5 * c.abs()) * U * dsr.abs() * S + TINY * (1 + c.abs()) * (1 + dsr.abs())
    prior = inp["prior"].double()
    hot = torch.zeros(NC + 1, B, dtype=torch.float64)
    hot[eff, torch.arange(B)] = 1
    n = hot.sum(1, keepdim=True)
    dtable = prior + hot @ g
    b_dtable = 2 * n * U * (prior.abs() * (n > 0) + hot @ g.abs()) + hot @ e_g
    return dict(eff=eff, c=c, b_c=torch.zeros_like(c), c32=c32, silu_c=silu, b_silu_c=b_silu, dt_emb=g, b_dt_emb=ulp_out(g, kind) + e_g,
                dtable=dtable, b_dtable=b_dtable, untouched=(n[:, 0] == 0))


LABEL_MUTATIONS = ("drop_not_null", "dsilu_unrounded", "dtable_overwrite", "batch_short")
LABEL_OUTPUTS = ("c", "silu_c", "dt_emb", "dtable")


def label_restatement(inp, mutation=None):
    """label_cond_kernel and label_cond_bwd_kernel in fp32 torch (sigmoid as 1 / (1 + exp2(-log2(e) c)), the kernels' form).
    mutation: drop_not_null = a dropped sample keeps its own label; dsilu_unrounded = dsilu not rounded to the operand type;
    dtable_overwrite = `=` for `+=`; batch_short = the batch loop stops one short (the last dt_emb row stays NaN)."""
    assert mutation is None or mutation in LABEL_MUTATIONS
    kind, B, D = inp["kind"], inp["B"], inp["D"]
    dt = DTYPE[kind]
    eff = inp["labels"].clone() if mutation == "drop_not_null" else inp["eff"]
    c = inp["t_emb"].float() + inp["table"][eff]
    sig = lambda v: 1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=torch.float32) * v))  # noqa: E731
    s = sig(c)
    silu = (c * s).to(dt)
    ds = inp["dsilu"] if mutation == "dsilu_unrounded" else inp["dsilu"].to(dt).float()
    g = ds * (s * (1.0 + c * (1.0 - s)))
    dt_emb = torch.full((B, D), float("nan"))
    dtable = inp["prior"].clone()
    for b in range(B - 1 if mutation == "batch_short" else B):
        dt_emb[b] = g[b]
        dtable[eff[b]] = g[b] if mutation == "dtable_overwrite" else dtable[eff[b]] + g[b]
    return dict(eff=eff, c=c, silu_c=silu, dt_emb=dt_emb.to(dt), dtable=dtable)
