"""fp64 references, error budgets and fp32 restatements for the adaLN row kernels (csrc/norm.hip: LayerNorm+modulate forward and
backward, the gate backward), the final layer (csrc/embed.hip) and the loss kernels (csrc/loss.hip).  A plain module, not a test
file, after the pattern of tests/rowpass_ref.py: tests/test_adaln_budgets_cpu.py proves the budgets on the CPU (the restatement
stays at or below 0.6 of them, every realistic bug leaves them), tests/test_adaln_gpu.py, test_final_layer_gpu.py and
test_loss_gpu.py hold the kernels to them.

Every fp64 reference starts from the operand-type inputs and the kernels' documented contract (include/reed_hip.h):
s1 = (1 + scale.float()).to(dt) is the kernels' bfround(1.f + a), an exact restatement without an error term; the gate backward
reads dg = dx.to(dt); fp64 from there on.  The backward kernels and final_layer_bwd_rows take mean / rstd as fp32 INPUTS: their
references use those very fp32 numbers, so no conditioning term enters a backward budget.

Budgets are bounds derived from the arithmetic (u = 2**-24, rowpass_ref.U), never from what a kernel delivers:
  * ulp_out(ref, kind) per rounding to the output type;
  * d u sum|terms| for a sum whose tree is d additions deep (depth() below);
  * the conditioning term of a small spread on a large mean (the mean's error times rstd), as rowpass_ref.qk_reference has it;
  * where a value is rounded to the operand type and then USED (dg = round(dx) in the gate backward, h = round(...) in the final
    layer's dot products), the rounding can flip when the value's own error carries it across a rounding boundary: the
    consumer's budget is taken from the interval [round(ref - budget), round(ref + budget)], which is a single point for
    most elements, not from a bit comparison and not from a whole ulp per element.
"""
import math

import torch

from tests.rowpass_ref import DTYPE, U, ulp_out, worst

LN_EPS = 1e-6
MAXV = 5                                         # float4 per lane (csrc/norm.hip): D <= 1280
BWD2 = {128: (0, 1), 256: (0, 2), 384: (0, 3), 512: (1, 0), 768: (1, 2), 1024: (2, 0), 1152: (2, 1)}   # D -> (NF, TS), REED_LNB2
# (B, T, D) of the GPU tests (tests/test_adaln_gpu.py); the CPU test proves the budgets at the same shapes
FWD_SHAPES = ((3, 7, 4), (3, 7, 260), (2, 16, 384), (2, 16, 1152), (1, 5, 1280))
BWD_WIDTHS = (128, 256, 384, 512, 768, 1024, 1152, 4, 200, 640, 1280)
BWD_SHAPES = tuple((B, T, D) for D in BWD_WIDTHS for B, T in ((3, 16), (2, 48)))
FINAL_SHAPES = tuple((B, T, D, C, P) for C, P in ((4, 2), (8, 2)) for D in (384, 1152) for B, T in ((3, 9), (5, 16), (1, 1)))
MSE_SHAPES = ((1, 1), (5, 255), (5, 4096), (2, 4097))
COS_SHAPES = ((5, 1, 4), (3, 7, 260), (2, 16, 768), (1, 300, 1024))
# Worst absolute error of the cosine path's four coefficients (cosf(t pi/2), sinf(t pi/2) and their derivatives' pi/2 multiples,
# csrc/loss.hip interpolant_kernel) against fp64 over t = 0, 1/1024, ..., 1, measured once on an MI355X through the kernel itself
# (x = 1, noise = 0 returns a and da; x = 0, noise = 1 returns s and ds; profiles/adaln_tests.txt): no document shipped with
# ROCm states an ULP bound for cosf / sinf.  The budget is twice the figure: the factor 2 covers an argument off the grid.
COSF_SINF_MEASURED = 1.988e-7          # da = -(pi / 2) sinf(t pi / 2) at t = 643 / 1024; the same in all three builds
COEF_ERR = 2 * COSF_SINF_MEASURED


def rnd(x, kind):
    """fp64 -> fp32 -> the build's operand type, as fp64: the kernels' f2bf / bfround of an fp32 value (monotone)."""
    return x.float().to(DTYPE[kind]).double()


def depth(D):
    """Additions between an element and its row sum in the deepest of the kernels' trees: a per-lane chain of 4 per float4,
    <= 4 ceil(D / 256) (norm.hip ln_mod_fwd_kernel `s += v[k][0] + v[k][1] + v[k][2] + v[k][3]`; the backward's chain over NE =
    D / 128 elements in ln_mod_bwd2_kernel `a1 += gy[e]` is shorter), the 6 butterfly steps of wave_sum (common.hpp), and 1
    for the two half-row sums exchanged through LDS (ln_mod_bwd2_kernel `a1 = (t[0] + t[2]) / D`)."""
    return 4 * -(-D // 256) + 7


def _gen(seed):
    g = torch.Generator().manual_seed(4321 + seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def _mod(rn, B, D, kind):
    """The engine's layout: one [B, 6 D + 8] array, shift / scale / gate at column offsets 0, D, 2 D (multiples of 4 elements:
    the fp32 build loads 16 bytes); a distinct vector per sample."""
    return (0.5 * rn(B, 6 * D + 8)).to(DTYPE[kind])


def _rows(rn, M, D):
    """x: per-row scale exp(N(0,1)) and offset; row 0 constant (variance 0: eps decides), the LAST row (in the last block) a tiny
    spread on a mean of 3.  A single row stays an ordinary one."""
    x = (rn(M, D) * torch.exp(rn(M, 1)) + 2.0 * rn(M, 1)).float()
    if M > 1:
        x[0] = 1.625
        x[M - 1] = (3.0 + 0.01 * rn(D)).float()
    return x


def _s1(scale, kind):
    return (1 + scale.float()).to(DTYPE[kind]).double()


def _per_row(v, T):
    return v.repeat_interleave(T, 0)


# ------------------------------------------------------------------------------------------- LayerNorm + modulate, forward
def ln_inputs(B, T, D, kind, seed=0):
    rn = _gen(seed)
    M = B * T
    x, mod = _rows(rn, M, D), _mod(rn, B, D, kind)
    return dict(x=x, mod=mod, shift=mod[:, :D], scale=mod[:, D:2 * D], gate=mod[:, 2 * D:3 * D], B=B, T=T, D=D, M=M, kind=kind)


def _ln_core(x, s1, sh):
    """fp64 LayerNorm + modulate of fp32 rows x [M, D] with per-row s1 / shift [M, D] (fp64).  Returns the unrounded output H, its
    error e_h BEFORE the rounding to the output type, the statistics and their budgets."""
    D = x.shape[1]
    d = depth(D)
    X = x.double()
    MEAN = X.mean(-1, keepdim=True)
    VAR = ((X - MEAN) ** 2).mean(-1, keepdim=True)
    R = 1.0 / torch.sqrt(VAR + LN_EPS)
    XH = (X - MEAN) * R
    H = XH * s1 + sh
    mabs = X.abs().mean(-1, keepdim=True)
    b_mean = (d + 2) * U * mabs                               # the tree, and the division by D
    # var + eps: the tree over the squares (each two roundings), the division and the addition: (d + 5) u relative; the mean's
    # error enters only in second order (sum (x - mu')^2 = sum (x - mu)^2 + D (mu' - mu)^2); rsqrtf: 2 u (one ulp)
    b_rstd = R * ((d + 5) / 2 * U + 2 * U + 0.5 * (R * b_mean) ** 2)
    dxh = R * b_mean + XH.abs() * (b_rstd / R + 3 * U)        # the conditioning term, and xhat's own roundings
    e_h = dxh * s1.abs() + 3 * U * ((XH * s1).abs() + sh.abs())
    return dict(H=H, e_h=e_h, XH=XH, mean=MEAN[:, 0], rstd=R[:, 0], b_mean=b_mean[:, 0], b_rstd=b_rstd[:, 0])


def ln_reference(inp):
    kind, T = inp["kind"], inp["T"]
    c = _ln_core(inp["x"], _per_row(_s1(inp["scale"], kind), T), _per_row(inp["shift"].double(), T))
    return dict(h=c["H"], b_h=ulp_out(c["H"], kind) + c["e_h"], mean=c["mean"], b_mean=c["b_mean"], rstd=c["rstd"],
                b_rstd=c["b_rstd"], cast=inp["x"].to(DTYPE[kind]))


def _lanes(v):
    """[..., D] -> [..., nk, 64, 4], zero-padded: element (k, lane, j) is column (lane + 64 k) * 4 + j, as the one-wave kernels own
    them."""
    D = v.shape[-1]
    nk = -(-D // 256)
    pad = torch.zeros(*v.shape[:-1], nk * 256 - D, dtype=v.dtype)
    return torch.cat([v, pad], -1).reshape(*v.shape[:-1], nk, 64, 4)


def _wave(c):
    """[..., 64] -> [...]: the butterfly of wave_sum."""
    n = 64
    while n > 1:
        n //= 2
        c = c[..., :n] + c[..., n:2 * n]
    return c[..., 0]


def _lane_sum(v, grouped=False):
    """fp32 row sum of [..., D] in the one-wave kernels' order: per lane a chain over its float4s (grouped: the four added first, as
    `s += v0 + v1 + v2 + v3`), then the butterfly.  Padded lanes add 0."""
    L = _lanes(v)
    s = torch.zeros_like(L[..., 0, :, 0])
    for k in range(L.shape[-3]):
        if grouped:
            s = s + (((L[..., k, :, 0] + L[..., k, :, 1]) + L[..., k, :, 2]) + L[..., k, :, 3])
        else:
            for j in range(4):
                s = s + L[..., k, :, j]
    return _wave(s)


def _ln_stats_f32(x, mutation=None):
    D = x.shape[1]
    Df = torch.tensor(float(D))
    mu = (_lane_sum(x, grouped=True) / Df)[:, None]
    dd = x - mu
    var = _lane_sum(dd * dd) / (Df - 1 if mutation == "biased_var" else Df)
    r = torch.rsqrt(var if mutation == "no_eps" else var + torch.tensor(LN_EPS))[:, None]
    return mu, r


LN_MUTATIONS = ("neighbour_sample", "biased_var", "no_eps")


def ln_restatement(inp, mutation=None):
    """ln_mod_fwd_kernel in fp32 torch."""
    assert mutation is None or mutation in LN_MUTATIONS
    kind, T, B = inp["kind"], inp["T"], inp["B"]
    x = inp["x"]
    mu, r = _ln_stats_f32(x, mutation)
    smp = torch.arange(inp["M"]) // T
    if mutation == "neighbour_sample":
        smp = (smp + 1) % B
    s1 = (1 + inp["scale"].float()).to(DTYPE[kind]).float()[smp]
    h = ((x - mu) * r * s1 + inp["shift"].float()[smp]).to(DTYPE[kind])
    return dict(h=h, mean=mu[:, 0], rstd=r[:, 0])


def ratios(got, ref, outputs):
    """{output: (worst error / budget, flat index)} of a result dict (tensors of any float type) against a reference dict."""
    return {k: worst((got[k].double().cpu() - ref[k]).abs(), ref["b_" + k]) for k in outputs if k in got}


# ------------------------------------------------------------------------- LayerNorm + modulate backward, gate backward
def bwd_inputs(B, T, D, kind, seed=0):
    """The forward's inputs plus dh, a non-zero dx0, the branch output y, and mean / rstd: the fp64 statistics rounded to fp32."""
    inp = ln_inputs(B, T, D, kind, seed + 100)
    rn = _gen(seed + 200)
    M = inp["M"]
    X = inp["x"].double()
    mean = X.mean(-1)
    rstd = 1.0 / torch.sqrt(((X - mean[:, None]) ** 2).mean(-1) + LN_EPS)
    inp.update(dh=(0.5 * rn(M, D)).to(DTYPE[kind]), dx0=rn(M, D).float(), y=rn(M, D).to(DTYPE[kind]), mean=mean.float(),
               rstd=rstd.float())
    return inp


def _chunks(v):
    """[M, D] -> [M / 16, D]: sums over the 16-row chunks."""
    return v.reshape(v.shape[0] // 16, 16, v.shape[1]).sum(1)


def _interval(lo, hi):
    return torch.minimum(lo, hi), torch.maximum(lo, hi)


def gate_reference(DX, b_dx, inp, frac=1.0):
    """dy = round(dg gate), part_g = chunk sums of round(dg y), part_dy = chunk sums of dy, with dg = round(dx), from a dx known
    to b_dx: each rounded product lies between its values at round(dx - b_dx) and round(dx + b_dx) (rounding and the fp32
    product are monotone; in the 16-bit builds the product of two operands is exact in fp32).  For most elements of a 16-bit
    build the interval is one point and the budget 0: the output must then have the reference's bits.
    A flip is all or nothing, so `error <= 0.6 budget` cannot be asked of these three outputs; frac = 0.6 gives the
    budgets that follow from a dx inside 0.6 of ITS budget (and 0.6 of the sums' own term), which is how the CPU test states
    the restatement's condition for them."""
    kind, T = inp["kind"], inp["T"]
    b_dx = frac * b_dx
    gate, y = _per_row(inp["gate"].double(), T), inp["y"].double()
    dg, dg_lo, dg_hi = rnd(DX, kind), rnd(DX - b_dx, kind), rnd(DX + b_dx, kind)
    out = {}
    for name, f in (("dy", gate), ("gy", y)):
        ref = rnd(dg * f, kind)
        lo, hi = _interval(rnd(dg_lo * f, kind), rnd(dg_hi * f, kind))
        out[name], out["b_" + name] = ref, torch.maximum(hi - ref, ref - lo)
    res = dict(dy=out["dy"], b_dy=out["b_dy"])
    for name, src in (("part_g", "gy"), ("part_dy", "dy")):
        res[name] = _chunks(out[src])
        res["b_" + name] = frac * 16 * U * _chunks(out[src].abs() + out["b_" + src]) + _chunks(out["b_" + src])
    return res


def bwd_reference(inp, frac=1.0):
    kind, T, D = inp["kind"], inp["T"], inp["D"]
    d = depth(D)
    s1 = _per_row(_s1(inp["scale"], kind), T)
    mu, R = inp["mean"].double()[:, None], inp["rstd"].double()[:, None]
    XH = (inp["x"].double() - mu) * R
    dxh = 3 * U * XH.abs()                                    # (x - mu) * r: two roundings, mu and r are inputs
    G = inp["dh"].double()
    GY = G * s1
    A1 = GY.mean(-1, keepdim=True)
    A2 = (GY * XH).mean(-1, keepdim=True)
    TERM = GY - A1 - XH * A2
    DX = inp["dx0"].double() + R * TERM
    da1 = (d + 3) * U * GY.abs().mean(-1, keepdim=True)
    da2 = (d + 4) * U * (GY * XH).abs().mean(-1, keepdim=True) + (GY.abs() * dxh).mean(-1, keepdim=True)
    e_term = da1 + XH.abs() * da2 + A2.abs() * dxh + 4 * U * (GY.abs() + A1.abs() + (XH * A2).abs())
    b_dx = R * e_term + 3 * U * (inp["dx0"].double().abs() + (R * TERM).abs())
    part = torch.stack([_chunks(G), _chunks(G * XH)], 1)      # [M / 16, 2, D]
    b_part = torch.stack([16 * U * _chunks(G.abs()), 20 * U * _chunks((G * XH).abs())], 1)
    res = dict(dx=DX, b_dx=b_dx, part=part, b_part=b_part)
    res.update(gate_reference(DX, b_dx, inp, frac))
    return res


def _half_sums(v, D):
    """fp32 sums of [M, D] as ln_mod_bwd2_kernel forms them: per half row, per lane a chain over its NE = 4 NF + TS elements in
    HalfRow's order, the butterfly; returns [M, 2] (the two halves, added by the caller)."""
    NF, TS = BWD2[D]
    NE = 4 * NF + TS
    lane = torch.arange(64)[:, None]
    cols = [(lane + 64 * (e // 4)) * 4 + e % 4 if e < 4 * NF else 256 * NF + 64 * (e - 4 * NF) + lane for e in range(NE)]
    idx = torch.cat(cols, 1)                                  # [64, NE]
    idx = torch.stack([idx, idx + 64 * NE])                   # [2, 64, NE]
    assert sorted(idx.flatten().tolist()) == list(range(D))
    L = v[:, idx]                                             # [M, 2, 64, NE]
    s = torch.zeros_like(L[..., 0])
    for e in range(NE):
        s = s + L[..., e]
    return _wave(s)


def _chunk_tree(c, drop_last=False):
    """[M, D] fp32 -> [M / 16, D]: a chain over the 4 rows of a row group from 0.0f, then ((g0 + g1) + g2) + g3."""
    c = c.reshape(c.shape[0] // 16, 4, 4, c.shape[1])
    s = torch.zeros_like(c[:, :, 0])
    for rr in range(4):
        if drop_last:
            s = torch.cat([s[:, :3] + c[:, :3, rr], s[:, 3:] + (c[:, 3:, rr] if rr < 3 else 0 * c[:, 3:, rr])], 1)
        else:
            s = s + c[:, :, rr]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


BWD_MUTATIONS = ("neighbour_sample", "half_sums", "dx_overwrite", "part_scaled", "part_15", "gate_unrounded")
BWD_OUTPUTS = ("dx", "part", "dy", "part_g", "part_dy")


def bwd_restatement(inp, mutation=None):
    """ln_mod_bwd2_kernel<GATE> (D in BWD2) or ln_mod_bwd_kernel<GATE> (every other D) in fp32 torch; ln_modulate_bwd followed by
    gate_bwd is the same arithmetic."""
    assert mutation is None or mutation in BWD_MUTATIONS
    kind, T, B, D, M = inp["kind"], inp["T"], inp["B"], inp["D"], inp["M"]
    dt = DTYPE[kind]
    smp = (torch.arange(M) // 16 * 16) // T                  # the sample of the block's first row
    if mutation == "neighbour_sample":
        smp = (smp + 1) % B
    s1 = (1 + inp["scale"].float()).to(dt).float()[smp]
    gate = inp["gate"].float()[smp]
    mu, r = inp["mean"][:, None], inp["rstd"][:, None]
    g = inp["dh"].float()
    xh = (inp["x"] - mu) * r
    gy = g * s1
    Df = torch.tensor(float(D))
    if D in BWD2:
        h1, h2 = _half_sums(gy, D), _half_sums(gy * xh, D)
        if mutation == "half_sums":
            a1, a2 = h1[:, :1] / Df, h2[:, :1] / Df
        else:
            a1, a2 = ((h1[:, 0] + h1[:, 1]) / Df)[:, None], ((h2[:, 0] + h2[:, 1]) / Df)[:, None]
    else:
        assert mutation != "half_sums", "the one-wave form has no exchange"
        a1, a2 = (_lane_sum(gy) / Df)[:, None], (_lane_sum(gy * xh) / Df)[:, None]
    add = r * (gy - a1 - xh * a2)
    dx = add if mutation == "dx_overwrite" else inp["dx0"] + add
    pin = gy if mutation == "part_scaled" else g
    part = torch.stack([_chunk_tree(pin, mutation == "part_15"), _chunk_tree(pin * xh, mutation == "part_15")], 1)
    dg = dx if mutation == "gate_unrounded" else dx.to(dt).float()
    dy = (dg * gate).to(dt)
    dg = dx.to(dt).float()
    part_g = _chunk_tree((dg * inp["y"].float()).to(dt).float())
    part_dy = _chunk_tree(dy.float())
    return dict(dx=dx, part=part, dy=dy, part_g=part_g, part_dy=part_dy)


# ------------------------------------------------------------------------------------------------------------ final layer
def unpatchify(lin, C, P):
    """[B, T, P P C] in the (pi, pj, c) order -> [B, C, G P, G P], T = G G row-major tokens (the public SiT unpatchify:
    x.reshape(n, h, w, p, p, c), einsum nhwpqc->nchpwq)."""
    B, T, _ = lin.shape
    G = math.isqrt(T)
    return lin.reshape(B, G, G, P, P, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, G * P, G * P)


def patchify_out(img, C, P):
    """The inverse of unpatchify: [B, C, HW, HW] -> [B, T, P P C]."""
    B, _, HW, _ = img.shape
    G = HW // P
    return img.reshape(B, C, G, P, G, P).permute(0, 2, 4, 3, 5, 1).reshape(B, G * G, P * P * C)


def final_form(kind, C, P, D, backward, aligned):
    """'lds' or 'rows': the size rules of reed_final_layer_fwd / reed_final_layer_bwd_rows (csrc/embed.hip) restated."""
    NO = P * P * C
    wb = NO * D * (4 if kind == "fp32" else 2)
    need = wb + (4 * NO * 4 if backward else 0)
    return "lds" if need <= 64 * 1024 and (NO * D) % 8 == 0 and aligned else "rows"


def final_inputs(B, T, D, C, P, kind, seed=0):
    rn = _gen(seed + 300)
    M, NO, HW = B * T, P * P * C, math.isqrt(T) * P
    x, mod = _rows(rn, M, D), _mod(rn, B, D, kind)
    X = x.double()
    mean = X.mean(-1)
    rstd = 1.0 / torch.sqrt(((X - mean[:, None]) ** 2).mean(-1) + LN_EPS)
    return dict(x=x, mod=mod, shift=mod[:, :D], scale=mod[:, D:2 * D], w=(0.05 * rn(NO, D)).to(DTYPE[kind]),
                bias=rn(NO).to(DTYPE[kind]), dout=rn(B, C, HW, HW).float(), mean=mean.float(), rstd=rstd.float(),
                B=B, T=T, D=D, C=C, P=P, M=M, NO=NO, HW=HW, kind=kind)


def final_reference(inp, bias=True):
    kind, T, D, C, P, B, NO = inp["kind"], inp["T"], inp["D"], inp["C"], inp["P"], inp["B"], inp["NO"]
    s1, sh = _per_row(_s1(inp["scale"], kind), T), _per_row(inp["shift"].double(), T)
    W = inp["w"].double()
    bj = inp["bias"].double() if bias else torch.zeros(NO, dtype=torch.float64)
    c = _ln_core(inp["x"], s1, sh)
    H, e = c["H"], c["e_h"]
    Hr = rnd(H, kind)
    flip = torch.maximum(rnd(H + e, kind) - Hr, Hr - rnd(H - e, kind))     # 0 unless H's error can carry it across a boundary
    LIN = Hr @ W.T + bj
    # the dot product: depth(D) additions deep, the products' roundings, the bias; then the second rounding
    b_lin = ulp_out(LIN, kind) + flip @ W.abs().T + (depth(D) + 3) * U * (Hr.abs() @ W.abs().T + bj.abs())
    res = dict(out=unpatchify(LIN.reshape(B, T, NO), C, P), b_out=unpatchify(b_lin.reshape(B, T, NO), C, P),
               mean=c["mean"], b_mean=c["b_mean"], rstd=c["rstd"], b_rstd=c["b_rstd"])
    # backward rows, from the fp32 mean / rstd inputs
    XH = (inp["x"].double() - inp["mean"].double()[:, None]) * inp["rstd"].double()[:, None]
    HB = XH * s1 + sh
    res.update(hbuf=HB, b_hbuf=ulp_out(HB, kind) + 4 * U * ((XH * s1).abs() + sh.abs()))
    dlin = rnd(patchify_out(inp["dout"].double(), C, P).reshape(-1, NO), kind)
    DH = dlin @ W
    res.update(dlin=dlin, dh=DH, b_dh=ulp_out(DH, kind) + NO * U * (dlin.abs() @ W.abs()))
    return res


FINAL_MUTATIONS = ("no_bias", "wrong_pair_sample", "neighbour_sample")
FINAL_OUTPUTS = ("out", "mean", "rstd", "hbuf", "dh")


def final_restatement(inp, bias=True, mutation=None):
    """final_fwd_kernel / final_fwd_lds_kernel and final_bwd_rows(_lds)_kernel in fp32 torch."""
    assert mutation is None or mutation in FINAL_MUTATIONS
    kind, T, D, C, P, B, NO, M = inp["kind"], inp["T"], inp["D"], inp["C"], inp["P"], inp["B"], inp["NO"], inp["M"]
    dt = DTYPE[kind]
    x, w = inp["x"], inp["w"].float()
    mu, r = _ln_stats_f32(x)
    row = torch.arange(M)
    smp = row // T
    if mutation == "wrong_pair_sample":                       # the second row of a pair (an odd row: 64-row groups) takes the first's
        smp = torch.where(row % 2 == 1, (row - 1) // T, smp)
    if mutation == "neighbour_sample":
        smp = (smp + 1) % B
    s1 = (1 + inp["scale"].float()).to(dt).float()[smp]
    sh = inp["shift"].float()[smp]
    h = ((x - mu) * r * s1 + sh).to(dt).float()
    L = _lanes(h[:, None, :] * w[None, :, :])                 # [M, NO, nk, 64, 4]
    acc = torch.zeros(M, NO, 64)
    for k in range(L.shape[2]):
        acc = acc + (((L[:, :, k, :, 0] + L[:, :, k, :, 1]) + L[:, :, k, :, 2]) + L[:, :, k, :, 3])
    lin = _wave(acc)
    if bias and mutation != "no_bias":
        lin = lin + inp["bias"].float()
    out = unpatchify(lin.to(dt).float().reshape(B, T, NO), C, P)
    hb = ((x - inp["mean"][:, None]) * inp["rstd"][:, None] * s1 + sh).to(dt)
    dlin = patchify_out(inp["dout"], C, P).reshape(M, NO).to(dt)
    dh = torch.zeros(M, D)
    for j in range(NO):
        dh = dh + dlin[:, j:j + 1].float() * w[j]
    return dict(out=out, mean=mu[:, 0], rstd=r[:, 0], hbuf=hb, dlin=dlin, dh=dh.to(dt))


# ------------------------------------------------------------------------------------------------------------------ loss
def mse_inputs(B, per, seed=0):
    """x / noise (out / target of the MSE), t with t = 0 and t = 1 among the samples, moments and eps of sample_posterior, a
    distinct gscale per sample.  The last element of every sample is large: a dropped per % 256 tail shows."""
    rn = _gen(seed + 400)
    x, n = rn(B, per).float(), rn(B, per).float()
    x[:, -1] = 4.0
    n[:, -1] = -3.0
    t = torch.rand(B, generator=torch.Generator().manual_seed(seed + 5), dtype=torch.float64).float()
    t[0] = 0.0
    t[B - 1] = 1.0 if B > 1 else 0.0
    return dict(x=x, n=n, t=t, t1=torch.ones(B), gs=(0.5 + torch.arange(B) * 0.37).float(), mom=rn(B, 2 * per).float(),
                eps=rn(B, per).float(), B=B, per=per, scale=float(torch.tensor(0.18215).float()), bias=0.25)


def mse_reference(inp):
    x, n, per = inp["x"].double(), inp["n"].double(), inp["per"]
    res = {}
    for pt, t in ((0, inp["t"]), (1, inp["t"]), (2, inp["t1"])):        # 2: the cosine path at t = 1 in every sample
        tt = t.double()[:, None]
        if pt == 0:
            a, s, da, ds, ce = 1 - tt, tt, -torch.ones_like(tt), torch.ones_like(tt), 0.0
        else:
            hp = math.pi / 2
            a, s, da, ds, ce = torch.cos(tt * hp), torch.sin(tt * hp), -hp * torch.sin(tt * hp), hp * torch.cos(tt * hp), COEF_ERR
        res[f"xt{pt}"], res[f"tg{pt}"] = a * x + s * n, da * x + ds * n
        # each coefficient to ce (linear path: one rounding of 1 - t), two products, one addition
        res[f"b_xt{pt}"] = (ce + U) * (x.abs() + n.abs()) + 3 * U * ((a * x).abs() + (s * n).abs())
        res[f"b_tg{pt}"] = ce * (x.abs() + n.abs()) + 3 * U * ((da * x).abs() + (ds * n).abs())
    d2 = (x - n) ** 2
    res["mse"] = d2.mean(1)
    # per thread a chain of ceil(per / 256) squares (loss.hip mse_fwd_kernel `s += d * d`), 6 butterfly steps, 3 additions over the
    # waves, the difference and the square (3 u), the division
    res["b_mse"] = (-(-per // 256) + 6 + 3 + 4) * U * res["mse"]
    res["dout"] = inp["gs"].double()[:, None] * 2 * (x - n) / per
    # gs * 2 is exact; the division, the difference and the product: three roundings, and two more for a division formed as a
    # reciprocal and a product
    res["b_dout"] = 5 * U * res["dout"].abs()
    half = per
    mom = inp["mom"].double()
    mean, sd = mom[:, :half], mom[:, half:]
    res["post"] = (mean + sd * inp["eps"].double()) * inp["scale"] + inp["bias"]
    res["b_post"] = 4 * U * ((mean.abs() + (sd * inp["eps"].double()).abs()) * abs(inp["scale"]) + abs(inp["bias"]))
    return res


MSE_MUTATIONS = ("mse_tail", "mse_no_2")


def mse_restatement(inp, mutation=None):
    x, n, per, B = inp["x"], inp["n"], inp["per"], inp["B"]
    res = {}
    hp = torch.tensor(1.5707963267948966)
    for pt, t in ((0, inp["t"]), (1, inp["t"]), (2, inp["t1"])):
        tt = t[:, None]
        if pt == 0:
            a, s, da, ds = 1 - tt, tt, -torch.ones_like(tt), torch.ones_like(tt)
        else:
            a, s, da, ds = torch.cos(tt * hp), torch.sin(tt * hp), -hp * torch.sin(tt * hp), hp * torch.cos(tt * hp)
        res[f"xt{pt}"], res[f"tg{pt}"] = a * x + s * n, da * x + ds * n
    d = x - n
    d2 = d * d
    if mutation == "mse_tail":
        d2 = d2[:, :per - per % 256]
    pad = torch.zeros(B, -(-per // 256) * 256 - d2.shape[1])
    c = torch.cat([d2, pad], 1).reshape(B, -1, 4, 64)          # thread i owns elements i, i + 256, ...
    s = torch.zeros(B, 4, 64)
    for k in range(c.shape[1]):
        s = s + c[:, k]
    wv = _wave(s)
    res["mse"] = (((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]) / torch.tensor(float(per))
    g = inp["gs"] * (1.0 if mutation == "mse_no_2" else 2.0) / torch.tensor(float(per))
    res["dout"] = g[:, None] * d
    res["post"] = (inp["mom"][:, :per] + inp["mom"][:, per:] * inp["eps"]) * torch.tensor(inp["scale"]) + torch.tensor(inp["bias"])
    return res


MSE_OUTPUTS = ("xt0", "tg0", "xt1", "tg1", "xt2", "tg2", "mse", "dout", "post")


def cos_inputs(B, T, Z, kind, seed=0):
    """zt (the projector output, operand type) and z (fp32) with a per-row scale; one all-zero zt row and one all-zero z row (the
    1e-12 clamps decide), in different samples where there are two; a distinct gscale per sample."""
    rn = _gen(seed + 500)
    M = B * T
    zt = (rn(M, Z) * torch.exp(0.5 * rn(M, 1))).to(DTYPE[kind])
    z = (rn(M, Z) * torch.exp(0.5 * rn(M, 1))).float()
    zero_zt, zero_z = M - 1, (M // 2 if M > 2 else 0)
    zt[zero_zt] = 0
    z[zero_z] = 0
    return dict(zt=zt, z=z, gs=(0.5 + torch.arange(B) * 0.37).float(), B=B, T=T, Z=Z, M=M, kind=kind, zero_zt=zero_zt, zero_z=zero_z)


def cos_reference(inp):
    """The analytic fp64 cosine alignment and its gradient (tests/test_adaln_budgets_cpu.py holds it to autograd through
    F.normalize(., dim=-1, eps=1e-12) in fp64)."""
    kind, B, T, Z = inp["kind"], inp["B"], inp["T"], inp["Z"]
    a, b = inp["zt"].double(), inp["z"].double()
    # per lane a chain of 4 ceil(Z / 256) products (loss.hip cosine_rows_kernel `dot += av * b[j]`), 6 butterfly steps, the products
    dc = 4 * -(-Z // 256) + 6 + 2
    nt = a.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    nz = b.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    cosv = (a * b).sum(-1, keepdim=True) / (nt * nz)
    # the dot product's tree; each norm: half the tree's relative error and the square root; two products and a division
    b_row = dc * U * (a * b).abs().sum(-1, keepdim=True) / (nt * nz) + (dc + 6) * U * cosv.abs()
    rows = cosv.reshape(B, T)
    loss = -rows.mean(1)
    b_loss = b_row.reshape(B, T).mean(1) + (-(-T // 256) + 6 + 3 + 2) * U * rows.abs().mean(1)
    g = -_per_row(inp["gs"].double(), T)[:, None] / T / nt
    dzt = g * (b / nz - cosv * a / nt)
    b_dzt = ulp_out(dzt, kind) + g.abs() * ((dc + 8) * U * (b.abs() / nz + cosv.abs() * a.abs() / nt) + b_row * a.abs() / nt)
    return dict(rowdot=cosv[:, 0], b_rowdot=b_row[:, 0], loss=loss, b_loss=b_loss, dzt=dzt, b_dzt=b_dzt)


COS_MUTATIONS = ("z_tail", "no_clamp", "cos_wrong_sample")
COS_OUTPUTS = ("rowdot", "loss", "dzt")


def cos_restatement(inp, mutation=None):
    assert mutation is None or mutation in COS_MUTATIONS
    kind, B, T, Z, M = inp["kind"], inp["B"], inp["T"], inp["Z"], inp["M"]
    a, b = inp["zt"].float(), inp["z"]
    an, bn = (a[:, :256], b[:, :256]) if mutation == "z_tail" else (a, b)
    dot, n1, n2 = _lane_sum(a * b), _lane_sum(an * an), _lane_sum(bn * bn)
    lo = torch.tensor(0.0 if mutation == "no_clamp" else 1e-12)
    nt, nz = torch.maximum(torch.sqrt(n1), lo), torch.maximum(torch.sqrt(n2), lo)
    rowdot = dot / (nt * nz)
    pad = torch.zeros(B, -(-T // 256) * 256 - T)
    c = torch.cat([rowdot.reshape(B, T), pad], 1).reshape(B, -1, 4, 64)
    s = torch.zeros(B, 4, 64)
    for k in range(c.shape[1]):
        s = s + c[:, k]
    wv = _wave(s)
    loss = -(((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]) / torch.tensor(float(T))
    smp = torch.arange(M) // T
    if mutation == "cos_wrong_sample":
        smp = (smp + 1) % B
    g = (-inp["gs"][smp] / torch.tensor(float(T)) / nt)[:, None]
    dzt = (g * (b / nz[:, None] - rowdot[:, None] * a / nt[:, None])).to(DTYPE[kind])
    return dict(rowdot=rowdot, loss=loss, dzt=dzt)


def cos_ratios(got, ref, inp):
    """ratios() for the cosine outputs.  Where the fp64 gradient overflows the operand type (the clamp rows: O(1 / eps)), the output
    must be the infinity of the same sign: those elements are compared by value, the rest against the budget."""
    res = {k: worst((got[k].double().cpu() - ref[k]).abs(), ref["b_" + k]) for k in ("rowdot", "loss") if k in got}
    if "dzt" in got:
        want = rnd(ref["dzt"], inp["kind"])
        over = torch.isinf(want)
        g = got["dzt"].double().cpu()
        err = torch.where(over, torch.where(g == want, 0.0, float("inf")), (g - ref["dzt"]).abs())
        res["dzt"] = worst(err, torch.where(over, torch.ones_like(want), ref["b_dzt"]))
    return res
