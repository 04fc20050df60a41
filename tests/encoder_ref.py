"""fp64 references, error budgets and fp32 restatements for the frozen encoders' row kernels (csrc/encoder.hip: ln_affine_bf16 /
ln_affine_f32, clip_im2col, clip_tokens, vit_tokens, preprocess_image).  A plain module, not a test file, after the pattern of
tests/rowpass_ref.py and tests/adaln_ref.py: tests/test_encoder_budgets_cpu.py proves the budgets on the CPU (each restatement
stays at or below 0.6 of them, every realistic bug leaves them), tests/test_encoder_rows_gpu.py holds the kernels to them in all
three builds.

Budgets are BOUNDS derived from the arithmetic of encoder.hip (u = 2**-24, rowpass_ref.U), never from what a kernel delivers:
  * ulp_out(ref, kind) per rounding to the operand type;
  * d u sum|terms| for a sum whose tree is d additions deep (ln_depth() below);
  * the conditioning term of a small spread on a large mean (the mean's error times rstd), as adaln_ref._ln_core has it;
  * token assembly and im2col are gathers with at most one fp32 addition and no product: the same fp32 chain on the CPU is the
    reference and the comparison is bit for bit (the rule tests/test_reductions_gpu.py states), written here as a budget of 0;
  * bicubic resampling: a coordinate term (through the interpolant's Lipschitz constant), a coefficient term (the Horner
    evaluation of the cubics) and a sum term, each derived at pre_reference.
"""
import math
from fractions import Fraction

import torch

from tests.rowpass_ref import DTYPE, KINDS, U, ulp_out, worst  # noqa: F401  (KINDS, worst: re-exported to the two test files)

F32 = torch.float32
F64 = torch.float64


def _gen(seed):
    g = torch.Generator().manual_seed(8642 + seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=F64)


def f32(v):
    """A Python number as the fp32 the C ABI receives (float arguments and ctypes.c_float arrays round to nearest)."""
    return float(torch.tensor(v, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_MAXC = 4                                     # 16-byte chunks per lane (encoder.hip): D <= 64 * 8 * 4 = 2048
LN_WIDTHS = ((5, 8), (37, 384), (4, 512), (6, 1024), (5, 1280), (3, 1536), (1, 2048))    # (M, D) of the GPU tests
LN_EPS = {"bf16": 1e-5, "f32": 1e-6}            # the entry point's default: CLIP's LayerNorm / the ViT towers'
# (entry point, output is fp32, ldo - D): reed_ln_affine_bf16 reads and writes the operand type; reed_ln_affine_f32 reads fp32
LN_FORMS = (("bf16", False, 0), ("f32", False, 0), ("f32", True, 0), ("f32", False, 8), ("f32", True, 8))
LN_GAP_WIDTHS = (384, 1280)                     # the widths that also run with ldo = D + 8


def ln_cases():
    """Every (M, D, entry, out_f32, gap) the GPU test runs and the CPU test proves."""
    return [(M, D, e, of, gap) for e, of, gap in LN_FORMS for M, D in LN_WIDTHS if gap == 0 or D in LN_GAP_WIDTHS]


def ln_depth(D):
    """Additions between an element and its row sum in ln_affine_kernel: a per-lane chain of 8 per 16-byte chunk over
    ceil(D / 512) chunks (`for j: s += v[k][j]`), then the 6 butterfly steps of wave_sum (common.hpp)."""
    return 8 * -(-D // 512) + 6


def _rows(rn, M, D):
    """adaln_ref._rows: per-row scale exp(N(0,1)) and offset; row 0 constant (variance 0: eps decides, the output is b), the LAST
    row a spread of 0.01 on a mean of 3.  A single row stays an ordinary one."""
    x = (rn(M, D) * torch.exp(rn(M, 1)) + 2.0 * rn(M, 1)).float()
    if M > 1:
        x[0] = 1.625
        x[M - 1] = (3.0 + 0.01 * rn(D)).float()
    return x


def ln_inputs(M, D, kind, entry, seed=0):
    """x as the kernel reads it: operand-type rows for ln_affine_bf16 (entry 'bf16'), fp32 rows for ln_affine_f32 ('f32'); distinct
    fp32 affine vectors.  eps is the fp32 number the entry point receives."""
    assert D % 8 == 0 and D <= 512 * LN_MAXC
    rn = _gen(seed + 7 * D + M)
    x = _rows(rn, M, D)
    if entry == "bf16":
        x = x.to(DTYPE[kind])
    w, b = (1 + 0.3 * rn(D)).float(), (0.2 * rn(D)).float()
    return dict(x=x, w=w, b=b, M=M, D=D, kind=kind, entry=entry, eps=f32(LN_EPS[entry]))


def ln_reference(inp, out_f32):
    """fp64 LayerNorm (biased variance, the call's eps, fp32 w / b) of the rows as read, and its budget: the structure of
    adaln_ref._ln_core with this kernel's tree depth and eps, w in place of 1 + scale and b in place of shift."""
    D, kind = inp["D"], inp["kind"]
    d = ln_depth(D)
    X, W, B = inp["x"].double(), inp["w"].double(), inp["b"].double()
    MEAN = X.mean(-1, keepdim=True)
    VAR = ((X - MEAN) ** 2).mean(-1, keepdim=True)
    R = 1.0 / torch.sqrt(VAR + inp["eps"])
    XH = (X - MEAN) * R
    OUT = XH * W + B
    mabs = X.abs().mean(-1, keepdim=True)
    b_mean = (d + 2) * U * mabs                               # the tree, and the division by D
    # var + eps: the tree over the squares (each two roundings), the division and the addition: (d + 5) u relative; the mean's
    # error enters only in second order (sum (x - mu')^2 = sum (x - mu)^2 + D (mu' - mu)^2); rsqrtf: 2 u (one ulp)
    b_rstd = R * ((d + 5) / 2 * U + 2 * U + 0.5 * (R * b_mean) ** 2)
    dxh = R * b_mean + XH.abs() * (b_rstd / R + 3 * U)        # the conditioning term, and xhat's own roundings
    b_out = dxh * W.abs() + 3 * U * ((XH * W).abs() + B.abs())   # the affine: a product and an addition (3 u budgeted, as adaln_ref)
    if not out_f32:
        b_out = b_out + ulp_out(OUT, kind)                    # the rounding to the operand type; the fp32-out form has none
    return dict(out=OUT, b_out=b_out, mean=MEAN[:, 0], rstd=R[:, 0])


def _lanes8(v):
    """[..., D] -> [..., nk, 64, 8], zero-padded to the next multiple of 512: element (k, lane, j) is column (lane + 64 k) * 8 + j, as
    ln_affine_kernel's lanes own them."""
    D = v.shape[-1]
    width = -(-D // 512) * 512
    pad = torch.zeros(*v.shape[:-1], width - D, dtype=v.dtype)
    return torch.cat([v, pad], -1).reshape(*v.shape[:-1], width // 512, 64, 8)


def _wave(c):
    """[..., 64] -> [...]: the butterfly of wave_sum (offsets 32, 16, ..., 1)."""
    n = 64
    while n > 1:
        n //= 2
        c = c[..., :n] + c[..., n:2 * n]
    return c[..., 0]


def _lane_sum8(v):
    """fp32 row sum in ln_affine_kernel's order: per lane one chain over its chunks' 8 elements, then the butterfly."""
    L = _lanes8(v)
    s = torch.zeros_like(L[..., 0, :, 0])
    for k in range(L.shape[-3]):
        for j in range(8):
            s = s + L[..., k, :, j]
    return _wave(s)


LN_MUTATIONS = ("eps", "var_unbiased", "neighbour_row", "wb_prev_chunk", "dead_lanes", "mean_padded")


def ln_restatement(inp, out_f32, mutation=None):
    """ln_affine_kernel<XF, OF> in fp32 torch.  mutation: one of LN_MUTATIONS = a realistic bug of exactly this kernel."""
    assert mutation is None or mutation in LN_MUTATIONS
    D, kind = inp["D"], inp["kind"]
    x = inp["x"].float()
    w, b = inp["w"], inp["b"]
    padded = -(-D // 512) * 512
    Df = torch.tensor(float(padded if mutation == "mean_padded" else D))
    mu = (_lane_sum8(x) / Df)[:, None]
    dd = x - mu
    if mutation == "dead_lanes":                  # `if (lane + 64 * k < nch)` removed: the ragged chunk's idle lanes add (0 - mu)^2
        dd = torch.cat([dd, (0.0 - mu).expand(-1, padded - D)], -1)
    var = _lane_sum8(dd * dd) / (torch.tensor(float(D - 1)) if mutation == "var_unbiased" else torch.tensor(float(D)))
    eps = inp["eps"]
    if mutation == "eps":
        eps = f32(LN_EPS["f32" if inp["entry"] == "bf16" else "bf16"])
    r = torch.rsqrt(var + torch.tensor(eps))[:, None]
    if mutation == "neighbour_row":
        mu, r = mu.roll(1, 0), r.roll(1, 0)
    if mutation == "wb_prev_chunk":               # chunk k >= 1 reads w / b at (lane + 64 (k - 1)) * 8 + j
        col = torch.arange(D)
        col = torch.where(col >= 512, col - 512, col)
        w, b = w[col], b[col]
    y = (x - mu) * r * w + b
    return dict(out=y if out_f32 else y.to(DTYPE[kind]))


# ----------------------------------------------------------------------------------------------------------- token assembly
TOK_SHAPES = ((3, 5, 128), (2, 2, 8), (1, 17, 1280))          # (B, T, D) of clip_tokens: one class row and T - 1 patch rows
VIT_PREFIXES = (0, 1, 5)


def vit_shapes():
    """(B, T, D, nprefix) of vit_tokens: the patch rows of each TOK_SHAPES entry behind 0, 1 and 5 prefix rows, T = T_clip - 1 +
    nprefix, so that T > nprefix throughout (and nprefix = 1 is CLIP's shape itself)."""
    return [(B, T - 1 + n, D, n) for B, T, D in TOK_SHAPES for n in VIT_PREFIXES]


def tok_inputs(B, T, D, kind, nprefix, seed=0):
    """patches [B (T - nprefix), D] in the operand type, fp32 prefix rows cls [nprefix, D] (CLIP: one) and pos [T, D], every pos
    row non-zero and distinct.  The values carry more bits than the operand type, so a missing rounding shows."""
    rn = _gen(seed + 100 + T + D + nprefix)
    return dict(patches=rn(B * (T - nprefix), D).to(DTYPE[kind]), cls=rn(max(nprefix, 1), D).float()[:nprefix],
                pos=(rn(T, D) + 0.5).float(), B=B, T=T, D=D, nprefix=nprefix, kind=kind)


CLIP_TOK_MUTATIONS = ("cls_unrounded", "patch_row_t", "batch_stride_T")
VIT_TOK_MUTATIONS = ("patch_row_t", "prefix_pos0", "batch_stride_T")


def _assemble(inp, prefix, pos, mutation):
    """[prefix rows | patch rows] + pos in fp32: one addition per element, in the kernels' own operand order."""
    B, T, D, n = inp["B"], inp["T"], inp["D"], inp["nprefix"]
    P = inp["patches"].float()
    t = torch.arange(n, T)
    bb = torch.arange(B)[:, None]
    row = bb * (T if mutation == "batch_stride_T" else T - n) + (t if mutation == "patch_row_t" else t - n)[None, :]
    body = P[row % P.shape[0]]                    # a read past the array stands for whatever lies behind it
    pre = prefix[None].expand(B, n, D)
    ppos = pos.clone()
    if mutation == "prefix_pos0":
        ppos[:n] = pos[0]
    return torch.cat([pre, body], 1) + ppos[None]


def clip_tokens_reference(inp, mutation=None):
    """clip_tokens_kernel: bf2f(v) + bfround(pos), rounded once; cls and pos are rounded to the operand type BEFORE the addition
    (clip_vit.py's eager-mode casts).  The sum of two operand-type numbers in fp32, then one rounding: the same chain here has the
    same bits, so this is both the reference and the restatement."""
    assert inp["nprefix"] == 1 and (mutation is None or mutation in CLIP_TOK_MUTATIONS)
    dt = DTYPE[inp["kind"]]
    cls = inp["cls"] if mutation == "cls_unrounded" else inp["cls"].to(dt).float()
    return _assemble(inp, cls, inp["pos"].to(dt).float(), mutation).to(dt)


def vit_tokens_reference(inp, mutation=None):
    """vit_tokens_kernel: fp32 prefix row or float(patch), plus the fp32 pos row: one fp32 addition, bit for bit."""
    assert mutation is None or mutation in VIT_TOK_MUTATIONS
    return _assemble(inp, inp["cls"], inp["pos"], mutation)


def exact_ratio(got, want):
    """worst() for a bit-for-bit contract: the budget is 0, so any differing element (a NaN included) is infinitely far outside.
    -0.0 against +0.0 counts as a difference too."""
    g, w = got.double().flatten(), want.double().flatten()
    assert g.shape == w.shape
    if g.numel() == 0:
        return 0.0, -1
    err = (g - w).abs()
    err = torch.where(torch.signbit(g) != torch.signbit(w), torch.full_like(err, float("inf")), err)
    return worst(err, torch.zeros_like(err))


# ------------------------------------------------------------------------------------------------------------------- im2col
IM2COL_SHAPES = ((2, 28, 14, 592), (2, 28, 14, 640), (1, 32, 16, 768), (3, 6, 2, 16))      # (B, S, P, Kp)
IM2COL_MUTATIONS = ("swap_py_px", "order_py_px_c", "pad_unwritten")


def im2col_inputs(B, S, P, Kp, seed=0):
    return dict(img=_gen(seed + 200 + S + Kp)(B, 3, S, S).float(), B=B, S=S, P=P, Kp=Kp)


def im2col_reference(inp, kind, mutation=None):
    """Row (b, gy, gx), column c P P + py P + px = the operand-type rounding of img[b, c, gy P + py, gx P + px]; columns 3 P P .. Kp
    exactly +0.  pad_unwritten leaves them at the NaN the tests pre-fill."""
    assert mutation is None or mutation in IM2COL_MUTATIONS
    B, S, P, Kp = inp["B"], inp["S"], inp["P"], inp["Kp"]
    G, K = S // P, 3 * P * P
    v = inp["img"].reshape(B, 3, G, P, G, P)      # b, c, gy, py, gx, px
    perm = {None: (0, 2, 4, 1, 3, 5), "pad_unwritten": (0, 2, 4, 1, 3, 5), "swap_py_px": (0, 2, 4, 1, 5, 3),
            "order_py_px_c": (0, 2, 4, 3, 5, 1)}[mutation]
    out = torch.full((B * G * G, Kp), float("nan") if mutation == "pad_unwritten" else 0.0, dtype=DTYPE[kind])
    out[:, :K] = v.permute(*perm).reshape(B * G * G, K).to(DTYPE[kind])
    return out


# --------------------------------------------------------------------------------------------------------------- preprocess
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
ODD_MEAN, ODD_STD = (0.1, 0.5, 0.9), (0.2, 0.5, 1.25)          # three clearly different per-channel values
# (B, R, S, order); 16 -> 16 takes the kernel's S == R branch (no resampling); 8 -> 12 is upsampling: negative source coordinates
# and taps two outside the image at both edges
PRE_SHAPES = ((2, 16, 16, 0), (2, 16, 16, 1), (2, 16, 8, 0), (2, 16, 14, 0), (2, 16, 14, 1), (1, 8, 12, 1))
PRE_CASES = tuple(s + (CLIP_MEAN, CLIP_STD) for s in PRE_SHAPES) + ((2, 16, 14, 1, ODD_MEAN, ODD_STD), (2, 16, 14, 0, ODD_MEAN, ODD_STD))
CUBIC_A = -0.75
ULP1 = 2 * U                                    # a whole fp32 ulp (relative, at the bottom of a binade): see pre_reference


def _cubic(t, A=CUBIC_A):
    """The four cubic-convolution weights at fraction t (taps -1, 0, 1, 2), in t's own precision and the kernel's Horner form."""
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    outer = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A          # noqa: E731
    inner = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0                # noqa: E731
    return torch.stack([outer(x0), inner(x1), inner(x2), outer(x3)], -1)


def _cubic_slopes():
    """(L, LAMBDA) = sup over t in [0, 1] of sum_j |c_j'(t)| and of sum_j |c_j(t)|, on a grid of 2^20 + 1 points in fp64."""
    A = CUBIC_A
    t = torch.linspace(0.0, 1.0, 2 ** 20 + 1, dtype=F64)
    d_outer = lambda x: A * (3 * x * x - 10 * x + 8)                          # noqa: E731
    d_inner = lambda x: 3 * (A + 2) * x * x - 2 * (A + 3) * x                 # noqa: E731
    slope = d_outer(t + 1).abs() + d_inner(t).abs() + d_inner(1 - t).abs() + d_outer(2 - t).abs()
    return float(slope.max()), float(_cubic(t).abs().sum(-1).max())


# L = 3.0 (at t = 1/2: 0.1875 + 1.3125 + 1.3125 + 0.1875) and LAMBDA = 1.375 (at t = 1/2: 2 * 0.09375 + 2 * 0.59375) for A = -0.75
CUBIC_L, CUBIC_LAMBDA = _cubic_slopes()
# Absolute error of one weight from its fp32 Horner evaluation, by a running error analysis over x in [1, 2] (outer taps) and
# [0, 1] (inner taps), every operation rounded (a contraction to fma only removes roundings):
#   outer ((A x - 5A) x + 8A) x - 4A: |A x| <= 1.5, |. - 5A| <= 3, |. x| <= 4.5, |. + 8A| <= 3, |. x| <= 3: the error grows
#     1.5 u -> 4.5 u -> 2 * 4.5 u + 4.5 u = 13.5 u -> 16.5 u -> 2 * 16.5 u + 3 u = 36 u (= 6 u times the largest intermediate
#     8|A| = 6) -> 36.1 u; its argument t + 1 or 2 - t is rounded too (<= u, times |c'| <= 0.75): 37 u in all;
#   inner ((A+2) x - (A+3)) x x + 1: 1.25 u -> 3.5 u -> 4.5 u -> 5.5 u -> 6.5 u; the argument 1 - t: u/2 times |c'| <= 1.32: 8 u.
COEF_ERR = torch.tensor([37.0, 8.0, 8.0, 37.0], dtype=F64) * U


def pre_inputs(B, R, seed=0):
    """Random uint8 images; with B > 1 image 1 is a 0 / 255 checkerboard: the largest overshoot the taps can see."""
    g = torch.Generator().manual_seed(97 + seed + R + B)
    raw = torch.randint(0, 256, (B, 3, R, R), generator=g, dtype=torch.uint8)
    if B > 1:
        yy, xx = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
        raw[1] = (((yy + xx) % 2) * 255).to(torch.uint8)
    return dict(raw=raw, B=B, R=R)


def _src_exact(R, S):
    """Per destination index the exact source coordinate (dst + 0.5) R / S - 0.5 as a rational: (floor, fraction as fp64)."""
    fl, fr = [], []
    for d in range(S):
        c = Fraction((2 * d + 1) * R, 2 * S) - Fraction(1, 2)
        i = math.floor(c)
        fl.append(i), fr.append(float(c - i))
    return torch.tensor(fl), torch.tensor(fr, dtype=F64)


def _is_f32(fr):
    return Fraction(f32(float(fr))) == fr


def coord_err(R, S):
    """Bound on |fp32 coordinate - exact coordinate| per destination index, as preprocess_image_kernel forms it:
    scale = (float)R / (float)S (correctly rounded, <= u relative; 2 u budgeted), scale * (dst + 0.5f) (dst + 0.5 is exact; the
    product rounds: u |product|), - 0.5f (u |result|; under fma contraction this is the only rounding of the two), and the
    fraction ry - floor(ry), exact for ry >= 0 but rounded where ry is in (-1, 0) (the result is in [0.5, 1): u / 2; u budgeted).
    Where R / S, every product and every coordinate are fp32 numbers (16 -> 8: scale 2, coordinates 2 dst + 0.5) nothing rounds
    and the term is exactly 0."""
    sc = Fraction(R, S)
    prods = [sc * Fraction(2 * d + 1, 2) for d in range(S)]
    if _is_f32(sc) and all(_is_f32(p) and _is_f32(p - Fraction(1, 2)) and p >= Fraction(1, 2) for p in prods):
        return torch.zeros(S, dtype=F64)
    p = torch.tensor([float(q) for q in prods], dtype=F64)
    return 2 * U * p + U * p + U * (p - 0.5).abs() + U


def _taps(idx, R, lo, hi):
    """[S] floor indices -> [S, hi - lo + 1] tap indices idx + lo .. idx + hi, clamped to the image."""
    return (idx[:, None] + torch.arange(lo, hi + 1)[None, :]).clamp(0, R - 1)


def pre_reference(inp, S, order, mean, std):
    """fp64 preprocess: x / 255, bicubic (A = -0.75, clamped taps, exact rational coordinates), (x - mean) / std with the fp32 mean
    and std the kernel receives.  order 0 normalises after the resampling and order 1 before it; the weights sum to 1, so in exact
    arithmetic the two are ONE function and one reference serves both (a swapped order is therefore not a detectable bug; only
    the budget knows the order, because the roundings fall on different magnitudes).

    The budget of one output, from the code of preprocess_image_kernel.  p is the pixel as the taps see it: x / 255 for order 0,
    (x / 255 - mean) / std for order 1.  Its chain is one to three roundings long, so the worst case u per rounding is all but
    attained and leaves a restatement no room; each of these roundings is budgeted at a whole ulp, ULP1 = 2 u, the rule of
    rowpass_ref for a single rounding (half an ulp moves a value, a whole one is budgeted), which also covers a device division
    that is faithful rather than correctly rounded.  e_p = ULP1 x / 255 for the division, and for order 1 that over std plus
    2 ULP1 |p| for the subtraction and the second division: the subtraction's cancellation is carried honestly.
      coordinate   the interpolant is continuous in the source coordinate, also where floor() flips and the taps shift by one, so
                   a coordinate off by dy, dx moves it by at most L LAMBDA (dy + dx) max|p| over the taps on both sides of a flip
                   (rows iy - 2 .. iy + 3, columns likewise): |df/dy| = |sum_i cy_i' sum_j cx_j p_ij| <= L LAMBDA max|p|;
      coefficient  sum_ij (e_i |cx_j| + |cy_i| e_j + e_i e_j) |p_ij| with e = COEF_ERR;
      sum          sum_ij |cy_i| |cx_j| (e_p + 10 u |p_ij|): a product and 4 additions per row, a product and 4 additions over rows
                   (n = 10 for the 4 x 4 sum; with the pixel's 1 or 3 roundings and order 0's final 2 the count from the code
                   is 13 for either order);
      order 0      the whole divided by std, plus 2 ULP1 |ref| for the final subtraction and division.
    S == R: no resampling, (x / 255 - mean) / std: ULP1 (x / 255) / std + 2 ULP1 |ref|."""
    raw, B, R = inp["raw"], inp["B"], inp["R"]
    m = torch.tensor([f32(v) for v in mean], dtype=F64).view(1, 3, 1, 1)
    sd = torch.tensor([f32(v) for v in std], dtype=F64).view(1, 3, 1, 1)
    V = raw.double() / 255.0
    if S == R:
        ref = (V - m) / sd
        return dict(out=ref, b_out=ULP1 * V / sd + 2 * ULP1 * ref.abs())
    idx, fr = _src_exact(R, S)
    C = _cubic(fr)                                             # [S, 4]
    if order == 1:
        Pm = (V - m) / sd
        e_p = ULP1 * V / sd + 2 * ULP1 * Pm.abs()
    else:
        Pm = V
        e_p = ULP1 * V
    tp = _taps(idx, R, -1, 2)                                  # [S, 4]
    gather = lambda a, t: a[:, :, t][:, :, :, :, t]            # noqa: E731  [B, 3, S, k, S, k]
    Pt, Et = gather(Pm, tp), gather(e_p, tp)
    cy, cx = C[None, None, :, :, None, None], C[None, None, None, None, :, :]
    ey, ex = COEF_ERR[None, None, None, :, None, None], COEF_ERR[None, None, None, None, None, :]
    r = (cy * cx * Pt).sum((3, 5))
    wabs = cy.abs() * cx.abs()
    b_sum = (wabs * (Et + 10 * U * Pt.abs())).sum((3, 5))
    b_coef = ((ey * cx.abs() + cy.abs() * ex + ey * ex) * Pt.abs()).sum((3, 5))
    pmax = gather(Pm.abs(), _taps(idx, R, -2, 3)).amax((3, 5))
    dc = coord_err(R, S)
    b_coord = CUBIC_L * CUBIC_LAMBDA * (dc[None, None, :, None] + dc[None, None, None, :]) * pmax
    b = b_coord + b_coef + b_sum
    if order == 1:
        return dict(out=r, b_out=b, b_coord=b_coord)
    ref = (r - m) / sd
    return dict(out=ref, b_out=b / sd + 2 * ULP1 * ref.abs(), b_coord=b_coord / sd)


PRE_MUTATIONS = ("a_half", "align_corners", "reflect", "clamp_one_deep", "swap_cy_cx", "channel0_stats", "div_256")


def pre_restatement(inp, S, order, mean, std, mutation=None):
    """preprocess_image_kernel in fp32 torch, operation by operation.  mutation: one of PRE_MUTATIONS."""
    assert mutation is None or mutation in PRE_MUTATIONS
    raw, B, R = inp["raw"], inp["B"], inp["R"]
    if mutation == "channel0_stats":
        mean, std = (mean[0], mean[1], mean[0]), (std[0], std[1], std[0])
    m = torch.tensor(mean, dtype=F32).view(1, 3, 1, 1)
    sd = torch.tensor(std, dtype=F32).view(1, 3, 1, 1)
    V = raw.float() / torch.tensor(256.0 if mutation == "div_256" else 255.0)
    Pm = (V - m) / sd if order == 1 else V
    if S == R:
        return dict(out=Pm if order == 1 else (Pm - m) / sd)
    dst = torch.arange(S, dtype=F32)
    if mutation == "align_corners":
        rc = dst * (torch.tensor(float(R - 1)) / torch.tensor(float(S - 1)))
    else:
        rc = (torch.tensor(float(R)) / torch.tensor(float(S))) * (dst + 0.5) - 0.5
    fl = torch.floor(rc)
    C = _cubic(rc - fl, -0.5 if mutation == "a_half" else CUBIC_A)            # fp32 [S, 4]
    assert C.dtype == F32
    tp = fl.long()[:, None] + torch.arange(-1, 3)[None, :]
    if mutation == "reflect":
        tp = torch.where(tp < 0, -tp, tp)
        tp = torch.where(tp > R - 1, 2 * (R - 1) - tp, tp)
    elif mutation == "clamp_one_deep":            # an index one outside is pulled in, one two outside lands one outside: the
        tp = torch.where(tp < 0, tp + 1, tp)      # neighbouring row's (column's) far end, here by wrapping
        tp = torch.where(tp > R - 1, tp - 1, tp) % R
    else:
        tp = tp.clamp(0, R - 1)
    Pt = Pm[:, :, tp][:, :, :, :, tp]                          # [B, 3, S(y), 4(i), S(x), 4(j)]
    by_y = lambda k: C[:, k][None, None, :, None]              # noqa: E731  weight k of the output's row / of its column
    by_x = lambda k: C[:, k][None, None, None, :]              # noqa: E731
    if mutation == "swap_cy_cx":                  # the row sum weighted by cy[j], the rows by cx[i]
        by_y, by_x = by_x, by_y
    out = torch.zeros(B, 3, S, S)
    for i in range(4):
        row = torch.zeros(B, 3, S, S)
        for j in range(4):
            row = row + Pt[:, :, :, i, :, j] * by_x(j)
        out = out + row * by_y(i)
    return dict(out=out if order == 1 else (out - m) / sd)


def pre_torch(inp, S, order, mean, std):
    """torch's own fp32 path, the contract in the kernel's comment: F.interpolate(mode='bicubic', align_corners=False) around the
    normalisation in the order given.  A second witness of the budget: it must stay inside it too."""
    import torch.nn.functional as Fn
    m = torch.tensor(mean, dtype=F32).view(1, 3, 1, 1)
    sd = torch.tensor(std, dtype=F32).view(1, 3, 1, 1)
    x = inp["raw"].float() / 255.0
    rs = (lambda a: a) if S == inp["R"] else (lambda a: Fn.interpolate(a, size=(S, S), mode="bicubic", align_corners=False))
    return dict(out=rs((x - m) / sd) if order == 1 else (rs(x) - m) / sd)
