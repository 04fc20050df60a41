"""fp64 references, error budgets and an fp32 restatement for the row-pass kernels (csrc/qknorm.hip, the reductions of
csrc/norm.hip).  A plain module, not a test file: tests/test_rowpass_budgets_cpu.py proves the budgets on the CPU (the
restatement stays well inside them, realistic bugs leave them), tests/test_qknorm_gpu.py and tests/test_reductions_gpu.py
hold the kernels to them.

The budgets are BOUNDS derived from the arithmetic, not measurements of what the kernels deliver.  u = 2**-24 is the unit
roundoff of fp32; a sequential or tree-shaped fp32 sum of n terms is within n * u * sum|terms| of the exact sum (Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2: gamma_{n-1} <= n u for n u << 1), and one rounding to the output type moves a value by at
most half of ulp_out(ref) (a whole one is budgeted, so that a reference that sits just across a binade edge is covered).
"""
import torch

U = 2.0 ** -24
QK_EPS = 1e-5
KINDS = ("bf16", "fp16", "fp32")
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_FMT = {"bf16": (7, -126), "fp16": (10, -14), "fp32": (23, -126)}   # explicit mantissa bits, exponent of the minimum normal
MUTATIONS = ("eps", "var_unbiased", "swap_w", "a2_64", "no_w_bwd")
QK_SHAPES = ((5, 2, 64), (128, 2, 64), (100, 3, 72), (48, 16, 72))    # (M, H, hd): see tests/test_qknorm_gpu.py


def ulp_out(ref, kind):
    """Spacing of the `kind` numbers at |ref| (fp64 tensor in, fp64 tensor out): 2**(floor(log2|ref|) - mantissa bits), the
    exponent clamped at the type's minimum normal (below it the spacing is that of the subnormals; ref = 0 lands there too)."""
    p, emin = _FMT[kind]
    ref = torch.as_tensor(ref, dtype=torch.float64)
    _, e = torch.frexp(ref.abs())                      # |ref| = m * 2**e, m in [0.5, 1): floor(log2|ref|) = e - 1
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref), e - p)


def worst(err, budget):
    """(largest err / budget, flat index of it).  A NaN or an infinite error counts as infinitely far outside."""
    err, budget = err.double().flatten(), budget.double().flatten().expand(err.numel())
    ratio = err / budget
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where((err == 0) & (budget == 0), torch.zeros_like(ratio), ratio)
    i = int(torch.argmax(ratio))
    return float(ratio[i]), i


# ------------------------------------------------------------------------------------------------------------ qk-norm
def qk_inputs(M, H, hd, kind, seed=0):
    """Seeded CPU inputs of the qk-norm tests: qkv [M, 3, H, hd] with a per-segment scale exp(N(0,1)) and offset 2 N(0,1), one
    constant segment (variance 0: eps decides, the output is b), one segment of tiny spread on a mean of 3; distinct affine
    vectors; an upstream gradient of about 0.02 N.  qkv and dn are in the build's operand type."""
    g = torch.Generator().manual_seed(1234 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = rn(M, 3, H, hd) * torch.exp(rn(M, 3, H, 1)) + 2.0 * rn(M, 3, H, 1)
    x[0, 1, H - 1] = 1.625                                      # constant segment (a k segment)
    x[M - 1, 0, 0] = 3.0 + 0.01 * rn(hd)                        # tiny spread on a large mean (a q segment, in the last block)
    qw, kw = (1 + 0.3 * rn(hd)).float(), (1 + 0.3 * rn(hd)).float()
    qb, kb = (0.2 * rn(hd)).float(), (0.2 * rn(hd)).float()
    dn = 0.02 * rn(M, 3, H, hd)
    return dict(qkv=x.to(DTYPE[kind]), dn=dn.to(DTYPE[kind]), qw=qw, qb=qb, kw=kw, kb=kb, M=M, H=H, hd=hd, kind=kind)


def _block_sum(c, M, H):
    """c [M, 3, H, ...] per-segment contributions -> [nblocks, ...]: sums over each block of 256 consecutive segments."""
    nseg = M * 3 * H
    nb = (nseg + 255) // 256
    c = c.reshape(nseg, *c.shape[3:])
    pad = torch.zeros(nb * 256 - nseg, *c.shape[1:], dtype=c.dtype)
    return torch.cat([c, pad]).reshape(nb, 256, *c.shape[1:]).sum(1)


def _part_layout(cq_w, cq_b, ck_w, ck_b, M, H):
    """Per-(token, head) contributions [M, H, hd] of q and k -> per-block partials [nblocks, 2 (q,k), 2 (dw,db), hd]."""
    hd = cq_w.shape[-1]
    c = torch.zeros(M, 3, H, 2, 2, hd, dtype=cq_w.dtype)
    c[:, 0, :, 0, 0], c[:, 0, :, 0, 1] = cq_w, cq_b
    c[:, 1, :, 1, 0], c[:, 1, :, 1, 1] = ck_w, ck_b
    return _block_sum(c, M, H)


def qk_reference(inp):
    """fp64 qk-norm from the operand-type inputs and the fp32 affine vectors.  Returns the forward output, the statistics in the
    documented layout, the backward, the parameter-gradient partials per block and in total, and the budget of each."""
    M, H, hd, kind = inp["M"], inp["H"], inp["hd"], inp["kind"]
    X = inp["qkv"].double()[:, :2]                                      # [M, 2, H, hd]
    G = inp["dn"].double()[:, :2]
    W = torch.stack([inp["qw"], inp["kw"]]).double()[None, :, None, :]
    B = torch.stack([inp["qb"], inp["kb"]]).double()[None, :, None, :]
    MEAN = X.mean(-1, keepdim=True)
    VAR = ((X - MEAN) ** 2).mean(-1, keepdim=True)
    R = 1.0 / torch.sqrt(VAR + QK_EPS)
    XH = (X - MEAN) * R
    OUT = XH * W + B
    GY = G * W
    A1 = GY.mean(-1, keepdim=True)
    A2 = (GY * XH).mean(-1, keepdim=True)
    DPRE = R * (GY - A1 - XH * A2)
    mabs = X.abs().mean(-1, keepdim=True)
    # absolute error of xhat: hd roundings in each of the mean, the variance and the product, and the conditioning of a small
    # spread on a large mean (the mean's error hd u mean|X|, scaled by rstd)
    dxh = 2 * hd * U * (XH.abs() + R * mabs)
    b_out = ulp_out(OUT, kind) + dxh * W.abs() + 4 * U * ((XH * W).abs() + B.abs())
    S = GY.abs() + GY.abs().mean(-1, keepdim=True) + XH.abs() * (GY * XH).abs().mean(-1, keepdim=True)
    b_dpre = ulp_out(DPRE, kind) + 2 * hd * U * R * S + R * (A2.abs() * dxh + XH.abs() * (GY.abs() * dxh).mean(-1, keepdim=True))
    stats = torch.stack([MEAN[..., 0], R[..., 0]], -1)                  # [M, 2, H, 2]
    b_stats = torch.stack([2 * hd * U * mabs[..., 0], 2 * hd * U * R[..., 0]], -1)
    # parameter gradients: dw = sum G xhat, db = sum G over the q (k) segments of a block / of everything
    lay = lambda f: _part_layout(f[:, 0], torch.zeros_like(f[:, 0]), f[:, 1], torch.zeros_like(f[:, 0]), M, H)  # noqa: E731
    part = _part_layout((G * XH)[:, 0], G[:, 0], (G * XH)[:, 1], G[:, 1], M, H)
    ones = torch.ones(M, H, hd, dtype=torch.float64)
    cnt = _part_layout(ones, ones, ones, ones, M, H)                    # contributing segments per slot
    s_abs = _part_layout((G * XH).abs()[:, 0], G.abs()[:, 0], (G * XH).abs()[:, 1], G.abs()[:, 1], M, H)
    s_dxh = lay(G.abs() * dxh)                                          # only the dw slots carry xhat's error
    b_part = 2 * cnt * U * s_abs + s_dxh
    total = part.sum(0)
    b_total = 2 * cnt.sum(0) * U * s_abs.sum(0) + s_dxh.sum(0)
    return dict(out=OUT, b_out=b_out, stats=stats, b_stats=b_stats, dpre=DPRE, b_dpre=b_dpre, part=part, b_part=b_part,
                total=total, b_total=b_total, nblocks=part.shape[0])


def _seqsum(x):
    """fp32 sum over the last axis in index order, as one thread of the kernel does it."""
    s = torch.zeros_like(x[..., 0])
    for e in range(x.shape[-1]):
        s = s + x[..., e]
    return s


def _tree256(c):
    """[nb, 256, ...] fp32 -> [nb, ...]: a butterfly over the 64 lanes of each wave, then (w0 + w1) + (w2 + w3)."""
    c = c.reshape(c.shape[0], 4, 64, *c.shape[2:])
    n = 64
    while n > 1:
        n //= 2
        c = c[:, :, :n] + c[:, :, n:2 * n]
    c = c[:, :, 0]
    return (c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])


def qk_restatement(inp, mutation=None):
    """The kernels' arithmetic restated in fp32 torch: two-pass variance with in-order sums, rsqrt, the round to the output
    type, a1 / a2 as csrc/qknorm.hip forms them, the per-block butterfly.  mutation: one of MUTATIONS = a realistic bug."""
    assert mutation is None or mutation in MUTATIONS
    M, H, hd, kind = inp["M"], inp["H"], inp["hd"], inp["kind"]
    dt = DTYPE[kind]
    x = inp["qkv"].float()[:, :2]
    g = inp["dn"].float()[:, :2]
    wq, wk, bq, bk = inp["qw"], inp["kw"], inp["qb"], inp["kb"]
    if mutation == "swap_w":
        wq, wk, bq, bk = wk, wq, bk, bq
    w = torch.stack([wq, wk])[None, :, None, :]
    b = torch.stack([bq, bk])[None, :, None, :]
    hdf = torch.tensor(float(hd))
    mu = (_seqsum(x) / hdf)[..., None]
    d = x - mu
    q = _seqsum(d * d)
    var = q / (hdf - 1 if mutation == "var_unbiased" else hdf)
    r = torch.rsqrt(var if mutation == "eps" else var + torch.tensor(QK_EPS))[..., None]
    out = ((x - mu) * r * w + b).to(dt)
    xh = (x - mu) * r
    gy = g if mutation == "no_w_bwd" else g * w
    a1 = (_seqsum(gy) / hdf)[..., None]
    a2 = (_seqsum((gy * xh)[..., :64] if mutation == "a2_64" else gy * xh) / hdf)[..., None]
    dpre = (r * (gy - a1 - xh * a2)).to(dt)
    nseg = M * 3 * H
    nb = (nseg + 255) // 256
    c = torch.zeros(M, 3, H, 2, 2, hd)
    c[:, 0, :, 0, 0], c[:, 0, :, 0, 1] = (g * xh)[:, 0], g[:, 0]
    c[:, 1, :, 1, 0], c[:, 1, :, 1, 1] = (g * xh)[:, 1], g[:, 1]
    c = torch.cat([c.reshape(nseg, 2, 2, hd), torch.zeros(nb * 256 - nseg, 2, 2, hd)]).reshape(nb, 256, 2, 2, hd)
    part = _tree256(c)
    total = torch.zeros(2, 2, hd)
    for i in range(nb):
        total = total + part[i]
    return dict(out=out, stats=torch.stack([mu[..., 0], r[..., 0]], -1), dpre=dpre, part=part, total=total)


QK_OUTPUTS = ("out", "stats", "dpre", "part", "total")


def qk_ratios(got, ref):
    """{output: (worst error / budget, flat index)} of a result dict (tensors of any float type) against qk_reference's."""
    res = {}
    for k in QK_OUTPUTS:
        if k in got:
            res[k] = worst((got[k].double().cpu() - ref[k]).abs(), ref["b_" + k])
    return res


# --------------------------------------------------------------------------------------------------------- reductions
def sum_budget(terms, dim, kind=None):
    """(fp64 sum over `dim`, its budget): n u sum|terms| for the n values summed into one output, plus ulp_out(ref) where the
    output is rounded to a 16-bit type."""
    t = terms.double()
    ref = t.sum(dim)
    b = t.shape[dim] * U * t.abs().sum(dim)
    if kind in ("bf16", "fp16"):
        b = b + ulp_out(ref, kind)
    return ref, b


def seq_sum_f32(terms, dim=0):
    """One sequential fp32 chain over `dim`, starting from 0.0f: the order of csrc/norm.hip's reduce_slabs and token_mean."""
    t = terms.float().movedim(dim, 0)
    s = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


# ------------------------------------------------------------------------------------------- guard bands (GPU tests)
BAND = 256


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


class Guarded:
    """n elements of `dtype` pre-filled with `fill` (NaN: an unwritten slot shows), a canary band of BAND elements behind."""

    def __init__(self, n, dtype, dev, fill=float("nan")):
        self.n = n
        self.full = torch.full((n + BAND,), fill, dtype=dtype, device=dev)
        self.full[n:] = (torch.arange(BAND, device=dev) * 3 + 1000).to(dtype)
        self.band = self.full[n:].clone()
        self.t = self.full[:n]

    def intact(self):
        return torch.equal(bits(self.full[self.n:]), bits(self.band))
