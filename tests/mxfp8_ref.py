"""The MX-fp8 format in torch (quantiser, decode), fp64 products of decoded operands with the budgets of tests/gemm_ref.py, and a
hook that makes oracle.sit run its four block linears on quantise-decoded operands.  A plain module, not a test file:
tests/test_mxfp8_budgets_cpu.py proves the quantiser and the budgets on the CPU, tests/test_mxfp8_gemm_gpu.py and
tests/test_mxfp8_model_gpu.py hold csrc/gemm_mxfp8.hip and the fp8 sampling path to them.

FORMAT (include/reed_hip.h): e4m3fn elements (bias 7, max 448, NaN 0x7F / 0xFF), blocks of 32 along K, one E8M0 byte per block.
Finite block, amax > 0: X = clamp(floor(log2 amax) - 8, -127, 127), byte X + 127, code = RNE_e4m3(x 2^-X) saturated at 448 (the
scaled amax lies in [256, 512): (448, 512) saturates).  amax = 0: byte 127, signed zeros.  inf / NaN in the block: byte 0xFF,
every code 0x7F; decode gives NaN.

BUDGETS: the kernel multiplies the SAME decoded operands the reference multiplies (the quantiser is tested bit for bit on its
own), so the budget of a product is gemm_ref's with A, W replaced by their decoded values: e_acc = (K + 1) u' sum|terms|,
u' = 2 u (that module's "safe under truncation, UNMEASURED" convention: the products of two e4m3 codes have 8 significant bits
and are exact in fp32, the block scales are powers of two), plus its 16-bit-output and chained-epilogue terms, imported.
"""
import contextlib

import torch

from tests import gemm_ref
from tests.gemm_ref import BF16, GATE_RES, GELU, S  # noqa: F401  (re-exported for the tests)

BLOCK = 32
EPIS = (BF16, GELU, GATE_RES)
# (M, N, K): the shapes of the GPU test (and of the CPU proofs)
SHAPES = (S(9, 256, 128, "M < 16; one K-tile"), S(300, 384, 256, "ragged rows; N % 256 == 128"),
          S(520, 640, 384, "an odd K-tile count"), S(130, 1152, 640, "4.5 column tiles at 256"),
          S(257, 128, 4608, "fc2's K: 36 K-tiles"))


def _e4m3_table():
    c = torch.arange(256)
    e, m = (c >> 3) & 15, (c & 7).double()
    v = torch.where(e == 0, m * 2.0 ** -9, torch.ldexp(1 + m / 8, e - 7))
    v = torch.where((c & 0x7F) == 0x7F, torch.full_like(v, float("nan")), v)
    return torch.where(c >= 128, -v, v)


E4M3 = _e4m3_table()   # code -> value (fp64)


def e4m3_codes(v):
    """fp64 values, finite -> uint8 codes: round to nearest-even onto the e4m3 grid, signs and subnormals kept, saturated to 448."""
    a = v.abs().clamp(max=448.0)
    _, e = torch.frexp(a)
    E = (e - 1).clamp(min=-6)                          # exponent of the binade (subnormals share -6's spacing 2^-9)
    q = torch.round(torch.ldexp(a, 3 - E))             # multiples of the spacing; torch.round is half-to-even
    up = q == 16
    E, q = torch.where(up, E + 1, E), torch.where(up, torch.full_like(q, 8), q)
    code = torch.where(q < 8, q, ((E + 7) * 8 + (q - 8)).double()).to(torch.int64)
    return (code | (torch.signbit(v).to(torch.int64) << 7)).to(torch.uint8)


def quantize(x):
    """x [..., K] (K % 32 == 0; any float type, read exactly) -> (codes uint8 [..., K], scale bytes uint8 [..., K / 32])."""
    K = x.shape[-1]
    assert K % BLOCK == 0
    xb = x.double().reshape(*x.shape[:-1], K // BLOCK, BLOCK)
    bad = ~torch.isfinite(xb).all(-1, keepdim=True)
    amax = torch.where(bad, torch.ones_like(xb[..., :1]), xb.abs().amax(-1, keepdim=True))
    zero = amax == 0
    _, e = torch.frexp(torch.where(zero, torch.ones_like(amax), amax))
    X = torch.where(zero, torch.zeros_like(e), (e - 1 - 8).clamp(-127, 127))
    codes = e4m3_codes(torch.ldexp(torch.where(bad, torch.zeros_like(xb), xb), -X))
    codes = torch.where(bad, torch.full_like(codes, 0x7F), codes)
    scales = torch.where(bad, torch.full_like(X, 255), X + 127).to(torch.uint8)
    return codes.reshape(x.shape), scales.squeeze(-1)


def decode(codes, scales):
    """fp64 values of (codes [..., K], scales [..., K / 32]); a 0xFF scale byte decodes to NaN."""
    K = codes.shape[-1]
    v = E4M3[codes.long()].reshape(*codes.shape[:-1], K // BLOCK, BLOCK)
    s = torch.ldexp(torch.ones(scales.shape, dtype=torch.float64), scales.to(torch.int32) - 127).unsqueeze(-1)
    s = torch.where(scales.unsqueeze(-1) == 255, torch.full_like(s, float("nan")), s)
    return (v * s).reshape(codes.shape)


def fake_quant(x):
    """decode(quantize(x)) in x's type (every decoded value has 4 significant bits: exact in bf16, and in fp16 inside its range)."""
    return decode(*quantize(x)).to(x.dtype)


# ----------------------------------------------------------------------------------------------------------------- GEMM
def edge_rows(K, kind):
    """Rows of the quantiser's edge cases (K >= 128), in the operand type: one case per block of 32."""
    dt = gemm_ref.DTYPE[kind]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(12, K, generator=g, dtype=torch.float64)
    b = lambda r, i: x[r, 32 * i:32 * i + 32]  # noqa: E731
    b(0, 0)[:] = 0                                              # a zero block ...
    b(0, 0)[1::2] = -0.0                                        # ... with both zeros
    b(0, 1)[:] = torch.tensor([256.0] + [2.0 ** -9 * k for k in (0.5, 1.5, 2.5, 1, 3, 7.5, 8, 8.5)] + [0.0] * 23)   # subnormals, 2^-9 ties
    b(0, 2)[:] = 0
    b(0, 2)[3] = -4.0                                           # amax an exact power of two
    b(0, 3)[:] = torch.tensor([447.9, 448.0, 464.0, 479.9, -464.0, 256.0] + [1.0] * 26)   # the saturating band (scaled by 2^0)
    tiny = 2.0 ** -133 if kind == "bf16" else 2.0 ** -24        # the type's smallest subnormal (bf16: X clamps at -127)
    b(1, 0)[:] = tiny * torch.arange(32)
    b(1, 1)[:] = 0
    b(1, 1)[7] = tiny
    b(2, 0)[5] = float("inf")
    b(2, 1)[6] = float("-inf")
    b(2, 2)[0] = float("nan")
    big = 3.0e38 if kind == "bf16" else 65504.0
    b(3, 0)[:] = torch.tensor([big, -big, big / 3, 1.0] + [0.5] * 28)       # the type's largest finite values
    b(3, 1)[:] = 2.0 ** torch.arange(-16, 16, dtype=torch.float64)          # 32 binades in one block
    x[4] = x[4] * 1e-3
    x[5] = x[5] * 1e3
    return x.to(dt)


def inputs(sh, kind):
    """gemm_ref.inputs (per-row scales exp(0.5 N), a zero last row, bias / gate / residual) with the operands quantised: Aq / As /
    Wq / Ws are what the kernel reads, A / W (what every reference of gemm_ref multiplies) their decoded values in fp64."""
    inp = gemm_ref.inputs(sh, kind)
    inp["A16"], inp["W16"] = inp["A"], inp["W"]
    inp["Aq"], inp["As"] = quantize(inp["A16"])
    inp["Wq"], inp["Ws"] = quantize(inp["W16"])
    inp["A"], inp["W"] = decode(inp["Aq"], inp["As"]), decode(inp["Wq"], inp["Ws"])
    return inp


def variants(epi):
    """The calls of one epilogue: gemm_ref's, for a forward NT row of its table."""
    return [dict(v, _bias=True) for v in gemm_ref.variants(gemm_ref.ROWS[0], epi, None)]


def reference(inp, epi, var, got):
    """{output: (fp64 reference, budget)}: gemm_ref.reference on the decoded operands (K + 1 terms, u' = 2 u)."""
    return gemm_ref.reference(inp, epi, var, got)


MUTATIONS = ("neighbour_scale", "k_order", "fnuz_bias", "no_saturation", "drop_last_ktile", "bias_before_scales")


def accumulate32(inp, mode="sequential", mutation=None):
    """The kernel's K loop in fp32: per 128-code K-tile and block of 32 the partial sums of code products (exact in fp32), scaled by
    2^(Xa + Xw) and added in k order; mode "truncating" chops every partial sum toward zero to 24 bits.  Returns acc [M, N]."""
    sh = inp["sh"]
    Aq, Wq, As, Ws = inp["Aq"], inp["Wq"], inp["As"], inp["Ws"]
    if mutation == "no_saturation":                   # the kernel's rounding without its clamp: a scaled value in (464, 496) rounds to
        def unsat(x16, q, s):                         # 480 = the NaN code 0x7F, one from 496 on to 512 = exponent field 16: a carry into
            v = torch.ldexp(x16.double().reshape(*s.shape, BLOCK), (127 - s.to(torch.int32)).unsqueeze(-1)).reshape(q.shape)   # the sign bit, code +-0
            out = torch.where(v.abs() >= 496, torch.zeros_like(v), E4M3[q.long()])
            return torch.where((v.abs() > 464) & (v.abs() < 496), torch.full_like(v, float("nan")), out)
        a, w = unsat(inp["A16"], Aq, As), unsat(inp["W16"], Wq, Ws)
    else:
        tab = E4M3 * 0.5 if mutation == "fnuz_bias" else E4M3
        a, w = tab[Aq.long()], tab[Wq.long()]
    if mutation == "k_order":                         # W's 16-byte halves of a lane's 32 codes swapped against A's
        w = w.reshape(sh.N, -1, 2, 16).flip(2).reshape(sh.N, -1)
    sa = torch.ldexp(torch.ones(As.shape, dtype=torch.float64), As.to(torch.int32) - 127)
    sw = torch.ldexp(torch.ones(Ws.shape, dtype=torch.float64), Ws.to(torch.int32) - 127)
    if mutation == "neighbour_scale":
        sa = torch.roll(sa, 1, 1)
    nb = sh.K // BLOCK - (4 if mutation == "drop_last_ktile" else 0)
    acc = torch.zeros(sh.M, sh.N, dtype=torch.float32)
    if mutation == "bias_before_scales":              # the bias joins the first block's code sum and is scaled with it
        acc = acc + inp["bias"].float() * (sa[:, :1] * sw[:, :1].T).float()
    for j in range(nb):
        k = slice(BLOCK * j, BLOCK * j + BLOCK)
        p = (a[:, k].float() @ w[:, k].float().T) * (sa[:, j:j + 1] * sw[:, j:j + 1].T).float()
        acc = acc + p
        if mode == "truncating":
            acc = _chop(acc)
    return acc


def _chop(x):
    """fp32 -> the fp32 value toward zero with the last mantissa bit cleared (a sum that was truncated, not rounded)."""
    return (x.view(torch.int32) & ~1).view(torch.float32)


def restatement(inp, epi, var, mode="sequential", mutation=None):
    """gemm_ref.restatement's epilogues behind accumulate32: the kernel's order of operations in fp32 torch."""
    acc = accumulate32(inp, mode, mutation)
    m = "bias_dropped" if mutation == "bias_before_scales" else None
    out = gemm_ref.restatement(inp, gemm_ref.ROWS[0], epi, var, mutation=m, acc=([acc], [None]))
    return out


# --------------------------------------------------------------------------------------------------------- oracle hook
class _FProxy:
    def __init__(self, real, weights, count):
        self._real, self._weights, self._count = real, weights, count

    def __getattr__(self, name):
        return getattr(self._real, name)

    def linear(self, x, w, b=None):
        if id(w) not in self._weights:
            return self._real.linear(x, w, b)
        self._count[0] += 1
        dt = torch.get_autocast_dtype("cpu") if torch.is_autocast_enabled("cpu") else x.dtype
        return self._real.linear(fake_quant(x.to(dt)), fake_quant(w.to(dt)), b)


@contextlib.contextmanager
def mx_emulation(P, depth):
    """Inside the block, oracle.sit evaluates the four block linears (qkv, proj, fc1, fc2 of every block of P) on quantise-decoded
    operands (under autocast: of the operands cast to the autocast type); everything else is untouched.  Yields a one-element
    list that counts the substituted calls."""
    import oracle.sit as osit
    names = [f"blocks.{i}.{w}.weight" for i in range(depth) for w in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
    count = [0]
    real = osit.F
    osit.F = _FProxy(real, {id(P[n]) for n in names}, count)
    try:
        yield count
    finally:
        osit.F = real


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
