"""CPU proofs for tests/mxfp8_ref.py: the reference quantiser against torch's own e4m3 casts and on its edge cases, the budgets of
the MX-fp8 products (fp32 restatements stay at or below 0.6 of them, every realistic bug leaves them by more than 20 times, on
the shapes of tests/test_mxfp8_gemm_gpu.py), the host-side plan against the shape rules, the oracle hook, and the command line."""
import pytest
import torch

from oracle import detfill
from oracle import sit as osit
from tests import gemm_ref as G
from tests import mxfp8_ref as R
from tests.test_oracle_golden import TINY_CASES, inputs

KINDS = G.KINDS16
_INP = {}


def _inputs(sh, kind):
    if (sh, kind) not in _INP:
        while len(_INP) >= 2:
            _INP.pop(next(iter(_INP)))
        _INP[(sh, kind)] = R.inputs(sh, kind)
    return _INP[(sh, kind)]


@pytest.mark.parametrize("kind", KINDS)
def test_quantiser_against_torch_e4m3_casts(kind):
    g = torch.Generator().manual_seed(5)
    n = 1563                                           # x 128 = 200 064 elements
    x = (torch.randn(n, 128, generator=g) * torch.exp(1.5 * torch.randn(n, 1, generator=g))).to(G.DTYPE[kind])
    q, s = R.quantize(x)
    X = s.to(torch.int32) - 127
    v = torch.ldexp(x.double().reshape(n, 4, 32), -X.unsqueeze(-1)).reshape(n, 128)
    assert float(v.abs().max()) < 512 and float(v.abs().reshape(n, 4, 32).amax(-1).min()) >= 256      # the scaled amax lies in [256, 512)
    want = v.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
    bad = int((want != q).sum())
    print(f"[quantiser {kind}] {bad} mismatches of {q.numel()} against torch.float8_e4m3fn; saturated {float((v.abs() > 448).double().mean()):.4f}")
    assert bad == 0


@pytest.mark.parametrize("kind", KINDS)
def test_quantiser_edge_cases(kind):
    x = R.edge_rows(128, kind)
    q, s = R.quantize(x)
    d = R.decode(q, s)
    blk = lambda r, i: slice(32 * i, 32 * i + 32)  # noqa: E731
    # a zero block: scale byte 127, signed zeros kept
    assert int(s[0, 0]) == 127 and q[0, blk(0, 0)].tolist() == [0x00, 0x80] * 16
    # subnormals and ties at multiples of 2^-10 (scaled by 2^0: amax 256): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 7.5 -> 8, 8.5 -> 8 (x 2^-9)
    assert int(s[0, 1]) == 127 and q[0, 32:41].tolist() == [0x78, 0, 2, 2, 1, 3, 8, 8, 8]
    # amax an exact power of two: 4 = 2^2 -> X = -6, code of 256
    assert int(s[0, 2]) == 127 - 6 and int(q[0, 64 + 3]) == 0xF8 and float(d[0, 64 + 3]) == -4.0
    # the saturating band: everything from 448 up is 448 (0x7E); never the NaN code
    sat = x[0, blk(0, 3)].double().abs() >= 448
    assert int(s[0, 3]) == 127 and int(sat.sum()) >= 4 and bool((q[0, blk(0, 3)][sat] & 0x7F == 0x7E).all())
    assert not bool(((q[:2] & 0x7F) == 0x7F).any())
    # the type's subnormals: bf16's clamp X at -127 (byte 0), fp16's do not
    assert int(s[1, 0]) == (0 if kind == "bf16" else 127 - 24 + 4 - 8) and torch.equal(d[1, 32:64], x[1, 32:64].double())
    # inf / NaN blocks: byte 0xFF, NaN codes, NaN on decode; the row's clean block untouched
    assert s[2].tolist()[:3] == [255, 255, 255] and int(s[2, 3]) != 255
    assert bool((q[2, :96] == 0x7F).all()) and bool(torch.isnan(d[2, :96]).all()) and bool(torch.isfinite(d[2, 96:]).all())
    # idempotence on everything finite
    fin = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    q2, s2 = R.quantize(d[fin])
    assert torch.equal(q2, q[fin]) and torch.equal(s2, s[fin])
    # |decode - x| <= 2^-4 |x| for unsaturated normals, <= 2^-3 |x| for saturated ones
    xs = x[fin].double()
    X = (s[fin].to(torch.int32) - 127).unsqueeze(-1)
    v = torch.ldexp(xs.reshape(len(fin), 4, 32), -X).reshape(xs.shape).abs()
    err = (d[fin] - xs).abs()
    normal, satd = (v >= 2.0 ** -6) & (v <= 448), v > 448
    assert bool((err[normal] <= 2.0 ** -4 * xs.abs()[normal]).all()) and bool((err[satd] <= 2.0 ** -3 * xs.abs()[satd]).all())
    assert bool((err[v < 2.0 ** -6] <= torch.ldexp(torch.ones_like(v), X.expand(-1, -1, 32).reshape(v.shape) - 10)[v < 2.0 ** -6]).all())


CASES = [(sh, kind) for sh in R.SHAPES for kind in KINDS]
IDS = [f"{s.M}x{s.N}x{s.K}-{k}" for s, k in CASES]


@pytest.mark.parametrize("sh,kind", CASES, ids=IDS)
def test_restatements_stay_inside_the_budget(sh, kind):
    inp = _inputs(sh, kind)
    for epi in R.EPIS:
        for var in R.variants(epi):
            for mode in ("sequential", "truncating"):
                got = {k: v.double() for k, v in R.restatement(inp, epi, var, mode).items()}
                rat = G.ratios(got, R.reference(inp, epi, var, got))
                for k, (r, i) in rat.items():
                    assert r <= 0.6, (G.EPI_NAME[epi], var, mode, k, r, i)


@pytest.mark.parametrize("sh,kind", CASES, ids=IDS)
def test_every_realistic_bug_leaves_the_budget(sh, kind):
    inp = _inputs(sh, kind)
    var = dict(_bias=True)
    for mutation in R.MUTATIONS:
        got = {k: v.double() for k, v in R.restatement(inp, G.BF16, var, mutation=mutation).items()}
        r, i = G.ratios(got, R.reference(inp, G.BF16, var, got))["C"]
        print(f"[{mutation} {kind} {tuple(sh[:3])}] worst error / budget {r:.1f}")
        assert r > 20, (mutation, r, i)


def test_plan_follows_the_shape_rules_both_ways():
    from reed_amd import ops
    for kind in KINDS:
        for epi in range(18):
            for M in (1, 9, 300):
                for N in (64, 128, 144, 384, 1152):
                    for K in (64, 96, 128, 144, 640, 4608):
                        want = epi in R.EPIS and N % 128 == 0 and K % 128 == 0
                        assert ops.gemm_mxfp8_plan(epi, M, N, K, precision=kind) == want, (kind, epi, M, N, K)
        assert not ops.gemm_mxfp8_plan(G.BF16, 0, 128, 128, precision=kind)
    assert not ops.gemm_mxfp8_plan(G.BF16, 9, 128, 128, precision="fp32")     # the fp32-operand build: an argument-error stub


def test_emulation_hook_fires_on_the_block_linears_only():
    cfg = TINY_CASES["hd64"]["cfg"]
    xi, _, ti, yi, _, _ = inputs(4, 4, cfg["input_size"], 11, [], 0, 10)
    P = {k: v.double() for k, v in detfill.fill_state_dict(osit.init_params(cfg), base_seed=11).items()}
    real_F = osit.F
    with torch.no_grad():
        exact = osit.OracleModel(P, cfg)(xi.double(), ti.double(), yi)[0]
        with R.mx_emulation(P, cfg["depth"]) as count:
            mx = osit.OracleModel(P, cfg)(xi.double(), ti.double(), yi)[0]
        again = osit.OracleModel(P, cfg)(xi.double(), ti.double(), yi)[0]
    assert osit.F is real_F and torch.equal(again, exact)
    assert count[0] == 4 * cfg["depth"]
    d = R.rel_l2(mx, exact)
    print(f"[hd64] the MX emulation moves the fp64 oracle by rel L2 {d:.3e}")
    assert 3e-3 <= d <= 3e-2


def test_generate_accepts_fp8():
    from reed_amd import generate
    args = generate.build_parser().parse_args(["--sample-precision", "fp8"])
    assert generate.sample_precision(args) == "fp8"
    assert "@@" not in generate.FP8_HELP
