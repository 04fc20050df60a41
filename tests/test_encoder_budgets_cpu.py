"""The error budgets of tests/encoder_ref.py, proven on the CPU before tests/test_encoder_rows_gpu.py relies on them (the two
conditions and the numbers of tests/test_rowpass_budgets_cpu.py and tests/test_adaln_budgets_cpu.py).

(a) the fp32 restatement of each kernel's own arithmetic stays at or below 0.6 of every budget, in all three builds' types, at
    every shape, form and flag the GPU test uses: the kernel keeps the rest for the hardware's rsqrt, division and FMA
    contraction.  Token assembly and im2col have a budget of 0: the restatement IS the reference, and what is checked is that the
    reference agrees with an independent formulation (torch's own cat / unfold);
(b) every realistic bug of exactly these kernels leaves the budget (worst error / budget above 1.0) in at least one of the
    shapes listed for it; where a bug cannot show in some shape or build (a missing rounding in the fp32 build, a neighbouring
    row when there is one row) the test says so and asserts that it is then no difference at all or still inside;
(c) torch's own fp32 F.interpolate + normalise stays inside the preprocess budget on the same inputs: a second witness that the
    budget is not mis-derived.
"""
import pytest
import torch

from tests import encoder_ref as E
from tests.encoder_ref import KINDS, worst

_CACHE = {}


def _ln(kind, M, D, entry, out_f32):
    """(inputs, fp64 reference) of one LayerNorm case: computed once, shared, never modified (ldo does not enter the values)."""
    key = (kind, M, D, entry, out_f32)
    if key not in _CACHE:
        inp = E.ln_inputs(M, D, kind, entry)
        _CACHE[key] = (inp, E.ln_reference(inp, out_f32))
    return _CACHE[key]


def _pre(case):
    B, R, S, order, mean, std = case
    if case not in _CACHE:
        inp = E.pre_inputs(B, R)
        _CACHE[case] = (inp, E.pre_reference(inp, S, order, mean, std))
    return _CACHE[case]


def _ratio(got, ref):
    return worst((got["out"].double() - ref["out"]).abs(), ref["b_out"])


LN_VALUE_CASES = sorted({(M, D, e, of) for M, D, e, of, _ in E.ln_cases()})


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("kind", KINDS)
def test_ln_restatement_stays_inside(kind):
    top = {}
    for M, D, entry, out_f32 in LN_VALUE_CASES:
        inp, ref = _ln(kind, M, D, entry, out_f32)
        got = E.ln_restatement(inp, out_f32)
        r, i = _ratio(got, ref)
        assert r <= 0.6, (kind, M, D, entry, out_f32, r, i)
        form = f"ln_affine_{entry} -> {'fp32' if out_f32 else 'operand type'}"
        top[form] = max(top.get(form, 0.0), r)
        if M > 1:     # the constant row: variance 0, xhat exactly 0, the output is b (rounded to the output type), bit for bit
            want = inp["b"] if out_f32 else inp["b"].to(E.DTYPE[kind])
            assert torch.equal(ref["out"][0], inp["b"].double())
            assert E.exact_ratio(got["out"][0], want)[0] == 0.0
    for form, r in top.items():
        print(f"[{form}, {kind}] worst error / budget over the widths: out {r:.3f}")


def test_ln_depth_counts_this_kernels_tree():
    assert [E.ln_depth(D) for D in (8, 384, 512, 1024, 1280, 1536, 2048)] == [14, 14, 14, 22, 30, 30, 38]
    assert sorted({D for _, D, _, _, gap in E.ln_cases() if gap}) == [384, 1280] and len(E.ln_cases()) == 7 * 3 + 2 * 2


# the widths where each bug can show at all: a chunk k >= 1 exists past D = 512; idle lanes in the ragged chunk and a padded width
# different from D exist where D is no multiple of 512; a neighbouring row needs M > 1
_LN_WHERE = {"eps": lambda M, D: M > 1, "var_unbiased": lambda M, D: True, "neighbour_row": lambda M, D: M > 1,
             "wb_prev_chunk": lambda M, D: D > 512, "dead_lanes": lambda M, D: D % 512 != 0, "mean_padded": lambda M, D: D % 512 != 0}


@pytest.mark.parametrize("mutation", E.LN_MUTATIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_ln_mutations_leave_the_budget(kind, mutation):
    """Per kernel form: the bug is outside the budget in at least one width; in the fp32-out form (no output rounding to hide
    behind) in EVERY width where the bug can show at all."""
    seen = {}
    for M, D, entry, out_f32 in LN_VALUE_CASES:
        inp, ref = _ln(kind, M, D, entry, out_f32)
        r, _ = _ratio(E.ln_restatement(inp, out_f32, mutation), ref)
        can = _LN_WHERE[mutation](M, D)
        if not can:
            assert r <= 0.6, (mutation, M, D, r)           # the mutation changes nothing here
        elif out_f32 and not (mutation == "eps" and M == 1):
            assert r > 1.0, (mutation, kind, M, D, r)
        seen.setdefault((entry, out_f32), []).append(r)
    for form, rs in seen.items():
        assert max(rs) > 1.0, (mutation, kind, form, rs)
        print(f"[ln_affine {mutation}, {kind}, {form}] ratio {min(rs):.3g} .. {max(rs):.3g}")


# ----------------------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("kind", KINDS)
def test_clip_tokens_reference_is_the_eager_chain(kind):
    dt = E.DTYPE[kind]
    for B, T, D in E.TOK_SHAPES:
        inp = E.tok_inputs(B, T, D, kind, 1)
        ref = E.clip_tokens_reference(inp)
        cls = inp["cls"].to(dt).expand(B, 1, D)
        eager = (torch.cat([cls, inp["patches"].view(B, T - 1, D)], 1).float() + inp["pos"].to(dt).float()).to(dt)
        assert ref.dtype == dt and E.exact_ratio(ref, eager)[0] == 0.0
        assert float(inp["pos"][0].abs().min()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_vit_tokens_reference_is_cat_plus_pos(kind):
    for B, T, D, n in E.vit_shapes():
        inp = E.tok_inputs(B, T, D, kind, n)
        ref = E.vit_tokens_reference(inp)
        eager = torch.cat([inp["cls"][None].expand(B, n, D), inp["patches"].float().view(B, T - n, D)], 1) + inp["pos"]
        assert ref.dtype == torch.float32 and E.exact_ratio(ref, eager)[0] == 0.0
        assert float(inp["pos"][:max(n, 1)].abs().min()) > 0       # a wrong pos row shows in the prefix rows too


def test_vit_prefix_shapes_keep_a_patch_row():
    """Three shapes times three prefix counts, T > nprefix throughout."""
    run = E.vit_shapes()
    assert len(run) == 9 and all(T > n for _, T, _, n in run) and {n for *_, n in run} == {0, 1, 5}


@pytest.mark.parametrize("mutation", E.CLIP_TOK_MUTATIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_clip_tokens_mutations_differ(kind, mutation):
    rs = []
    for B, T, D in E.TOK_SHAPES:
        inp = E.tok_inputs(B, T, D, kind, 1)
        rs.append(E.exact_ratio(E.clip_tokens_reference(inp, mutation), E.clip_tokens_reference(inp))[0])
    if mutation == "cls_unrounded" and kind == "fp32":
        assert max(rs) == 0.0          # the operand type is fp32: there is no rounding to forget, the mutation is no bug here
    else:
        assert max(rs) > 1.0, (mutation, kind, rs)
    print(f"[clip_tokens {mutation}, {kind}] ratio {min(rs):.3g} .. {max(rs):.3g}")


@pytest.mark.parametrize("mutation", E.VIT_TOK_MUTATIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_vit_tokens_mutations_differ(kind, mutation):
    rs = []
    for B, T, D, n in E.vit_shapes():
        inp = E.tok_inputs(B, T, D, kind, n)
        r = E.exact_ratio(E.vit_tokens_reference(inp, mutation), E.vit_tokens_reference(inp))[0]
        if n == 0:
            assert r == 0.0            # without prefix rows t - nprefix = t, T - nprefix = T and no prefix row reads pos
        rs.append(r)
    assert max(rs) > 1.0, (mutation, kind, rs)
    print(f"[vit_tokens {mutation}, {kind}] ratio {min(rs):.3g} .. {max(rs):.3g}")


# ------------------------------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("kind", KINDS)
def test_im2col_reference_is_unfold(kind):
    for B, S, P, Kp in E.IM2COL_SHAPES:
        inp = E.im2col_inputs(B, S, P, Kp)
        ref = E.im2col_reference(inp, kind)
        K = 3 * P * P
        unf = torch.nn.functional.unfold(inp["img"], P, stride=P).transpose(1, 2).reshape(-1, K).to(E.DTYPE[kind])
        assert ref.shape == (B * (S // P) ** 2, Kp) and E.exact_ratio(ref[:, :K], unf)[0] == 0.0
        assert E.exact_ratio(ref[:, K:], torch.zeros(ref.shape[0], Kp - K))[0] == 0.0
        for mutation in E.IM2COL_MUTATIONS:
            r = E.exact_ratio(E.im2col_reference(inp, kind, mutation), ref)[0]
            if mutation == "pad_unwritten" and Kp == K:
                assert r == 0.0        # no pad columns
            else:
                assert r > 1.0, (mutation, kind, (B, S, P, Kp))


# --------------------------------------------------------------------------------------------------------------- preprocess
def test_cubic_constants():
    """L and LAMBDA as computed on the grid, against their closed forms at t = 1/2; the weights sum to 1 (orders 0 and 1 are one
    function); the coordinate term is exactly 0 where nothing rounds and positive elsewhere."""
    assert abs(E.CUBIC_L - 3.0) < 1e-9 and abs(E.CUBIC_LAMBDA - 1.375) < 1e-9
    t = torch.linspace(0, 1, 1001, dtype=torch.float64)
    assert float((E._cubic(t).sum(-1) - 1).abs().max()) < 1e-14     # fp64 roundings of the four cubics
    assert float(E.coord_err(16, 8).abs().max()) == 0.0
    assert float(E.coord_err(16, 14).min()) > 0 and float(E.coord_err(8, 12).min()) > 0
    print(f"[bicubic A = -0.75] L = sup sum|c_j'| = {E.CUBIC_L:.6f}, LAMBDA = sup sum|c_j| = {E.CUBIC_LAMBDA:.6f}")


def test_pre_horner_error_bound_holds():
    """COEF_ERR against the fp32 Horner evaluation itself on a fine grid of fractions: inside 0.6 of the bound."""
    t = torch.linspace(0, 1, 200001, dtype=torch.float64).float()
    err = (E._cubic(t).double() - E._cubic(t.double())).abs().amax(0)
    assert (err <= 0.6 * E.COEF_ERR).all(), (err / E.COEF_ERR)
    print("[bicubic weights, fp32 Horner] worst error / bound per tap: " + ", ".join(f"{float(v):.3f}" for v in err / E.COEF_ERR))


@pytest.mark.parametrize("case", E.PRE_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}o{c[3]}{'odd' if c[4] is E.ODD_MEAN else ''}")
def test_pre_restatement_and_torch_stay_inside(case):
    B, R, S, order, mean, std = case
    inp, ref = _pre(case)
    r, i = _ratio(E.pre_restatement(inp, S, order, mean, std), ref)
    rt, it = _ratio(E.pre_torch(inp, S, order, mean, std), ref)
    print(f"[preprocess {(B, R, S, order)} mean {mean[0]:.2f}..] worst error / budget: restatement {r:.3f}, torch fp32 {rt:.3f}")
    assert r <= 0.6, (r, i)
    assert rt <= 1.0, (rt, it)
    if S != R:      # one reference serves both orders: the other order's fp32 result is inside ITS budget against the same values
        other = E.pre_reference(inp, S, 1 - order, mean, std)
        assert float((other["out"] - ref["out"]).abs().max()) <= 1e-13 * float(ref["out"].abs().max())
    if B > 1:
        assert set(inp["raw"][1].unique().tolist()) == {0, 255}


# where each bug can show: resampling bugs need S != R; taps outside the image on both sides need the upsampling case, one
# outside any resampling; exchanged weights need fractions that differ between rows and columns (16 -> 8 has 1/2 everywhere);
# per-channel statistics and the divisor show everywhere
_PRE_WHERE = {"a_half": lambda R, S: S != R, "align_corners": lambda R, S: S != R, "reflect": lambda R, S: S != R,
              "clamp_one_deep": lambda R, S: S > R, "swap_cy_cx": lambda R, S: R % S != 0, "channel0_stats": lambda R, S: True,
              "div_256": lambda R, S: True}


@pytest.mark.parametrize("mutation", E.PRE_MUTATIONS)
def test_pre_mutations_leave_the_budget(mutation):
    rs = []
    for case in E.PRE_CASES:
        B, R, S, order, mean, std = case
        inp, ref = _pre(case)
        r, _ = _ratio(E.pre_restatement(inp, S, order, mean, std, mutation), ref)
        if _PRE_WHERE[mutation](R, S):
            assert r > 1.0, (mutation, case[:4], r)
        else:
            assert r <= 0.6, (mutation, case[:4], r)
        rs.append(r)
    print(f"[preprocess {mutation}] ratio {min(rs):.3g} .. {max(rs):.3g}")
