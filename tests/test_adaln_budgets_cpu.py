"""The error budgets of tests/adaln_ref.py, proven on the CPU before the GPU tests rely on them (the two conditions and the numbers
of tests/test_rowpass_budgets_cpu.py).

(a) the fp32 restatement of each kernel's own arithmetic stays at or below 0.6 of every budget, in all three builds' types, at
    every shape the GPU tests use: the kernel keeps the rest for the hardware's rsqrt, sqrt, division and FMA contraction;
(b) every realistic bug of exactly these kernels leaves the budget of the output where it is made by more than 20 times.

Three outputs of the gate backward (dy and the two chunk sums over rounded products) hang on dg = round(dx): a rounding flips
or it does not, so their error is 0 or the whole budget and `<= 0.6 budget` has no meaning for them.  Their condition (a) is
the one that does: the restatement's dx is inside 0.6 of its budget, so its dy, part_g and part_dy must lie inside the budgets
BUILT from 0.6 of dx's budget (adaln_ref.gate_reference, frac = 0.6).
"""
import pytest
import torch

from tests import adaln_ref as A
from tests.rowpass_ref import KINDS
from tests.test_oracle_golden import load

_CACHE = {}


def _case(family, kind, shape):
    """(inputs, fp64 reference) of one (family, build type, shape): computed once, shared, never modified."""
    key = (family, kind, shape)
    if key not in _CACHE:
        if family == "ln":
            inp = A.ln_inputs(*shape, kind)
            _CACHE[key] = (inp, A.ln_reference(inp))
        elif family == "bwd":
            inp = A.bwd_inputs(*shape, kind)
            _CACHE[key] = (inp, A.bwd_reference(inp))
        elif family == "final":
            inp = A.final_inputs(*shape, kind)
            _CACHE[key] = (inp, A.final_reference(inp))
        elif family == "mse":
            inp = A.mse_inputs(*shape)
            _CACHE[key] = (inp, A.mse_reference(inp))
        else:
            inp = A.cos_inputs(*shape, kind)
            _CACHE[key] = (inp, A.cos_reference(inp))
    return _CACHE[key]


def _show(tag, ratios, fmt=".3f"):
    print(f"[{tag}] worst error / budget: " + ", ".join(f"{k} {v[0]:{fmt}}" for k, v in ratios.items()))


# --------------------------------------------------------------------------------------------------------- (a) restatements
@pytest.mark.parametrize("shape", A.FWD_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_ln_forward_restatement_stays_inside(kind, shape):
    inp, ref = _case("ln", kind, shape)
    got = A.ln_restatement(inp)
    ratios = A.ratios(got, ref, ("h", "mean", "rstd"))
    _show(f"ln fwd restatement, {kind}, {shape}", ratios)
    assert set(ratios) == {"h", "mean", "rstd"}
    for k, (r, i) in ratios.items():
        assert r <= 0.6, (k, r, i)
    # the constant row: variance 0, xhat exactly 0, h = shift rounded to the type, bit for bit, in both
    want = inp["shift"][0]
    assert torch.equal(ref["h"][0], want.double())
    assert torch.equal(got["h"][0].view(torch.int32 if kind == "fp32" else torch.int16),
                       want.view(torch.int32 if kind == "fp32" else torch.int16))


@pytest.mark.parametrize("shape", A.BWD_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_ln_backward_restatement_stays_inside(kind, shape):
    inp, ref = _case("bwd", kind, shape)
    got = A.bwd_restatement(inp)
    ratios = A.ratios(got, ref, ("dx", "part"))
    ratios.update(A.ratios(got, A.bwd_reference(inp, frac=0.6), ("dy", "part_g", "part_dy")))
    _show(f"ln bwd restatement, {kind}, {shape}", ratios)
    assert set(ratios) == set(A.BWD_OUTPUTS)
    for k in ("dx", "part"):
        assert ratios[k][0] <= 0.6, (k, ratios[k])
    for k in ("dy", "part_g", "part_dy"):            # against the budgets built from 0.6 of dx's: see the module docstring
        assert ratios[k][0] <= 1.0, (k, ratios[k])
    if kind != "fp32":     # a 16-bit dy is pinned to the bit wherever dx cannot reach a rounding boundary: almost everywhere
        assert float((ref["b_dy"] == 0).double().mean()) > 0.95


@pytest.mark.parametrize("shape", A.FINAL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_final_layer_restatement_stays_inside(kind, shape):
    inp, ref = _case("final", kind, shape)
    for bias in (True, False):
        r = ref if bias else A.final_reference(inp, bias=False)
        got = A.final_restatement(inp, bias=bias)
        ratios = A.ratios(got, r, A.FINAL_OUTPUTS)
        _show(f"final layer restatement, {kind}, {shape}, bias={bias}", ratios)
        assert set(ratios) == set(A.FINAL_OUTPUTS)
        for k, (v, i) in ratios.items():
            assert v <= 0.6, (k, v, i)
        assert torch.equal(got["dlin"].double(), r["dlin"])          # round(dout) in the (pi, pj, c) order: exact


@pytest.mark.parametrize("shape", A.MSE_SHAPES)
def test_mse_interpolant_restatement_stays_inside(shape):
    inp, ref = _case("mse", None, shape)
    ratios = A.ratios(A.mse_restatement(inp), ref, A.MSE_OUTPUTS)
    _show(f"mse / interpolant / posterior restatement, {shape}", ratios)
    assert set(ratios) == set(A.MSE_OUTPUTS)
    for k, (v, i) in ratios.items():
        assert v <= 0.6, (k, v, i)


@pytest.mark.parametrize("shape", A.COS_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_cosine_restatement_stays_inside(kind, shape):
    inp, ref = _case("cos", kind, shape)
    ratios = A.cos_ratios(A.cos_restatement(inp), ref, inp)
    _show(f"cosine restatement, {kind}, {shape}", ratios)
    assert set(ratios) == set(A.COS_OUTPUTS)
    for k, (v, i) in ratios.items():
        assert v <= 0.6, (k, v, i)


# ------------------------------------------------------------------------------------------------------------ (b) mutations
@pytest.mark.parametrize("shape,mutation", [(s, m) for m in A.LN_MUTATIONS for s in A.FWD_SHAPES
                                            if not (m == "neighbour_sample" and s[0] == 1)])   # one sample has no neighbour
@pytest.mark.parametrize("kind", KINDS)
def test_ln_forward_budgets_reject_the_bugs(kind, shape, mutation):
    inp, ref = _case("ln", kind, shape)
    got = A.ln_restatement(inp, mutation=mutation)
    ratios = A.ratios(got, ref, ("h", "mean", "rstd"))
    _show(f"ln fwd {mutation}, {kind}, {shape}", ratios, ".3g")
    if mutation == "no_eps":
        # eps = 1e-6 on a variance of order 1 is a change of 5e-7 relative: a rounding apart on an ordinary row.  It shows on the
        # two rows built for it: the constant row (variance 0: rstd = 1 / 0) and the tiny-spread row (variance 1e-4: 0.5 %)
        M = inp["M"]
        for row in (0, M - 1):
            err = (got["rstd"].double()[row] - ref["rstd"][row]).abs()
            assert not (err <= ref["b_rstd"][row]), (row, float(err), float(ref["b_rstd"][row]))
        return
    where = {"neighbour_sample": "h", "biased_var": "rstd"}[mutation]      # a bf16 h cannot see 1 / (2 D) at D = 1280: rstd does
    assert ratios[where][0] > 20, (where, ratios)


# half_sums: the one-wave form (D not in BWD2) has no exchange to forget; gate_unrounded: bfround is the identity in the fp32 build
@pytest.mark.parametrize("kind,shape,mutation", [(k, s, m) for k in KINDS for m in A.BWD_MUTATIONS for s in A.BWD_SHAPES
                                                 if not (m == "half_sums" and s[2] not in A.BWD2)
                                                 and not (m == "gate_unrounded" and k == "fp32")])
def test_ln_backward_budgets_reject_the_bugs(kind, shape, mutation):
    inp, ref = _case("bwd", kind, shape)
    ratios = A.ratios(A.bwd_restatement(inp, mutation=mutation), ref, A.BWD_OUTPUTS)
    _show(f"ln bwd {mutation}, {kind}, {shape}", ratios, ".3g")
    if mutation == "gate_unrounded":
        # round(dx gate) against round(round(dx) gate): one rounding apart by nature.  It shows on the elements whose budget is 0
        # (dx cannot reach a rounding boundary, the reference's bits are required): any difference there is outside
        assert ratios["dy"][0] > 1, ratios
        return
    where = {"neighbour_sample": "dx", "half_sums": "dx", "dx_overwrite": "dx", "part_scaled": "part", "part_15": "part"}[mutation]
    assert ratios[where][0] > 20, (where, ratios)
    if mutation == "neighbour_sample":      # the gate vector of the wrong sample too
        assert ratios["dy"][0] > 20, ratios


# wrong_pair_sample: a pair straddles two samples only where T is odd; (1, 1) has neither a pair nor a neighbour
@pytest.mark.parametrize("shape,mutation", [(s, m) for m in A.FINAL_MUTATIONS for s in A.FINAL_SHAPES
                                            if not (m == "wrong_pair_sample" and s[1] % 2 == 0) and not (m != "no_bias" and s[0] == 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_final_layer_budgets_reject_the_bugs(kind, shape, mutation):
    inp, ref = _case("final", kind, shape)
    ratios = A.ratios(A.final_restatement(inp, mutation=mutation), ref, A.FINAL_OUTPUTS)
    _show(f"final layer {mutation}, {kind}, {shape}", ratios, ".3g")
    assert ratios["out"][0] > 20, ratios
    if mutation == "neighbour_sample":
        assert ratios["hbuf"][0] > 20, ratios


@pytest.mark.parametrize("shape,mutation", [(s, m) for m in A.MSE_MUTATIONS for s in A.MSE_SHAPES
                                            if not (m == "mse_tail" and s[1] % 256 == 0)])     # no tail to drop
def test_mse_budgets_reject_the_bugs(shape, mutation):
    inp, ref = _case("mse", None, shape)
    ratios = A.ratios(A.mse_restatement(inp, mutation=mutation), ref, A.MSE_OUTPUTS)
    _show(f"mse {mutation}, {shape}", ratios, ".3g")
    assert ratios[{"mse_tail": "mse", "mse_no_2": "dout"}[mutation]][0] > 20, ratios


# z_tail: nothing past column 256 at Z = 4; cos_wrong_sample: one sample has no other
@pytest.mark.parametrize("shape,mutation", [(s, m) for m in A.COS_MUTATIONS for s in A.COS_SHAPES
                                            if not (m == "z_tail" and s[2] <= 256) and not (m == "cos_wrong_sample" and s[0] == 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_cosine_budgets_reject_the_bugs(kind, shape, mutation):
    inp, ref = _case("cos", kind, shape)
    ratios = A.cos_ratios(A.cos_restatement(inp, mutation=mutation), ref, inp)
    _show(f"cosine {mutation}, {kind}, {shape}", ratios, ".3g")
    assert ratios[{"z_tail": "rowdot", "no_clamp": "rowdot", "cos_wrong_sample": "dzt"}[mutation]][0] > 20, ratios


# ------------------------------------------------------------------------------------------------ the references themselves
def test_cosine_reference_is_normalize_in_fp64():
    """The analytic reference against autograd through F.normalize(., dim=-1, eps=1e-12) in fp64, the clamp rows included."""
    for shape in ((3, 7, 260), (5, 1, 4)):
        inp, ref = _case("cos", "bf16", shape)
        B, T, Z = shape
        zt = inp["zt"].double().requires_grad_(True)
        a = torch.nn.functional.normalize(zt, dim=-1, eps=1e-12)
        b = torch.nn.functional.normalize(inp["z"].double(), dim=-1, eps=1e-12)
        rows = (a * b).sum(-1)
        loss = -rows.reshape(B, T).mean(1)
        (loss * inp["gs"].double()).sum().backward()
        torch.testing.assert_close(rows, ref["rowdot"], atol=1e-14, rtol=1e-12)
        torch.testing.assert_close(loss, ref["loss"], atol=1e-14, rtol=1e-12)
        torch.testing.assert_close(zt.grad, ref["dzt"], atol=0, rtol=1e-9)
        assert float(zt.grad[inp["zero_zt"]].abs().max()) > 1e8          # O(1 / eps) on the clamped row


def test_unpatchify_restatement_is_the_golden_map():
    """adaln_ref.unpatchify / patchify_out against the reference's own index map at the size the goldens cover."""
    gs = load("static")
    C, P, T = 4, 2, 256
    un = torch.from_numpy(gs["unpatchify_idx"]).flatten().long()          # out.flat[i] = lin.flat[un[i]]
    lin = torch.arange(T * P * P * C, dtype=torch.float64).reshape(1, T, P * P * C)
    out = A.unpatchify(lin, C, P)
    assert torch.equal(out.flatten().long(), un)
    assert torch.equal(A.patchify_out(out, C, P), lin)


def test_final_form_rule():
    """The XL-width weight leaves the LDS form in the fp32 build, and in the 16-bit builds once P P C = 32."""
    assert A.final_form("bf16", 4, 2, 1152, False, True) == "lds" and A.final_form("fp32", 4, 2, 1152, False, True) == "rows"
    assert A.final_form("bf16", 8, 2, 1152, False, True) == "rows" and A.final_form("bf16", 8, 2, 384, True, True) == "lds"
    assert A.final_form("fp16", 4, 2, 384, True, False) == "rows"
