"""The error budgets of tests/input_grad_ref.py, proven on the CPU before tests/test_input_grad_gpu.py relies on them (the two
conditions of tests/test_embed_budgets_cpu.py), for both kernels, every build type, shape and kernel form of the GPU tests:

(a) the fp32 restatement of each kernel's own order of operations stays at or below 0.6 of every budget;
(b) every realistic bug of exactly these kernels leaves the budget of the output it damages by a factor of 20 or more.

A (mutation, shape) pair at which the mutation changes nothing is left out BY NAME, with the reason, next to the parametrisation;
the factor is never lowered.  Each worst ratio is printed.
"""
import pytest
import torch

from tests import embed_ref as E
from tests import input_grad_ref as R
from tests.rowpass_ref import KINDS

_CACHE = {}
FORMS = ("stream16", "generic")


def _forms(shape):
    """The forms the GPU test reaches at a shape: the entry point's choice at aligned addresses, and at K = 16 the generic kernel
    too (a weight at 8 (mod 16))."""
    _, C, _, P, D = shape
    first = R.bwdx_form(C * P * P, D, True)
    return (first,) if first == "generic" else FORMS


def _bwdx(kind, shape, form):
    """(inputs, reference) of one case: computed once, shared, never modified."""
    key = (kind, shape)
    if key not in _CACHE:
        _CACHE[key] = R.bwdx_inputs(*shape, kind)
    if key + (form,) not in _CACHE:
        _CACHE[key + (form,)] = R.bwdx_reference(_CACHE[key], form)
    return _CACHE[key], _CACHE[key + (form,)]


def _show(tag, ratios, fmt=".3f"):
    print(f"[{tag}] worst error / budget: " + ", ".join(f"{k} {v[0]:{fmt}}" for k, v in ratios.items()))


# ----------------------------------------------------------------------------------------------- patch embed, dL/dx
@pytest.mark.parametrize("shape", R.PATCH_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_bwdx_restatement_stays_inside(kind, shape):
    for form in _forms(shape):
        inp, ref = _bwdx(kind, shape, form)
        ratios = E.ratios(R.bwdx_restatement(inp, form), ref, ("dx",))
        _show(f"patch embed dL/dx restatement, {kind}, {shape}, {form}", ratios)
        assert ratios["dx"][0] <= 0.6, ratios
        assert bool(torch.isfinite(ref["dx"]).all())                # the index map writes every element of dx
        # the probe: an exact 0 at the last token, k = K - 1
        B, C, HW, P, D = shape
        last = E.patch_src_index(B, C, HW, P, 0)[-1]
        assert float(ref["dx"][last]) == 0.0 and float(ref["b_dx"][last]) > 0.0


def _noop(kind, shape, form, mutation):
    B, C, HW, P, D = shape
    return ((mutation == "ph_pw_swapped" and HW == P)               # one token per sample: it is its own transpose
            or (mutation == "d_tail_dropped" and R.bwdx_tail(form, D) is None)   # D fills the form's groups of columns exactly
            or (mutation == "dtok_unrounded" and kind == "fp32"))   # the rounding is the identity in the fp32 build


@pytest.mark.parametrize("kind,shape,form,mutation", [(k, s, f, m) for k in KINDS for m in R.BWDX_MUTATIONS for s in R.PATCH_SHAPES
                                                      for f in _forms(s) if not _noop(k, s, f, m)])
def test_bwdx_budgets_reject_the_bugs(kind, shape, form, mutation):
    inp, ref = _bwdx(kind, shape, form)
    ratios = E.ratios(R.bwdx_restatement(inp, form, mutation), ref, ("dx",))
    _show(f"patch embed dL/dx {mutation}, {kind}, {shape}, {form}", ratios, ".3g")
    assert ratios["dx"][0] >= 20, ratios


def test_bwdx_cases_reach_every_form_and_tail():
    forms = {R.bwdx_form(C * P * P, D, True) for _, C, _, P, D in R.PATCH_SHAPES}
    assert forms == set(FORMS)
    assert R.bwdx_form(16, 1280, True) == "stream16" and R.bwdx_form(16, 1284, True) == "generic"
    assert R.bwdx_form(16, 1152, False) == "generic" and R.bwdx_form(64, 1152, True) == "generic"
    stream = [(B * (HW // P) ** 2, D) for B, C, HW, P, D in R.PATCH_SHAPES if R.bwdx_form(C * P * P, D, True) == "stream16"]
    assert any(bt % 2 for bt, _ in stream) and any(bt > 32 and bt % 32 for bt, _ in stream)          # a single last token; > 1 block
    assert any(D % 256 == 0 and D > 256 for _, D in stream) and any(D > 256 and D % 256 for _, D in stream) and any(D < 256 for _, D in stream)
    assert {C * P * P for _, C, _, P, _ in R.PATCH_SHAPES} == {8, 16, 64, 256}
    # the tree: 4 columns per trip and lane in the streaming form, one per trip in the generic one
    assert R.tree_depth("stream16", 1280) == 20 + 6 and R.tree_depth("stream16", 4) == 4 + 6
    assert R.tree_depth("generic", 1284) == 21 + 6 and R.tree_depth("generic", 72) == 2 + 6
    for form in FORMS:
        for D in (4, 72, 328, 1280):
            assert sorted(d for c in R.lane_columns(form, D) for d in c) == list(range(D))


# ------------------------------------------------------------------------------------------------- sinusoid, dL/dt
@pytest.mark.parametrize("dim,max_period", E.SIN_CASES)
def test_sinusoid_bwd_restatement_stays_inside(dim, max_period):
    inp = R.sinb_inputs(dim)
    ratios = E.ratios(R.sinb_restatement(inp, max_period), R.sinb_reference(inp, max_period), ("dt",))
    _show(f"sinusoid dL/dt restatement, dim {dim}, max_period {max_period:g}", ratios)
    assert ratios["dt"][0] <= 0.6, ratios


# no_f: at half = 1 the only frequency is exp(0) = 1: leaving it out changes nothing at dim = 2
# pad_counted: an even dim has no padding column
@pytest.mark.parametrize("dim,max_period,mutation", [(d, p, m) for m in R.SINB_MUTATIONS for d, p in E.SIN_CASES
                                                     if not (m == "no_f" and d // 2 == 1) and not (m == "pad_counted" and d % 2 == 0)])
def test_sinusoid_bwd_budgets_reject_the_bugs(dim, max_period, mutation):
    inp = R.sinb_inputs(dim)
    ratios = E.ratios(R.sinb_restatement(inp, max_period, mutation), R.sinb_reference(inp, max_period), ("dt",))
    _show(f"sinusoid dL/dt {mutation}, dim {dim}, max_period {max_period:g}", ratios, ".3g")
    assert ratios["dt"][0] >= 20, ratios


def test_sinusoid_bwd_reference_is_autograd_of_the_forward():
    """The fp64 reference against torch.autograd through the reference's own expression of the table."""
    import math
    for dim, max_period in E.SIN_CASES:
        inp = R.sinb_inputs(dim)
        half = dim // 2
        t = inp["t"].double().requires_grad_(True)
        f = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
        tab = torch.cat([torch.cos(t[:, None] * f), torch.sin(t[:, None] * f)], 1)
        (tab * inp["dsin"].double()[:, :2 * half]).sum().backward()
        torch.testing.assert_close(R.sinb_reference(inp, max_period)["dt"], t.grad, rtol=1e-12, atol=1e-12)


def test_bwdx_reference_is_autograd_of_the_convolution():
    """The fp64 reference against torch.autograd through F.conv2d (what the reference model's autograd does)."""
    for shape in ((5, 4, 18, 2, 1280), (3, 4, 12, 4, 260), (3, 2, 6, 2, 72)):
        B, C, HW, P, D = shape
        inp, ref = _bwdx("bf16", shape, R.bwdx_form(C * P * P, D, True))
        x = torch.zeros(B, C, HW, HW, dtype=torch.float64, requires_grad=True)
        tok = torch.nn.functional.conv2d(x, inp["w"].double().reshape(D, C, P, P), None, stride=P).flatten(2).transpose(1, 2)
        g = inp["dtok"].to(torch.bfloat16).double().reshape(B, -1, D)
        (tok * g).sum().backward()
        torch.testing.assert_close(ref["dx"].reshape(B, C, HW, HW), x.grad, rtol=1e-12, atol=1e-12)
