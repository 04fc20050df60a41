"""The error budgets of tests/embed_ref.py, proven on the CPU before tests/test_embed_gpu.py relies on them (the two conditions of
tests/test_rowpass_budgets_cpu.py and tests/test_adaln_budgets_cpu.py), for every operation, build type and shape of the GPU tests:

(a) the fp32 restatement of each kernel's own order of operations stays at or below 0.6 of every budget;
(b) every realistic bug of exactly these kernels leaves the budget of the output where it is made by a factor above 20.

A (mutation, shape) pair at which the mutation changes nothing is left out BY NAME, with the reason, next to the parametrisation;
the factor is never lowered.  Each worst ratio is printed.
"""
import pytest
import torch

from tests import embed_ref as E
from tests.rowpass_ref import KINDS
from tests.test_oracle_golden import load

_CACHE = {}


def _smallk(kind, shape, wide_f32):
    """(inputs, stage-1 partials of the restatement) of one small-K case: computed once, shared, never modified."""
    key = ("smallk", kind, shape, wide_f32)
    if key not in _CACHE:
        inp = E.smallk_inputs(*shape, kind, wide_f32)
        _CACHE[key] = (inp, E.smallk_stage1(inp))
    return _CACHE[key]


def _patch(kind, shape):
    key = ("patch", kind, shape)
    if key not in _CACHE:
        inp = E.patch_inputs(*shape, kind)
        _CACHE[key] = (inp, {True: E.patch_reference(inp, True), False: E.patch_reference(inp, False)})
    return _CACHE[key]


def _label(kind, shape, drop):
    key = ("label", kind, shape, drop)
    if key not in _CACHE:
        inp = E.label_inputs(*shape, kind, drop)
        _CACHE[key] = (inp, E.label_reference(inp))
    return _CACHE[key]


def _show(tag, ratios, fmt=".3f"):
    print(f"[{tag}] worst error / budget: " + ", ".join(f"{k} {v[0]:{fmt}}" for k, v in ratios.items()))


# ------------------------------------------------------------------------------------------------------- small-K wgrad
@pytest.mark.parametrize("wide_f32", [True, False])
@pytest.mark.parametrize("shape", E.SMALLK_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_smallk_restatement_stays_inside(kind, shape, wide_f32):
    inp, parts = _smallk(kind, shape, wide_f32)
    for layout in (0, 1):
        for accumulate in (False, True):
            ref = E.smallk_reference(inp, layout, accumulate)
            ratios = E.ratios(E.smallk_reduce(parts, inp, layout, accumulate), ref, E.SMALLK_OUTPUTS)
            _show(f"small-K restatement, {kind}, {shape}, wide {'fp32' if wide_f32 else kind}, layout {layout}, accumulate={accumulate}",
                  ratios)
            assert set(ratios) == set(E.SMALLK_OUTPUTS)
            for k, (r, i) in ratios.items():
                assert r <= 0.6, (k, r, i)


# accumulate_overwrite runs with accumulate on (off, there is no prior value to lose).  No other pair is a no-op at these shapes:
# every shape has a slice whose row count is no multiple of RG (tail_unmasked), slice 0 is never empty (drop_slice, drop_last_row),
# and Dw != KS everywhere (layout_swap).
@pytest.mark.parametrize("mutation", E.SMALLK_MUTATIONS)
@pytest.mark.parametrize("shape", E.SMALLK_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_smallk_budgets_reject_the_bugs(kind, shape, mutation):
    M, Dw, KS = shape
    per, rg = -(-M // E.NSL), E.smallk_rg(KS)
    assert any(n % rg for n in {min(per, M - z * per) for z in range(E.NSL) if z * per < M}) and Dw != KS
    for wide_f32 in (True, False):
        inp, _ = _smallk(kind, shape, wide_f32)
        parts = E.smallk_stage1(inp, mutation) if mutation in E.SMALLK_STAGE1_MUTATIONS else _smallk(kind, shape, wide_f32)[1]
        for layout in (0, 1):
            for accumulate in ((True,) if mutation == "accumulate_overwrite" else (False, True)):
                ref = E.smallk_reference(inp, layout, accumulate)
                ratios = E.ratios(E.smallk_reduce(parts, inp, layout, accumulate, mutation), ref, E.SMALLK_OUTPUTS)
                _show(f"small-K {mutation}, {kind}, {shape}, wide {'fp32' if wide_f32 else kind}, layout {layout}, "
                      f"accumulate={accumulate}", ratios, ".3g")
                assert ratios["out"][0] > 20, ratios
                if mutation in ("tail_unmasked", "drop_last_row", "drop_slice", "accumulate_overwrite"):
                    assert ratios["cw"][0] > 20, ratios
                if mutation in ("drop_last_row", "drop_slice", "accumulate_overwrite"):
                    assert ratios["cs"][0] > 20, ratios


def test_smallk_cases_reach_every_instantiation_and_tail():
    forms = {E.smallk_form(KS, w) for _, _, KS in E.SMALLK_SHAPES for w in (True, False)}
    assert {f for f, _ in forms} == {f"smallk_wgrad_kernel<{w}, {k}>" for w in ("true", "false") for k in (16, 32)}
    assert {z for _, z in forms} == {1, 2, 8}
    pers = {-(-M // E.NSL) for M, _, _ in E.SMALLK_SHAPES}
    assert {1, 2, 10} <= pers
    assert {KS % 32 for _, _, KS in E.SMALLK_SHAPES if KS > 16} >= {0, 8, 24}      # KSP = 32: whole, one live 8-chunk, three
    assert any(Dw % 128 for _, Dw, _ in E.SMALLK_SHAPES)


# ------------------------------------------------------------------------------------------- patchify and patch embed
@pytest.mark.parametrize("shape", E.PATCH_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_patch_embed_restatement_stays_inside(kind, shape):
    inp, refs = _patch(kind, shape)
    for bias in (True, False):
        ratios = E.ratios(E.patch_restatement(inp, bias), refs[bias], ("tok",))
        _show(f"patch embed restatement, {kind}, {shape}, bias={bias}", ratios)
        assert ratios["tok"][0] <= 0.6, ratios
    # the probe: lin = 0 exactly at the last token, column D - 1, and pos = 0 there
    assert float(refs[True]["tok"][-1, -1]) == 0.0 and float(refs[False]["tok"][-1, -1]) == 0.0


# pos_neighbour: a single token (G = 1) is its own neighbour; x_unrounded: the rounding is the identity in the fp32 build
@pytest.mark.parametrize("kind,shape,mutation", [(k, s, m) for k in KINDS for m in E.PATCH_MUTATIONS for s in E.PATCH_SHAPES
                                                 if not (m == "pos_neighbour" and s[2] == s[3])
                                                 and not (m == "x_unrounded" and k == "fp32")])
def test_patch_embed_budgets_reject_the_bugs(kind, shape, mutation):
    inp, refs = _patch(kind, shape)
    ratios = E.ratios(E.patch_restatement(inp, True, mutation), refs[True], ("tok",))
    _show(f"patch embed {mutation}, {kind}, {shape}", ratios, ".3g")
    assert ratios["tok"][0] > 20, ratios


def test_patch_index_map_is_the_golden_map_and_the_permute():
    """patch_src_index (the kernel's integer arithmetic restated) against the reference's own patchify map at the size the goldens
    cover, and against the reshape / permute form at every test shape, in both orders."""
    gs = load("static")
    idx = torch.from_numpy(gs["patchify_idx"]).flatten().long()
    assert torch.equal(E.patch_src_index(1, 4, 32, 2, 0), idx)
    for B, C, HW, P, _ in E.PATCH_SHAPES:
        flat = torch.arange(B * C * HW * HW, dtype=torch.float64).reshape(B, C, HW, HW)
        for order in (0, 1):
            i = E.patch_src_index(B, C, HW, P, order)
            assert sorted(i.tolist()) == list(range(flat.numel()))           # a permutation
            assert torch.equal(flat.flatten()[i], E.patches(flat, C, P, order).flatten())


def test_embed_form_rule():
    """The register form takes K = 16 at widths up to 1280 that are multiples of 4, aligned; everything else is the generic kernel."""
    assert E.embed_form("bf16", 16, 1152, True) == "reg16" and E.embed_form("fp32", 16, 1280, True) == "reg16"
    assert E.embed_form("bf16", 16, 1284, True) == "generic" and E.embed_form("fp16", 16, 1152, False) == "generic"
    assert E.embed_form("bf16", 64, 260, True) == "generic" and E.embed_form("bf16", 16, 6, True) == "generic"
    forms = {E.embed_form("bf16", C * P * P, D, True) for _, C, _, P, D in E.PATCH_SHAPES}
    assert forms == {"reg16", "generic"}
    assert {C * P * P for _, C, _, P, _ in E.PATCH_SHAPES} == {8, 16, 64, 256}


# ------------------------------------------------------------------------------------------------------------ sinusoid
@pytest.mark.parametrize("dim,max_period", E.SIN_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_sinusoid_restatement_stays_inside(kind, dim, max_period):
    inp = E.sin_inputs(kind)
    ref = E.sin_reference(inp, dim, max_period)
    got = E.sin_restatement(inp, dim, max_period)
    ratios = E.ratios(got, ref, ("out",))
    _show(f"sinusoid restatement, {kind}, dim {dim}, max_period {max_period:g}", ratios)
    assert ratios["out"][0] <= 0.6, ratios
    if dim % 2:
        assert (ref["out"][:, -1] == 0).all() and (got["out"][:, -1] == 0).all()


# no_max_period: at half = 1 the only frequency is exp(0) = 1 whatever max_period is: it cannot show at dim = 2
# odd_unwritten: an even dim has no such column
@pytest.mark.parametrize("dim,max_period,mutation", [(d, p, m) for m in E.SIN_MUTATIONS for d, p in E.SIN_CASES
                                                     if not (m == "no_max_period" and d // 2 == 1)
                                                     and not (m == "odd_unwritten" and d % 2 == 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_sinusoid_budgets_reject_the_bugs(kind, dim, max_period, mutation):
    inp = E.sin_inputs(kind)
    ratios = E.ratios(E.sin_restatement(inp, dim, max_period, mutation), E.sin_reference(inp, dim, max_period), ("out",))
    _show(f"sinusoid {mutation}, {kind}, dim {dim}, max_period {max_period:g}", ratios, ".3g")
    assert ratios["out"][0] > 20, ratios


def test_sinusoid_reference_is_the_golden_table():
    """The fp64 reference at dim 256, max_period 10000 against the reference implementation's recorded fp32 table."""
    gs = load("static")
    inp = dict(t=torch.from_numpy(gs["sinus_t"]).float(), kind="fp32")
    ref = E.sin_reference(inp, 256, 10000.0)
    torch.testing.assert_close(ref["out"].float(), torch.from_numpy(gs["sinus"]).float(), atol=2e-6, rtol=0)


# -------------------------------------------------------------------------------------------------- label conditioning
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("shape", E.LABEL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_label_restatement_stays_inside(kind, shape, drop):
    inp, ref = _label(kind, shape, drop)
    got = E.label_restatement(inp)
    ratios = E.ratios(got, ref, E.LABEL_OUTPUTS)
    _show(f"label conditioning restatement, {kind}, {shape}, drop={drop}", ratios)
    assert set(ratios) == set(E.LABEL_OUTPUTS)
    assert torch.equal(got["eff"], ref["eff"]) and torch.equal(got["c"], ref["c32"])      # exact
    for k, (r, i) in ratios.items():
        assert r <= 0.6, (k, r, i)
    B, D, NC = shape
    # duplicates, an untouched row wherever the table has more rows than the batch can select, and every special value of c
    if B > 1:
        assert len(set(ref["eff"].tolist())) < B
    assert set(E.C_SPECIAL[:B * D]) <= set(ref["c"].flatten().tolist())
    if drop:
        assert int(inp["drop"].sum()) >= 1 and (ref["eff"][inp["drop"].bool()] == NC).all()


def test_label_special_values_are_all_reached():
    assert any(set(E.C_SPECIAL) <= set(_label("bf16", s, False)[1]["c"].flatten().tolist()) for s in E.LABEL_SHAPES)


# drop_not_null needs a drop mask (every case with one drops at least one sample whose label is not the null row);
# dsilu_unrounded: the rounding is the identity in the fp32 build
@pytest.mark.parametrize("kind,shape,mutation", [(k, s, m) for k in KINDS for m in E.LABEL_MUTATIONS for s in E.LABEL_SHAPES
                                                 if not (m == "dsilu_unrounded" and k == "fp32")])
def test_label_budgets_reject_the_bugs(kind, shape, mutation):
    inp, ref = _label(kind, shape, True)
    ratios = E.ratios(E.label_restatement(inp, mutation), ref, E.LABEL_OUTPUTS)
    _show(f"label conditioning {mutation}, {kind}, {shape}", ratios, ".3g")
    where = {"drop_not_null": "c", "dsilu_unrounded": "dtable", "dtable_overwrite": "dtable", "batch_short": "dtable"}[mutation]
    assert ratios[where][0] > 20, (where, ratios)
    if mutation == "drop_not_null":
        assert ratios["silu_c"][0] > 20, ratios
    if mutation == "batch_short":
        assert ratios["dt_emb"][0] > 20, ratios
