"""The error budgets of tests/attention_ref.py, proven on the CPU before tests/test_attention_ref_gpu.py relies on them.  For every
cell of the table, both 16-bit builds, every T and flavour:

(a) the fp32 restatement of the kernel's own order of operations stays at or below 0.6 of every budget;
(b) every realistic bug of exactly this code (attention_ref.MUTATIONS) leaves the budget of an output it touches by a factor above
    20 at one (T, flavour) of the cell at least.  Which (mutation, cell, T) can hold the bug at all is attention_ref.mutation_applies;
    a pair where an applicable mutation changes nothing is left out BY NAME in NO_OP below, with the reason.  The factors are never
    lowered;
(a') the sharp backward check the tests use (delta from the O the kernel is given) implies the stated one (delta from the exact
    O, the O-rounding term in the budget): attention_ref's docstring says why the stated one cannot hold (a) at its factor;
(c) the guard check and the finiteness check of attention_ref.Band fail on a planted write one row past T of the last batch and on
    a NaN in a live element, planted in a copy of the restatement's output.

Each worst ratio is printed.
"""
import math

import pytest
import torch

from tests import attention_ref as A

_INP, _REF = {}, {}


def _case(ci, T, kind, flavour):
    """One case's inputs and (reference, budget) pairs: computed once, shared by the restatement and every mutation, never modified
    (the T x T matrices behind them are gone by then: only [B H, T, hd] arrays are kept)."""
    key = (ci, T, kind, flavour)
    if key not in _INP:
        if any(k[0] != ci for k in _INP):               # the tests run cell by cell: one cell's cases are kept
            _INP.clear(), _REF.clear()
        _INP[key] = A.inputs(ci, T, kind, flavour)
        _REF[key] = A.reference(_INP[key])
    return _INP[key], _REF[key]


def _dbl(out):
    return {k: v.double() for k, v in out.items()}


@pytest.mark.parametrize("kind", A.KINDS16)
@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_restatement_stays_inside(case, kind):
    ci, T = case
    for fl in A.flavours(A.CELLS[ci], kind):
        inp, ref = _case(ci, T, kind, fl)
        assert all(torch.isfinite(r).all() and torch.isfinite(b).all() for r, b in ref.values()), "the reference is not finite"
        rat = A.ratios(_dbl(A.restatement(inp)), ref)
        print(f"[{A.case_id(case)} {kind} {fl}] " + ", ".join(f"{k} {v[0]:.3f}" for k, v in rat.items()))
        for k, (r, i) in rat.items():
            assert r <= 0.6, (k, r, A.decode(inp, k, i), fl)


@pytest.mark.parametrize("kind", A.KINDS16)
@pytest.mark.parametrize("case", [c for c in A.CASES if A.CELLS[c[0]].entry != "fwd" and not A.CELLS[c[0]].reserve], ids=A.case_id)
def test_sharp_backward_check_implies_the_stated_one(case, kind):
    """attention_ref's docstring, delta: budget_sharp + |ref_sharp - ref_stated| <= budget_stated for every element, so whatever is
    inside the sharp budget is inside the stated one.  (Per item the same arithmetic: the 99-item cells are left to the (2, 3) ones.)"""
    ci, T = case
    for fl in A.flavours(A.CELLS[ci], kind):
        inp, sharp = _case(ci, T, kind, fl)
        stated = A.reference(inp, stated=True)
        for k in sharp:
            slack = stated[k][1] - (sharp[k][1] + (sharp[k][0] - stated[k][0]).abs())
            assert (slack >= -1e-12 * stated[k][1]).all(), (k, fl, float(slack.min()))


# (mutation, cell id) at which an applicable mutation changes nothing, each with its reason.
NO_OP = {}

_PAIRS = [(m, ci) for ci, c in enumerate(A.CELLS) for m in A.MUTATIONS
          if any(A.mutation_applies(m, c, T) for T, _ in c.cases) and (m, A.cell_id(ci)) not in NO_OP]


@pytest.mark.parametrize("kind", A.KINDS16)
@pytest.mark.parametrize("mutation,ci", _PAIRS, ids=[f"{m}-{A.cell_id(ci)}" for m, ci in _PAIRS])
def test_mutation_leaves_the_budget(mutation, ci, kind):
    cell, best = A.CELLS[ci], 0.0
    for T, _ in sorted(cell.cases, key=lambda c: -c[0] if c[0] <= 600 else c[0]):     # the cheap sizes that say most first
        if not A.mutation_applies(mutation, cell, T):
            continue
        for fl in reversed(A.flavours(cell, kind)[:2]):
            inp, ref = _case(ci, T, kind, fl)
            rat = A.ratios(_dbl(A.restatement(inp, mutation)), ref)
            print(f"[{mutation} {A.case_id((ci, T))} {kind} {fl}] " + ", ".join(f"{k} {v[0]:.1f}" for k, v in rat.items()))
            best = max(best, max(v[0] for v in rat.values()))
            if best > 20:
                return
    assert best > 20, (mutation, A.cell_id(ci), kind, best)


@pytest.mark.parametrize("case", [c for c in A.CASES if c[1] in (1, 100, 320)], ids=A.case_id)
def test_guards_and_finiteness_see_a_planted_fault(case):
    ci, T = case
    inp, _ = _case(ci, T, "bf16", "unit")
    out = A.restatement(inp)

    def fresh():
        bufs = A.buffers(inp)
        A.store(inp, bufs, out)
        return bufs

    got = A.collect(inp, fresh())                       # the clean copy passes and round-trips
    assert all(torch.equal(got[k], out[k].to(torch.bfloat16).float() if k != "lse" else out[k]) for k in out)
    for name in A.OUTPUTS[inp["cell"].entry]:
        bufs = fresh()
        band = bufs[name]
        row = math.prod(band.shape[2:]) if name != "lse" else 1          # one token row of the last batch's item, past T
        band.full[band.guard + band.n:band.guard + band.n + row] = 1.0
        with pytest.raises(AssertionError, match="written behind"):
            A.collect(inp, bufs)
        bufs = fresh()
        bufs[name].full[bufs[name].guard - 1] = 0.0
        with pytest.raises(AssertionError, match="written in front"):
            A.collect(inp, bufs)
        bufs = fresh()
        bufs[name].live.view(-1)[bufs[name].n // 2] = math.nan
        with pytest.raises(AssertionError, match="not finite"):
            A.collect(inp, bufs)


def test_the_table_names_every_dispatch_branch():
    """Held by hand to the bottom of csrc/attention.hip (there is no host planner): every kernel of the file is named by a row."""
    named = " ".join(c.kernel for c in A.CELLS)
    for k in ("attn_fwd256v_kernel<64>", "attn_fwd256v_kernel<72>", "attn_fwd256p_kernel<64, false>", "attn_fwd256p_kernel<72, false>",
              "attn_fwd256p_kernel<80, *>", "attn_fwd_kernel<64>", "attn_fwd_kernel<72>", "attn_fwd_rows_kernel", "attn_fwd_kernel<64, true>",
              "attn_bwd_ks_kernel<64>", "attn_bwd_ks_kernel<72>", "attn_bwd_ksp_kernel<64>", "attn_bwd_ksp_kernel<72>",
              "attn_bwd_ring_kernel<64>", "attn_bwd_ring_kernel<72>", "attn_bwd_long_kernel<64>", "attn_bwd_long_kernel<72>",
              "attn_dq_reduce_kernel", "attn_delta_kernel", "attn_delta_combine_kernel"):
        assert k in named, k
    ids = [A.case_id(c) for c in A.CASES]
    assert len(set(ids)) == len(ids)
    print(f"{len(A.CELLS)} cells, {len(A.CASES)} (cell, T) cases per build")
