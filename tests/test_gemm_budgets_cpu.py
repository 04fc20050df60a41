"""The error budgets of tests/gemm_ref.py, proven on the CPU before tests/test_gemm_epilogues_gpu.py relies on them, and the cell
table held to the planner.  For every cell (kernel, layout, epilogue) of the table, both 16-bit builds, every shape and call:

(a) the fp32 restatement of the kernel's own order of operations stays at or below 0.6 of every budget;
(b) every realistic bug of exactly this code (gemm_ref.MUTATIONS) leaves the budget of an output it touches by a factor above 20
    at one of the cell's shapes at least.  Which (mutation, cell, shape, call) can hold the bug at all is gemm_ref.mutation_applies;
    a pair where an applicable mutation changes nothing is left out BY NAME in NO_OP below, with the reason.  The factor is never
    lowered.

(c) the table against ops.gemm_plan (host arithmetic): every call of every cell plans exactly one launch of the cell's kernel (the
    persistent rows with the persistent grid and the tile walk they are there for), and over every kernel, layout and epilogue
    0..17 the dry run names the kernel IF AND ONLY IF the table has the cell: a new instantiation or a changed EPIS_* mask fails
    here until someone adds the cell.

Each worst ratio is printed.
"""
import pytest
import torch

from reed_amd import ops
from tests import gemm_ref as G

_INP, _ACC = {}, {}


def _inputs(sh, kind):
    """One shape's inputs, shared and never modified.  Of a shape with thousands of rows the first and the last 300 (the first row
    tile and the edge behind it, the last full tile, the ragged one and the zero row): gemm_ref.subset says why that proves the
    same thing."""
    if (sh, kind) not in _INP:
        inp = G.inputs(sh, kind)
        if sh.M > 2048:
            inp = G.subset(inp, torch.cat([torch.arange(300), torch.arange(sh.M - 300, sh.M)]))
        _INP[sh, kind] = inp
    return _INP[sh, kind]


def _acc(inp, var, mutation=None):
    """The restatement's K loop, shared by every epilogue of a shape (it depends on the split and the two K mutations only)."""
    m = mutation if mutation in ("drop_last_ktile", "ktile_twice") else None
    key = (inp["sh"], inp.get("M_full"), inp["kind"], var.get("split", 1), m)
    if key not in _ACC:
        _ACC[key] = G.accumulate32(inp, var, m)
    return _ACC[key]


def _calls(cell):
    row, epi = G.ROWS[cell[0]], cell[1]
    for sh in row.shapes:
        for var in G.variants(row, epi, sh):
            yield row, epi, sh, G.with_bias(row, epi, var)


def _dbl(out):
    return {k: v.double() for k, v in out.items()}


@pytest.mark.parametrize("fn", [G._f_gelu, G._f_silu, G._f_qgelu, G._f_erf], ids=["gelu", "silu", "qgelu", "erf"])
def test_derivative_bounds(fn):
    """F2 >= sup|f''| and F3 >= sup|f'''| (the chain terms' interval bounds), sampled at 2e-4 over [-12, 12]: beyond it every
    derivative is below 1e-20."""
    x = torch.arange(-12.0, 12.0, 2e-4, dtype=torch.float64)
    d2 = G._d2(fn, x)
    d3 = (G._d2(fn, x + 1e-4) - G._d2(fn, x - 1e-4)) / 2e-4
    print(f"[{fn.__name__}] sup|f''| = {float(d2.abs().max()):.4f}, sup|f'''| = {float(d3.abs().max()):.4f}")
    assert d2.abs().max() <= 0.9 * G.F2 and d3.abs().max() <= 0.9 * G.F3


@pytest.mark.parametrize("kind", G.KINDS16)
@pytest.mark.parametrize("cell", G.CELLS, ids=G.cell_id)
def test_restatement_stays_inside(cell, kind):
    for row, epi, sh, var in _calls(cell):
        inp = _inputs(sh, kind)
        got = _dbl(G.restatement(inp, row, epi, var, acc=_acc(inp, var)))
        rat = G.ratios(got, G.reference(inp, epi, var, got))
        print(f"[{G.cell_id(cell)} {kind} {tuple(sh[:3])} {var}] " + ", ".join(f"{k} {v[0]:.3f}" for k, v in rat.items()))
        for k, (r, i) in rat.items():
            assert r <= 0.6, (k, r, i, tuple(sh[:3]), var)


# (mutation, kernel, layout, epilogue) at which an applicable mutation changes nothing, each with its reason.  Empty: every shape set
# of the table has a shape at which each applicable mutation moves an output (the table is built that way: M > one row tile
# for the gate rows, a zero row of A for the polynomial coefficients, a prior value for the accumulating calls).
NO_OP = {}

_PAIRS = [(m, c) for c in G.CELLS for m in G.MUTATIONS
          if any(G.mutation_applies(m, r, e, sh, v) for r, e, sh, v in _calls(c))
          and (m, G.ROWS[c[0]].kernel, G.ROWS[c[0]].layout, c[1]) not in NO_OP]


@pytest.mark.parametrize("kind", G.KINDS16)
@pytest.mark.parametrize("mutation,cell", _PAIRS, ids=[f"{m}-{G.cell_id(c)}" for m, c in _PAIRS])
def test_mutation_leaves_the_budget(mutation, cell, kind):
    best = 0.0
    for row, epi, sh, var in _calls(cell):
        if not G.mutation_applies(mutation, row, epi, sh, var):
            continue
        inp = _inputs(sh, kind)
        got = _dbl(G.restatement(inp, row, epi, var, mutation, acc=_acc(inp, var, mutation)))
        rat = G.ratios(got, G.reference(inp, epi, var, got))
        r = max(v[0] for v in rat.values())
        print(f"[{mutation} {G.cell_id(cell)} {kind} {tuple(sh[:3])} {var}] " + ", ".join(f"{k} {v[0]:.1f}" for k, v in rat.items()))
        best = max(best, r)
    assert best > 20, (mutation, G.cell_id(cell), kind, best)


# ----------------------------------------------------------------------------------------------- the table against the planner
def _plan(row, epi, sh, var, kernel=None):
    a = G.plan_args(row, epi, sh, var)
    return ops.gemm_plan(a.pop("lay"), a.pop("epi"), a.pop("M"), a.pop("N"), a.pop("K"), a.pop("split_k"), **a,
                         forced=G.FORCED[kernel or row.kernel], ncu=256 - row.reserve, colsplit=0, use288=0)


@pytest.mark.parametrize("cell", G.CELLS, ids=G.cell_id)
def test_each_cell_names_its_kernel(cell):
    for row, epi, sh, var in _calls(cell):
        rc, launches = _plan(row, epi, sh, var)
        assert rc == 0 and [l["kernel"] for l in launches] == [row.kernel], (tuple(sh[:3]), var, rc, launches)
        l = launches[0]
        assert (l["row0"], l["rows"], l["col0"], l["cols"]) == (0, sh.M, 0, sh.N)
        assert l["splits"] == G.eff_splits(sh.K, var.get("split", 1))[0]
        if row.kernel == "256wp":
            assert l["grid"] == 256 - row.reserve
        if row.reserve:                              # the walk: workgroups with two tiles and workgroups with one fewer
            tiles = -(-sh.M // 256) * -(-sh.N // 256)
            assert l["grid"] < tiles < 2 * l["grid"] and -(-tiles // 8) > l["grid"] // 8, (tiles, l["grid"])


def test_leading_dimensions_all_differ():
    for row in G.ROWS:
        for epi in row.epis:
            for sh in row.shapes:
                ld = G.lds(row.layout, epi, sh)
                assert len(set(ld.values())) == len(ld) and all(v % 8 == 0 for v in ld.values())
                assert ld["ldc"] > G.ncols(epi, sh.N) and min(ld["ldc2"], ld["ldr"], ld["ldgate"]) > sh.N


def test_table_is_what_the_planner_can_launch():
    """Every kernel x layout x epilogue: the dry run names the kernel (forced to it, at the kernel's first shape of that layout;
    for a layout the table does not have, at every first shape of the kernel and at one that every kernel's eligibility takes) iff
    the table has the cell."""
    table = G.table_cells()
    universal = G.S(256, 1152, 256, "N % 128, 144, 288, 64 and 72 == 0; an even number of K-tiles >= 4; M % 128 == 0")
    seen = set()
    for kernel in G.KERNELS:
        rows = [r for r in G.ROWS if r.kernel == kernel]
        for lay in G.LAYOUTS:
            mine = [r for r in rows if r.layout == lay]
            shapes = [mine[0].shapes[0]] if mine else [r.shapes[0] for r in rows] + [universal]
            probe = (mine or rows)[0]._replace(layout=lay, reserve=0)
            for epi in range(18):
                named = False
                for sh in shapes:
                    vs = [dict(rpg=64)] if epi == G.GATE_RES else [dict(hd=64), dict(hd=72)] if epi == G.BF16_DOT else [dict()]
                    for var in vs:
                        rc, launches = _plan(probe, epi, sh, var, kernel)
                        named |= rc == 0 and any(l["kernel"] == kernel for l in launches)
                assert named == ((kernel, lay, epi) in table), (kernel, G.LAY_NAME[lay], G.EPI_NAME[epi], named)
                seen.add((kernel, lay, epi))
    assert table <= seen
    print(f"{len(table)} cells (kernel, layout, epilogue); {len(G.CELLS)} with the reserve rows; "
          f"{sum(len(list(_calls(c))) for c in G.CELLS)} calls per build")
