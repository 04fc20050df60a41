"""Every 16-bit GEMM kernel x layout x epilogue against fp64, in the bf16 and the IEEE-half build: the cells of tests/gemm_ref.py
(the table, the references and the budgets; proven on the CPU and held to the planner in tests/test_gemm_budgets_cpu.py).

Each case first asks the planner, with the process's own knobs, which kernel the call will run, and fails unless it is the cell's
(a forced tile is a request: what a kernel does not take falls to the heuristic, and a test that did not look would pass on the
128^2 kernel).  Then it launches under ops.forced_tile with every leading dimension different, every buffer NaN outside its live
elements (inputs too), holds every guard row, guard column and inter-row gap to NaN and every live element to finite, and compares
EVERY element of every output (C, C2, dbias, the head dots summed over their slots, the slabs after reduce_slabs) with the fp64
reference: worst error / budget <= 1, printed with its index.  profiles/gemm_epilogue_tests.txt records the measured ratios.
"""
import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

_INP = {}
CASES = [(c, kind) for i in range(len(G.ROWS)) for kind in G.KINDS16 for c in G.CELLS if c[0] == i]   # a row's shapes stay cached


def _inputs(sh, kind):
    """One shape's inputs and fp64 products: computed once, shared by the row's epilogues, never modified (the last eight kept)."""
    key = (sh, kind)
    if key not in _INP:
        while len(_INP) >= 8:
            _INP.pop(next(iter(_INP)))
        _INP[key] = G.inputs(sh, kind)
    return _INP[key]


def _guarded(buf, rows, cols, what):
    """The live [rows, cols] corner of a 2-D buffer (fp64, CPU) after checking: finite inside, NaN everywhere else."""
    buf = buf.cpu()
    live = buf[:rows, :cols]
    assert torch.isfinite(live).all(), f"{what}: a live element is not finite (never written, or NaN read from a gap)"
    mask = torch.ones(buf.shape, dtype=torch.bool)
    mask[:rows, :cols] = False
    assert torch.isnan(buf[mask]).all(), f"{what}: written outside the live elements (guard rows, guard columns or a gap)"
    return live.double()


def _guarded1(buf, n, what):
    buf = buf.cpu()
    assert torch.isfinite(buf[:n]).all(), f"{what}: a live element is not finite"
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    return buf[:n].double()


def _launch(inp, row, epi, var, dev):
    """One reed_gemm call (and the slab reduce) -> the logical outputs, guards checked."""
    from reed_amd import ops
    M, N, K = inp["sh"][:3]
    bufs, kw, live = G.call_buffers(inp, row, epi, var)
    d = {k: v.to(dev) for k, v in bufs.items()}
    ldc, slab = kw["ldc"], "ws" in d
    dbias = d.get("dbias")
    if slab and var.get("dbias"):
        dbias = d["ws"].data_ptr() + 4 * M * ldc
    ops.gemm(row.layout, epi, d["P"], d["Q"], M, N, K, d["ws"] if slab else d.get("C"), kw.pop("ldp"), kw.pop("ldq"), kw.pop("ldc"),
             C2=d.get("C2"), R=d.get("R"), bias=d.get("bias"), gate=d.get("gate"), dbias=dbias, **kw)
    got = {}
    if slab:
        ns, stride = G.eff_splits(K, var["split"])[0], kw["slab_stride"]
        ops.reduce_slabs(d["ws"], stride, ns, d["C"], M * ldc + M)
        torch.cuda.synchronize()
        for z in range(ns + 1):                       # every slab, then the reduced one: the same layout
            flat = d["C"] if z == ns else d["ws"][z * stride:(z + 1) * stride]
            what = "reduced slabs" if z == ns else f"slab {z}"
            c = _guarded(flat[:M * ldc].view(M, ldc), M, N, what)
            db = _guarded1(flat[M * ldc:], M if var.get("dbias") else 0, what + " bias slice")
        got["C"] = c
        if var.get("dbias"):
            got["dbias"] = db
        return got
    torch.cuda.synchronize()
    for name, lv in live.items():
        if isinstance(lv, tuple):
            got[name] = _guarded(d[name], lv[0], lv[1], name)
        else:
            got[name] = _guarded1(d[name], lv, name)
    if epi == G.BF16_DOT:
        hd = var["hd"]
        got["dsum"] = got.pop("C2").view(N // hd, 1 if hd == 64 else 2, M).sum(1)
    for name in ("P", "Q", "R", "bias", "gate"):      # the inputs are as they were
        if name in d:
            assert torch.equal(torch.nan_to_num(d[name].cpu().float(), nan=12345.0), torch.nan_to_num(bufs[name].float(), nan=12345.0)), name
    return got


@pytest.mark.parametrize("cell,kind", CASES, ids=[f"{G.cell_id(c)}-{k}" for c, k in CASES])
def test_cell(dev, cell, kind):
    from reed_amd import ops
    row, epi = G.ROWS[cell[0]], cell[1]
    prev_kind, prev_reserve = ops.use(kind), ops.cu_reserve()
    worst = {}
    try:
        ops.set_cu_reserve(row.reserve)
        with ops.forced_tile(row.forced):
            for sh in row.shapes:
                inp = _inputs(sh, kind)
                for v in G.variants(row, epi, sh):
                    var = G.with_bias(row, epi, v)
                    a = G.plan_args(row, epi, sh, var)
                    rc, launches = ops.gemm_plan(a.pop("lay"), a.pop("epi"), a.pop("M"), a.pop("N"), a.pop("K"), a.pop("split_k"), **a,
                                                 forced=ops.gemm_forced_tile(), ncu=0, precision=kind)
                    assert rc == 0 and [l["kernel"] for l in launches] == [row.kernel], (tuple(sh[:3]), v, rc, launches)
                    got = _launch(inp, row, epi, var, dev)
                    rat = G.ratios(got, G.reference(inp, epi, var, got))
                    print(f"[{G.cell_id(cell)} {kind} {tuple(sh[:3])} {v}] worst error / budget: "
                          + ", ".join(f"{k} {r:.3f} at {i}" for k, (r, i) in rat.items()))
                    for k, (r, i) in rat.items():
                        assert r <= 1, (k, r, i, tuple(sh[:3]), v)
                        worst[k] = max(worst.get(k, 0.0), r)
    finally:
        ops.set_cu_reserve(prev_reserve)
        ops.use(prev_kind)
    print(f"[cell {G.cell_id(cell)} {kind}] " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
