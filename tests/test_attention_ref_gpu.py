"""Every 16-bit attention kernel and dispatch path against fp64, in the bf16 and the IEEE-half build: the cells of
tests/attention_ref.py (the table, the reference and the budgets; proven on the CPU in tests/test_attention_budgets_cpu.py).

For every (cell, T) x build x flavour: one call of the entry point with every buffer a slice of a larger NaN allocation (inputs
too: a row read from a guard poisons exactly the outputs that must not depend on it) and the outputs NaN-filled; then every guard
element still NaN (for the workspace: behind ops.attention_bwd_ws_floats), every live output element finite, the inputs as they
were, and EVERY element of every output inside its budget: worst error / budget <= 1, printed with the index decoded to
(b, h, t, d).  T = 1 adds exact assertions.  profiles/attn_ref_tests.txt records the measured ratios.
"""
import pytest
import torch

from tests import attention_ref as A

pytestmark = pytest.mark.gpu

CASES = [(c, kind) for c in A.CASES for kind in A.KINDS16]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run(inp, dev):
    """One call of the case's entry point -> the logical outputs (CPU), guards, finiteness and untouched inputs checked."""
    from reed_amd import ops
    cell, B, T, H, hd = inp["cell"], inp["B"], inp["T"], inp["H"], inp["hd"]
    bufs = A.buffers(inp, dev)
    before = {k: b.full.clone() for k, b in bufs.items() if k not in A.OUTPUTS[cell.entry]}
    v = {k: b.live for k, b in bufs.items()}
    if cell.entry == "fwd":
        ops.attention_fwd(v["qkv"], v["o"], v["lse"], B, T, H, hd)
    else:
        ws = None
        if cell.entry != "bwd":
            nws = ops.attention_bwd_ws_floats(B, T, H)
            assert nws == A.ws_floats(B, T, H)
            ws = A.Band((nws,), torch.float32, None, dev)
        if cell.entry == "bwd_dp":
            ops.attention_bwd_dp(v["qkv"], v["do"], v["lse"], v["dpart"], v["dqkv"], ws.live, B, T, H, hd)
        else:
            ops.attention_bwd(v["qkv"], v["o"], v["do"], v["lse"], v["dqkv"], B, T, H, hd, ws=None if ws is None else ws.live)
        if ws is not None:
            torch.cuda.synchronize()
            ws.check("ws", finite=False)                # a scratch buffer (sized for hd 72): its guards only
    torch.cuda.synchronize()
    got = A.collect(inp, bufs)
    for k, t in before.items():
        assert torch.equal(_bits(bufs[k].full), _bits(t)), f"{k}: an input was written"
    return got


@pytest.mark.parametrize("case,kind", CASES, ids=[f"{A.case_id(c)}-{k}" for c, k in CASES])
def test_case(dev, case, kind):
    from reed_amd import ops
    ci, T = case
    cell = A.CELLS[ci]
    prev_kind, prev_reserve, prev_forms = ops.use(kind), ops.cu_reserve(), ops.comm_forms()
    worst = {}
    try:
        ops.set_cu_reserve(cell.reserve)
        if cell.comm:
            ops.set_comm_forms(True)
            ops.set_concurrent_comm(True)
        for fl in A.flavours(cell, kind):
            inp = A.inputs(ci, T, kind, fl)
            got = _run(inp, dev)
            rat = A.ratios(got, A.reference(inp))
            print(f"[{A.case_id(case)} {kind} {fl}] worst error / budget: "
                  + ", ".join(f"{k} {r:.3f} at {A.decode(inp, k, i)}" for k, (r, i) in rat.items()))
            for k, (r, i) in rat.items():
                assert r <= 1, (k, r, A.decode(inp, k, i), fl)
                worst[k] = max(worst.get(k, 0.0), r)
            if T == 1 and cell.entry == "fwd":          # one key: p = 1, l = 1, O is v bit for bit (lse = fp32(s): the budget above)
                assert torch.equal(_bits(got["O"].to(inp["v"].dtype)), _bits(inp["v"])), "T = 1: O is not v bit for bit"
            if T == 1 and cell.entry != "fwd":          # O = v: dP - delta = 0 in exact arithmetic, dQ = dK = 0 up to the tiny budget
                assert torch.equal(inp["O"], inp["v"])
                assert float(A.reference(inp)["dQ"][0].abs().max()) < 1e-9 * float(inp["dO"].double().abs().max())
    finally:
        if cell.comm:
            ops.set_concurrent_comm(False)
            ops.set_comm_forms(prev_forms)
        ops.set_cu_reserve(prev_reserve)
        ops.use(prev_kind)
    print(f"[case {A.case_id(case)} {kind}] " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
