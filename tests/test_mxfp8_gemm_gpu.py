"""csrc/gemm_mxfp8.hip on the GPU, in the bf16 and the IEEE-half build: the quantiser bit for bit against tests/mxfp8_ref.py, the
scaled MFMA's lane map and scale operands on exact-integer data, and the products of all three epilogues against the fp64
reference within that module's budgets (proven on the CPU in tests/test_mxfp8_budgets_cpu.py).  Every buffer has its own leading
dimension and is poisoned outside its live elements (NaN; code 0x7F / scale byte 0xFF in the operand arrays, which decode to NaN)."""
import pytest
import torch

from tests import gemm_ref as G
from tests import mxfp8_ref as R

pytestmark = pytest.mark.gpu

KINDS = G.KINDS16
_INP = {}


def _inputs(sh, kind):
    key = (sh, kind)
    if key not in _INP:
        while len(_INP) >= 4:
            _INP.pop(next(iter(_INP)))
        _INP[key] = R.inputs(sh, kind)
    return _INP[key]


def _u8buf(vals, ld, fill, guard=G.GUARD):
    b = torch.full((vals.shape[0] + guard, ld), fill, dtype=torch.uint8)
    b[:vals.shape[0], :vals.shape[1]] = vals
    return b


# ------------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", (128, 384, 1152))
@pytest.mark.parametrize("Rr", (1, 17, 300))
def test_quantiser_matches_the_reference_bit_for_bit(dev, kind, K, Rr):
    from reed_amd import ops
    dt = G.DTYPE[kind]
    g = torch.Generator().manual_seed(9 + Rr + K)
    x = (torch.randn(Rr, K, generator=g, dtype=torch.float64) * torch.exp(2.0 * torch.randn(Rr, 1, generator=g, dtype=torch.float64))).to(dt)
    edge = R.edge_rows(K, kind)
    n = min(Rr, edge.shape[0])
    x[:n] = edge[:n]
    ldx, ldq, lds = K + 8, K + 16, K // 32 + 3
    xb = torch.full((Rr + G.GUARD, ldx), float("nan"), dtype=dt)
    xb[:Rr, :K] = x
    q0, s0 = _u8buf(torch.zeros(0, K, dtype=torch.uint8), ldq, 0xA5, Rr + G.GUARD), _u8buf(torch.zeros(0, K // 32, dtype=torch.uint8), lds, 0x5A, Rr + G.GUARD)
    xd, qd, sd = xb.to(dev), q0.to(dev), s0.to(dev)
    prev = ops.use(kind)
    try:
        ops.mx_quantize(xd, qd, sd, Rr, K, ldx=ldx, ldq=ldq, lds=lds)
    finally:
        ops.use(prev)
    torch.cuda.synchronize()
    qref, sref = R.quantize(x)
    want_q, want_s = q0.clone(), s0.clone()
    want_q[:Rr, :K], want_s[:Rr, :K // 32] = qref, sref
    got_q, got_s = qd.cpu(), sd.cpu()
    bad = (got_q != want_q).nonzero()
    assert torch.equal(got_s, want_s), ("scale bytes (or a gap)", (got_s != want_s).nonzero()[:8].tolist())
    assert torch.equal(got_q, want_q), ("codes (or a gap)", bad[:8].tolist(), [(int(got_q[i, j]), int(want_q[i, j])) for i, j in bad[:8].tolist()])


# ---------------------------------------------------------------------------------------------------------- lane-map probe
def _probe_operands(M=40, N=256, K=256):
    """Exact small integers, mostly zeros, asymmetric in m, n and k; block scales 2^0..2^1 (A) and 2^-1..2^1 (W), distinct per
    (row, block) pattern: every product sum is a multiple of 1/2 below 128 — exact in bf16 and fp16 (asserted by the test)."""
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    A = torch.where((7 * k + 3 * m) % 11 == 0, ((m + k) % 2 + 1) * (1 - 2 * ((m + k // 3) % 2)), torch.zeros((), dtype=torch.int64)).double()
    W = torch.where((5 * k + n) % 13 == 0, ((n + 2 * k) % 3 + 1) * (1 - 2 * ((n // 2 + k) % 2)), torch.zeros((), dtype=torch.int64)).double()
    jb = torch.arange(K // 32)[None, :]
    As = (127 + (m + jb) % 2).to(torch.uint8)
    Ws = (127 + (n + 2 * jb) % 3 - 1).to(torch.uint8)
    return R.e4m3_codes(A), As, R.e4m3_codes(W), Ws


@pytest.mark.parametrize("kind", KINDS)
def test_lane_map_and_scale_operands_on_exact_integers(dev, kind):
    from reed_amd import ops
    M, N, K = 40, 256, 256
    Aq, As, Wq, Ws = _probe_operands(M, N, K)
    ref = R.decode(Aq, As) @ R.decode(Wq, Ws).T
    dt = G.DTYPE[kind]
    assert torch.equal(ref.to(dt).double(), ref) and int((ref != 0).sum()) > M * N // 4 and not torch.equal(ref[:, :M], ref[:, :M].T)
    C = torch.full((M + G.GUARD, N + 8), float("nan"), dtype=dt, device=dev)
    prev = ops.use(kind)
    try:
        ops.gemm_mxfp8(ops.EPI_BF16, Aq.to(dev), As.to(dev), Wq.to(dev), Ws.to(dev), M, N, K, C, N + 8)
    finally:
        ops.use(prev)
    torch.cuda.synchronize()
    got = C.cpu()
    assert torch.isnan(got[M:]).all() and torch.isnan(got[:, N:]).all()
    bad = (got[:M, :N].double() != ref).nonzero()
    assert len(bad) == 0, (len(bad), [(i, j, float(got[i, j]), float(ref[i, j])) for i, j in bad[:12].tolist()])


# ------------------------------------------------------------------------------------------------------------- products
def _launch(inp, epi, var, dev):
    from reed_amd import ops
    M, N, K = inp["sh"][:3]
    bufs, kw, live = G.call_buffers(inp, G.ROWS[0], epi, var)
    lda, ldw, ldas, ldws = K + 16, K + 32, K // 32 + 4, K // 32 + 8
    ob = dict(Aq=_u8buf(inp["Aq"], lda, 0x7F), As=_u8buf(inp["As"], ldas, 0xFF), Wq=_u8buf(inp["Wq"], ldw, 0x7F), Ws=_u8buf(inp["Ws"], ldws, 0xFF))
    d = {k: v.to(dev) for k, v in list(bufs.items()) + list(ob.items()) if k not in ("P", "Q")}
    ops.gemm_mxfp8(epi, d["Aq"], d["As"], d["Wq"], d["Ws"], M, N, K, d.get("C"), kw["ldc"], lda=lda, ldas=ldas, ldw=ldw, ldws=ldws,
                   C2=d.get("C2"), ldc2=kw.get("ldc2", 0), R=d.get("R"), ldr=kw.get("ldr", 0), bias=d.get("bias"), gate=d.get("gate"),
                   ldgate=kw.get("ldgate", 0), rows_per_gate=kw.get("rows_per_gate", 1))
    torch.cuda.synchronize()
    got = {}
    for name, (rows, cols) in live.items():
        buf = d[name].cpu()
        lv = buf[:rows, :cols]
        assert torch.isfinite(lv).all(), f"{name}: a live element is not finite (never written, or a poisoned gap was read)"
        mask = torch.ones(buf.shape, dtype=torch.bool)
        mask[:rows, :cols] = False
        assert torch.isnan(buf[mask]).all(), f"{name}: written outside the live elements"
        got[name] = lv.double()
    for name in ob:
        assert torch.equal(d[name].cpu(), ob[name]), name
    return got


CASES = [(sh, kind, epi) for sh in R.SHAPES for kind in KINDS for epi in R.EPIS]


@pytest.mark.parametrize("sh,kind,epi", CASES, ids=[f"{s.M}x{s.N}x{s.K}-{k}-{G.EPI_NAME[e]}" for s, k, e in CASES])
def test_products_within_the_fp64_budget(dev, sh, kind, epi):
    from reed_amd import ops
    assert ops.gemm_mxfp8_plan(epi, sh.M, sh.N, sh.K, precision=kind)
    inp = _inputs(sh, kind)
    prev = ops.use(kind)
    try:
        for var in R.variants(epi):
            got = _launch(inp, epi, var, dev)
            rat = G.ratios(got, R.reference(inp, epi, var, got))
            print(f"[mxfp8 {G.EPI_NAME[epi]} {kind} {tuple(sh[:3])} {var}] worst error / budget: "
                  + ", ".join(f"{k} {r:.3f} at {i}" for k, (r, i) in rat.items()))
            for k, (r, i) in rat.items():
                assert r <= 1, (k, r, i, tuple(sh[:3]), var)
    finally:
        ops.use(prev)


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_block_poisons_exactly_its_rows(dev, kind):
    """An inf in one activation row: scale byte 0xFF from the quantiser, and that output row — no other — comes out NaN."""
    from reed_amd import ops
    sh = R.SHAPES[1]
    inp = _inputs(sh, kind)
    M, N, K = sh[:3]
    x = inp["A16"].clone()
    x[5, 40] = float("inf")
    dt = G.DTYPE[kind]
    xd = x.to(dev)
    q, s = torch.empty(M, K, dtype=torch.uint8, device=dev), torch.empty(M, K // 32, dtype=torch.uint8, device=dev)
    C = torch.zeros(M, N, dtype=dt, device=dev)
    prev = ops.use(kind)
    try:
        ops.mx_quantize(xd, q, s, M, K)
        ops.gemm_mxfp8(ops.EPI_BF16, q, s, inp["Wq"].to(dev), inp["Ws"].to(dev), M, N, K, C, N)
    finally:
        ops.use(prev)
    torch.cuda.synchronize()
    assert int(s.cpu()[5, 1]) == 0xFF
    nan_rows = torch.isnan(C.cpu().float()).all(1)
    fin_rows = torch.isfinite(C.cpu().float()).all(1)
    assert bool(nan_rows[5]) and int(nan_rows.sum()) == 1 and int(fin_rows.sum()) == M - 1
