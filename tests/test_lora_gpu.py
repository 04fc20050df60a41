"""reed_lora_grads and reed_lora_merge (csrc/lora.hip) against fp64 in all three builds, to the budgets of tests/lora_ref.py (proven on
the CPU in tests/test_lora_budgets_cpu.py).  Every input sits in a buffer that is NaN behind its live elements (a MFMA row or
column loaded from a gap poisons the outputs), the outputs and the workspace are NaN before the call with a canary band behind,
every call runs twice and must give the same bits.  profiles/lora_tests.txt records the measured ratios.

reed_lora_grads shapes (tests/lora_ref.py: SHAPES): M = 16 (less than one 16-row MFMA tile group of the last wave), 63 (one
64-row slab of the u / v pass minus 1), 64, 144 (two slabs plus 16: a ragged last 32-row step of the partial-sum pass too);
(N, K) = (128, 128), (384, 128), (128, 512); R = 8 (padded to the 16-wide tile), 16, 64 (four tiles); and one tall case past 32
steps of 32 rows, where a slab of the partial-sum pass holds two steps and the last slab is ragged."""
import pytest
import torch

from tests import lora_ref as lr
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=KINDS)
def build(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def _behind_nan(t, dev):
    """t on the device with 256 NaN elements behind it."""
    full = torch.full((t.numel() + 256,), float("nan"), dtype=t.dtype, device=dev)
    full[:t.numel()] = t.flatten().to(dev)
    return full


def _run_grads(inp, accumulate, dev):
    from reed_amd import ops
    M, N, K, R = inp["M"], inp["N"], inp["K"], inp["R"]
    x, dy, a, b = (_behind_nan(inp[k], dev) for k in ("x", "dy", "a", "b"))
    outs = []
    for _ in range(2):
        ws = Guarded(ops.lora_grads_ws_floats(M, N, K, R), F32, dev)
        da, db = Guarded(R * K, F32, dev), Guarded(N * R, F32, dev)
        if accumulate:
            da.t.copy_(inp["da0"].flatten())
            db.t.copy_(inp["db0"].flatten())
        ops.lora_grads(x, dy, a, b, inp["scale"], da.full, db.full, ws.full, M, N, K, R, accumulate)
        torch.cuda.synchronize()
        assert da.intact() and db.intact() and ws.intact(), "written past the end of an output or of the workspace"
        outs.append((da, db))
    (da, db), (da2, db2) = outs
    assert torch.equal(bits(da.t), bits(da2.t)) and torch.equal(bits(db.t), bits(db2.t)), "two runs differ"
    return dict(da=da.t.view(R, K).cpu(), db=db.t.view(N, R).cpu())


def _check(inp, build, dev, tag):
    for accumulate in (False, True):
        ref = lr.grads_reference(inp, accumulate)
        r = lr.grads_ratio(_run_grads(inp, accumulate, dev), ref)
        print(f"[lora_grads {build} {tag} acc={int(accumulate)}] worst error / budget {r:.3f}")
        assert r <= 1.0, (tag, accumulate, r)


@pytest.mark.parametrize("R", lr.RS)
@pytest.mark.parametrize("N,K", lr.NKS)
def test_lora_grads(dev, build, N, K, R):
    for M in lr.MS:
        _check(lr.grads_inputs(M, N, K, R, build), build, dev, f"M={M} N={N} K={K} R={R}")


def test_lora_grads_tall(dev, build):
    """33.5 steps of 32 rows: slabs of two steps in the 16-bit builds, the last one ragged."""
    M, N, K, R = 32 * 33 + 16, 128, 128, 16
    _check(lr.grads_inputs(M, N, K, R, build), build, dev, f"M={M} N={N} K={K} R={R}")


def test_lora_grads_refuses_out_of_domain(dev, build):
    from reed_amd import ops
    q = 4 if build == "fp32" else 128
    t = torch.zeros(4096, dtype=DTYPE[build], device=dev)
    f = torch.zeros(4096, dtype=F32, device=dev)
    for (M, N, K, R) in ((16, 128, 128, 12), (16, 128 + q // 2, 128, 8), (16, 128, 128 + q // 2, 8), (0, 128, 128, 8)):
        with pytest.raises(ValueError):
            ops.lora_grads_ws_floats(M, N, K, R)
        with pytest.raises(RuntimeError, match="lora_grads"):
            ops.lora_grads(t, t, t, t, 1.0, f, f, f, M, N, K, R)
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0.0


@pytest.mark.parametrize("N,K,R", lr.MERGE_SHAPES)
def test_lora_merge(dev, build, N, K, R):
    from reed_amd import ops
    inp = lr.merge_inputs(N, K, R)
    w, a, b = (_behind_nan(inp[k], dev) for k in ("w", "a", "b"))
    dt = DTYPE[build]

    def run(bb, both=True):
        w32, wop = Guarded(N * K, F32, dev), Guarded(N * K, dt, dev)
        ops.lora_merge(w, a, bb, inp["scale"], wop.full, w32.full if both else None, N, K, R)
        torch.cuda.synchronize()
        assert w32.intact() and wop.intact()
        return w32.t.view(N, K), wop.t.view(N, K)

    w32, wop = run(b)
    ref, budget = lr.merge_reference(inp)
    r = lr.worst((w32.cpu().double() - ref).abs(), budget)[0]
    print(f"[lora_merge {build} N={N} K={K} R={R}] w32 worst error / budget {r:.3f}")
    assert r <= 1.0
    assert torch.equal(bits(wop), bits(w32.to(dt))), "w_op is not the cast of w32"
    assert torch.equal(bits(run(b, both=False)[1]), bits(wop)), "w_op alone differs"
    # B = 0: r(w) bit for bit (and w itself in fp32), negative zeros included
    w0 = inp["w"].clone()
    w0[0, :4] = -0.0
    w = _behind_nan(w0, dev)
    z32, zop = run(torch.zeros(N * R + 256, dtype=F32, device=dev))
    assert torch.equal(bits(z32), bits(w0.to(dev))) and torch.equal(bits(zop), bits(w0.to(dev).to(dt)))
