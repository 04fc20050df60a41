"""The loss kernels of csrc/loss.hip against fp64: interpolant (both paths), sample_posterior, mse_fwd / mse_bwd, cosine_fwd (rowdot
and loss) / cosine_bwd, in all three builds.  tests/adaln_ref.py holds the references and the budgets (proven on the CPU in
tests/test_adaln_budgets_cpu.py); NaN pre-fill, canary bands, two runs bit-equal as in tests/test_reductions_gpu.py.

(B, per) = (1, 1): one live thread; (5, 255): less than one lap of a block; (5, 4096): whole laps; (2, 4097): a per % 256 tail.
(B, T, Z) = (5, 1, 4): one lane live, T = 1, a last block of one row; (3, 7, 260): the Z tail past 256 and a partly filled last
4-row block; (2, 16, 768): whole laps; (1, 300, 1024): the T > 256 stride loop of cosine_sample_kernel.
"""
import pytest
import torch

from tests import adaln_ref as A
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=KINDS)
def build(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def inside(tag, got, ref, budget):
    """Worst |got - ref| / budget over the elements (fp64 CPU reference), returned; outside, the element is named."""
    got = got.double().cpu().flatten()
    ref, budget = ref.flatten(), budget.flatten()
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / budget, torch.full_like(err, float("inf")))
    ratio = torch.where((err == 0) & (budget == 0), torch.zeros_like(ratio), ratio)
    i = int(torch.argmax(ratio))
    r = float(ratio[i])
    assert r <= 1.0, (f"{tag}: element {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, budget {float(budget[i]):.3e}, "
                      f"ratio {r:.3g}")
    return r


def twice(fn):
    """Run fn() -> tuple of Guarded twice: canaries intact, the same bits both times.  Returns the first run's outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.intact() and y.intact(), "written past the end of an output"
        assert torch.equal(bits(x.full), bits(y.full)), "two runs differ"
    return a


@pytest.mark.parametrize("B,per", A.MSE_SHAPES)
def test_interpolant_posterior_mse(dev, build, B, per):
    from reed_amd import ops
    kind = build
    inp = A.mse_inputs(B, per)
    ref = A.mse_reference(inp)
    d = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    r = {}
    for pt, t in ((0, d["t"]), (1, d["t"]), (2, d["t1"])):       # t holds t = 0 and t = 1; 2: the cosine path at t = 1 everywhere
        def interp():
            xt, tg = Guarded(B * per, F32, dev), Guarded(B * per, F32, dev)
            ops.interpolant(d["x"], d["n"], t, xt.t, tg.t, B, per, min(pt, 1))
            return xt, tg

        xt, tg = twice(interp)
        r[f"xt{pt}"] = inside(f"interpolant {kind} {(B, per)} path {pt} xt", xt.t, ref[f"xt{pt}"], ref[f"b_xt{pt}"])
        r[f"tg{pt}"] = inside(f"interpolant {kind} {(B, per)} path {pt} target", tg.t, ref[f"tg{pt}"], ref[f"b_tg{pt}"])

    def post():
        out = Guarded(B * per, F32, dev)
        ops.sample_posterior(d["mom"], d["eps"], out.t, B, per, inp["scale"], inp["bias"])
        return (out,)

    out, = twice(post)
    r["post"] = inside(f"sample_posterior {kind} {(B, per)}", out.t, ref["post"], ref["b_post"])

    def mse():
        loss, dout = Guarded(B, F32, dev), Guarded(B * per, F32, dev)
        ops.mse_fwd(d["x"], d["n"], loss.t, B, per)
        ops.mse_bwd(d["x"], d["n"], d["gs"], dout.t, B, per)
        return loss, dout

    loss, dout = twice(mse)
    r["mse"] = inside(f"mse_fwd {kind} {(B, per)}", loss.t, ref["mse"], ref["b_mse"])
    r["dout"] = inside(f"mse_bwd {kind} {(B, per)}", dout.t, ref["dout"], ref["b_dout"])
    assert set(r) == set(A.MSE_OUTPUTS)
    print(f"[interpolant / posterior / mse {kind} {(B, per)}] worst error / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


@pytest.mark.parametrize("B,T,Z", A.COS_SHAPES)
def test_cosine_fwd_bwd(dev, build, B, T, Z):
    """One all-zero zt row and one all-zero z row: the 1e-12 clamps decide there (rowdot is exactly 0; the gradient of the zero zt
    row is O(1 / eps), compared relatively, and must be the infinity of its sign where it overflows fp16)."""
    from reed_amd import ops
    kind, dt, M = build, DTYPE[build], B * T
    inp = A.cos_inputs(B, T, Z, kind)
    ref = A.cos_reference(inp)
    zt, z, gs = inp["zt"].to(dev), inp["z"].to(dev), inp["gs"].to(dev)

    def run():
        rowdot, loss, dzt = Guarded(M, F32, dev), Guarded(B, F32, dev), Guarded(M * Z, dt, dev)
        ops.cosine_fwd(zt, z, rowdot.t, loss.t, B, T, Z)
        ops.cosine_bwd(zt, z, gs, dzt.t, B, T, Z)
        return rowdot, loss, dzt

    rowdot, loss, dzt = twice(run)
    got = dict(rowdot=rowdot.t, loss=loss.t, dzt=dzt.t.view(M, Z))
    ratios = A.cos_ratios(got, ref, inp)
    print(f"[cosine {kind} {(B, T, Z)}] worst error / budget: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in ratios.items()))
    for k, (r, i) in ratios.items():
        assert r <= 1.0, (k, r, i, float(got[k].flatten()[i]), float(ref[k].flatten()[i]), float(ref["b_" + k].flatten()[i]))
    # the clamp rows on their own: a zero row has a cosine of exactly 0; the zero z row has a gradient of exactly 0; the zero zt
    # row's gradient is gscale / T / 1e-12 * zhat, within the type's rounding of it (relative: the values are of order 1e10)
    for row in (inp["zero_zt"], inp["zero_z"]):
        assert float(rowdot.t[row]) == 0.0
    assert (dzt.t.view(M, Z)[inp["zero_z"]] == 0).all()
    g = dzt.t.view(M, Z)[inp["zero_zt"]].double().cpu()
    want, budget = ref["dzt"][inp["zero_zt"]], ref["b_dzt"][inp["zero_zt"]]
    assert float(want.abs().max()) > 1e8
    fin = torch.isfinite(A.rnd(want, kind)) & (want != 0)
    if fin.any():
        rel, rel_b = ((g - want).abs() / want.abs())[fin], (budget / want.abs())[fin]
        print(f"[cosine {kind} {(B, T, Z)}] clamped zt row: worst relative error {float(rel.max()):.3e}, relative budget there "
              f"{float(rel_b[rel.argmax()]):.3e}")
        assert (rel <= rel_b).all()
    else:
        assert torch.equal(g, A.rnd(want, kind))                  # every element overflows the type: the infinities of its signs


def test_loss_entry_points_refuse_empty_shapes(dev, build):
    from reed_amd import ops
    dt = DTYPE[build]
    a, b = torch.ones(64, device=dev), torch.ones(64, device=dev)
    zt = torch.ones(64, dtype=dt, device=dev)
    o1, o2, o3 = Guarded(64, F32, dev, fill=7.0), Guarded(64, F32, dev, fill=7.0), Guarded(64, dt, dev, fill=7.0)
    for B, per in ((0, 8), (2, 0), (-1, 8), (2, -8)):
        with pytest.raises(RuntimeError, match="interpolant"):
            ops.interpolant(a, b, a, o1.t, o2.t, B, per, 0)
        with pytest.raises(RuntimeError, match="sample_posterior"):
            ops.sample_posterior(a, b, o1.t, B, per, 1.0, 0.0)
        with pytest.raises(RuntimeError, match="mse_fwd"):
            ops.mse_fwd(a, b, o1.t, B, per)
        with pytest.raises(RuntimeError, match="mse_bwd"):
            ops.mse_bwd(a, b, a, o2.t, B, per)
    for B, T, Z in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-2, 2, 4), (2, -2, 4), (2, 2, -4)):
        with pytest.raises(RuntimeError, match="cosine_fwd"):
            ops.cosine_fwd(zt, a, o1.t, o2.t, B, T, Z)
        with pytest.raises(RuntimeError, match="cosine_bwd"):
            ops.cosine_bwd(zt, a, b, o3.t, B, T, Z)
    torch.cuda.synchronize()
    for o in (o1, o2, o3):                                      # nothing was launched
        assert o.intact() and (o.t == 7.0).all()
