"""The adaLN row kernels of csrc/norm.hip against fp64: LayerNorm+modulate forward (both instantiations, the plain cast), backward
with and without the gate (all seven two-wave widths and the one-wave fallback with masked lanes), gate_bwd, reduce_mod_parts.

Rules for every case (tests/adaln_ref.py; the budgets are proven on the CPU in tests/test_adaln_budgets_cpu.py): the reference is
fp64 from the operand-type inputs, the modulation operands lie in one [B, 6 D + 8] array as the engine lays them out, outputs are
pre-filled with NaN unless accumulating, a canary band follows every output, every case runs twice and must give the same bits,
in all three builds.  The two-wave backward reaches its arrays through buffer descriptors, where an out-of-range offset loads 0
and drops the store without a fault: only the comparison of every value with the reference sees that.
"""
import pytest
import torch

from tests import adaln_ref as A
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits, sum_budget

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


_REF = {}


def _bwd_case(kind, B, T, D, dev):
    """Inputs on the device and the fp64 reference of one backward case: computed once, shared, never modified."""
    key = (kind, B, T, D)
    if key not in _REF:
        inp = A.bwd_inputs(B, T, D, kind)
        _REF[key] = (inp, A.bwd_reference(inp), {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)})
    return _REF[key]


def _mod_ptrs(mod, D):
    """(shift, scale, gate) addresses inside the [B, 6 D + 8] array and its row stride in elements."""
    es = mod.element_size()
    return mod.data_ptr(), mod.data_ptr() + D * es, mod.data_ptr() + 2 * D * es, mod.shape[1]


# ----------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("B,T,D", A.FWD_SHAPES)
def test_ln_modulate_fwd(dev, build, B, T, D):
    """(3, 7, 4): one lane live, M = 21, the last block has one row; 260: a masked second float4; 1280: no lane masked."""
    from reed_amd import ops
    kind, dt, M = build, DTYPE[build], B * T
    inp = A.ln_inputs(B, T, D, kind)
    ref = A.ln_reference(inp)
    x, mod = inp["x"].to(dev), inp["mod"].to(dev)
    shift, scale, _, ld = _mod_ptrs(mod, D)

    def run():
        h, mean, rstd = Guarded(M * D, dt, dev), Guarded(M, F32, dev), Guarded(M, F32, dev)
        ops.ln_modulate_fwd(x, shift, scale, ld, h.t, mean.t, rstd.t, M, D, T)
        return h, mean, rstd

    h, mean, rstd = twice(run)
    r = {k: inside(f"ln_modulate_fwd {kind} {(B, T, D)} {k}", g.t, ref[k], ref["b_" + k])
         for k, g in (("h", h), ("mean", mean), ("rstd", rstd))}
    print(f"[ln_modulate_fwd {kind} {(B, T, D)}] worst error / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))

    def no_stats():          # mean = rstd = NULL: the same h
        h2 = Guarded(M * D, dt, dev)
        ops.ln_modulate_fwd(x, shift, scale, ld, h2.t, None, None, M, D, T)
        return (h2,)

    h2, = twice(no_stats)
    assert torch.equal(bits(h2.t), bits(h.t))

    def cast():              # scale = NULL: the plain cast, bit-exact against torch's
        h3 = Guarded(M * D, dt, dev)
        ops.ln_modulate_fwd(x, None, None, 0, h3.t, None, None, M, D, T)
        return (h3,)

    h3, = twice(cast)
    assert torch.equal(bits(h3.t), bits(ref["cast"].to(dev).flatten()))


def test_ln_modulate_fwd_non_temporal_instantiation(dev, build):
    """ln_mod_fwd_kernel<true> is chosen at M * D * 4 >= 256 MiB: D = 1280, M = 52432 (the first multiple of 16 at or above the
    threshold) in one call, then the same rows in two calls below it: h, mean and rstd bit-identical, and 2048 sampled rows inside
    the budget against fp64."""
    from reed_amd import ops
    kind, dt = build, DTYPE[build]
    D, T, M = 1280, 16, 52432
    B = M // T
    assert M % 16 == 0 and M * D * 4 >= (256 << 20) > (M - 16) * D * 4
    g = torch.Generator(device=dev).manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    x = rn(M, D) * torch.exp(rn(M, 1)) + 2.0 * rn(M, 1)
    mod = (0.5 * rn(B, 6 * D + 8)).to(dt)
    es, ld = mod.element_size(), mod.shape[1]

    def run(splits):
        h, mean, rstd = Guarded(M * D, dt, dev), Guarded(M, F32, dev), Guarded(M, F32, dev)
        for r0, r1 in splits:
            assert r0 % T == 0
            mp = mod.data_ptr() + (r0 // T) * ld * es
            ops.ln_modulate_fwd(x[r0:r1], mp, mp + D * es, ld, h.t[r0 * D:r1 * D], mean.t[r0:r1], rstd.t[r0:r1], r1 - r0, D, T)
        return h, mean, rstd

    one = run([(0, M)])
    half = (M // 2) // T * T
    assert max(half, M - half) * D * 4 < (256 << 20)
    two = run([(0, half), (half, M)])
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        assert a.intact() and b.intact(), "written past the end of an output"
        assert torch.equal(bits(a.full), bits(b.full)), "the two instantiations differ"
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:2048].sort().values
    smp = idx // T
    modc = mod[smp.to(dev)].cpu()
    c = A._ln_core(x[idx.to(dev)].cpu(), A._s1(modc[:, D:2 * D], kind), modc[:, :D].double())
    h, mean, rstd = one
    di = idx.to(dev)
    r = dict(h=inside(f"ln fwd NT {kind} h", h.t.view(M, D)[di], c["H"], A.ulp_out(c["H"], kind) + c["e_h"]),
             mean=inside(f"ln fwd NT {kind} mean", mean.t[di], c["mean"], c["b_mean"]),
             rstd=inside(f"ln fwd NT {kind} rstd", rstd.t[di], c["rstd"], c["b_rstd"]))
    print(f"[ln_modulate_fwd non-temporal {kind} M={M} D={D}] worst error / budget over 2048 rows: "
          + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def test_ln_modulate_fwd_refuses_one_statistic_without_the_other(dev, build):
    from reed_amd import ops
    dt, M, D, T = DTYPE[build], 4, 8, 2
    x = torch.ones(M, D, device=dev)
    mod = torch.zeros(2, 6 * D + 8, dtype=dt, device=dev)
    shift, scale, _, ld = _mod_ptrs(mod, D)
    h, mean, rstd = Guarded(M * D, dt, dev, fill=7.0), Guarded(M, F32, dev, fill=7.0), Guarded(M, F32, dev, fill=7.0)
    for m_, r_ in ((mean.t, None), (None, rstd.t)):
        with pytest.raises(RuntimeError, match="mean and rstd"):
            ops.ln_modulate_fwd(x, shift, scale, ld, h.t, m_, r_, M, D, T)
    torch.cuda.synchronize()
    for o in (h, mean, rstd):                                   # nothing was launched
        assert o.intact() and (o.t == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- backward
def _check_bwd(tag, outs, ref, with_pdy):
    dx, part, dy, pg, pd = outs
    r = {k: inside(f"{tag} {k}", g.t, ref[k], ref["b_" + k]) for k, g in (("dx", dx), ("part", part), ("dy", dy), ("part_g", pg))}
    if with_pdy:
        r["part_dy"] = inside(f"{tag} part_dy", pd.t, ref["part_dy"], ref["b_part_dy"])
    else:
        assert torch.isnan(pd.t).all(), "part_dy = NULL was written"
    return r


@pytest.mark.parametrize("with_pdy", [True, False])
@pytest.mark.parametrize("B,T", [(3, 16), (2, 48)])
@pytest.mark.parametrize("D", A.BWD_WIDTHS)
def test_ln_modulate_bwd_gate_and_two_passes(dev, build, D, B, T, with_pdy):
    """D in {128 .. 1152}: the seven ln_mod_bwd2_kernel instantiations; D in {4, 200, 640, 1280}: the one-wave ln_mod_bwd_kernel
    (4, 200, 640: masked lanes).  (3, 16): every block another sample; (2, 48): three blocks per sample.  The one-pass kernel and
    ln_modulate_bwd followed by gate_bwd each sit inside the same budgets; reduce_mod_parts over the checked part."""
    from reed_amd import ops
    kind, dt, M = build, DTYPE[build], B * T
    inp, ref, d = _bwd_case(kind, B, T, D, dev)
    _, scale, gate, ld = _mod_ptrs(d["mod"], D)
    nc = M // 16

    def outputs():
        dx = Guarded(M * D, F32, dev)
        dx.t.copy_(d["dx0"].flatten())                       # dx accumulates
        return dx, Guarded(nc * 2 * D, F32, dev), Guarded(M * D, dt, dev), Guarded(nc * D, F32, dev), Guarded(nc * D, F32, dev)

    def one_pass():
        dx, part, dy, pg, pd = o = outputs()
        ops.ln_modulate_bwd_gate(d["dh"], d["x"], d["mean"], d["rstd"], scale, ld, dx.t, part.t, d["y"], gate, ld, dy.t, pg.t,
                                 pd.t if with_pdy else None, M, D, T)
        return o

    def two_passes():
        dx, part, dy, pg, pd = o = outputs()
        ops.ln_modulate_bwd(d["dh"], d["x"], d["mean"], d["rstd"], scale, ld, dx.t, part.t, M, D, T)
        ops.gate_bwd(dx.t, d["y"], gate, ld, dy.t, pg.t, M, D, T, part_dy=pd.t if with_pdy else None)
        return o

    form = "two-wave" if D in A.BWD2 else "one-wave"
    res = {}
    for name, fn in (("one pass", one_pass), ("two passes", two_passes)):
        outs = twice(fn)
        res[name] = _check_bwd(f"ln bwd {form} {name} {kind} {(B, T, D)}", outs, ref, with_pdy)
        print(f"[ln bwd {form}, {name}, {kind}, {(B, T, D)}, part_dy={with_pdy}] worst error / budget: "
              + ", ".join(f"{k} {v:.3f}" for k, v in res[name].items()))
    if not with_pdy:
        return
    # reduce_mod_parts over the reference-checked part: dmod[b, 0:D] = sum over the chunks of sum dh, [D:2D] of sum dh xhat
    part = outs[1].t
    chunks = T // 16

    def reduce():
        dmod = Guarded(B * 2 * D, dt, dev)
        ops.reduce_mod_parts([(part.data_ptr(), 2 * D, 0), (part.data_ptr() + 4 * D, 2 * D, D)], dmod.t, 2 * D, B, D, chunks)
        return (dmod,)

    dmod, = twice(reduce)
    want, budget = sum_budget(part.cpu().view(B, chunks, 2 * D), 1, kind)
    r = inside(f"reduce_mod_parts {kind} {(B, T, D)}", dmod.t, want, budget)
    print(f"[reduce_mod_parts {kind} {(B, T, D)}] worst error / budget {r:.3f}")
