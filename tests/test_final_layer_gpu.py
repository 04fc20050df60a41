"""The final layer of csrc/embed.hip against fp64: reed_final_layer_fwd (out, mean, rstd) and reed_final_layer_bwd_rows (hbuf, dlin,
dh), in the form that stages the weight in LDS per 64 rows and in the wave-per-row form, with and without bias, in all three
builds.  tests/adaln_ref.py holds the reference and the budgets (proven on the CPU in tests/test_adaln_budgets_cpu.py); NaN
pre-fill, canary bands, two runs bit-equal as in tests/test_reductions_gpu.py.

(B, T) = (3, 9): odd T and odd M, so the LDS form's row pairs straddle two samples and a last single row is left; (5, 16): one full
64-row group plus a tail; (1, 1): a single row.  Which form runs follows from the size rules of the entry points, restated in
adaln_ref.final_form: the test computes it, says it, and a weight at an address that is 8 (mod 16) forces the wave-per-row form.
"""
import pytest
import torch

from tests import adaln_ref as A
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits
from tests.test_oracle_golden import load

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


def _at(t, residue, dev):
    """The values of t at a device address that is `residue` (mod 16)."""
    es = t.element_size()
    buf = torch.empty(t.numel() + 32, dtype=t.dtype, device=dev)
    k = ((residue - buf.data_ptr()) % 16) // es
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == residue
    return v


def _placements(kind):
    """16-byte aligned in every build.  8 (mod 16) in the 16-bit builds only: there the kernels' weight loads are 8 bytes wide; in
    the fp32 build they are 16 bytes wide and such an address is outside what a kernel may be given."""
    return (0, 8) if kind != "fp32" else (0,)


def _run_case(dev, kind, inp, ref, bias, tag):
    from reed_amd import ops
    dt = DTYPE[kind]
    B, T, D, C, P, M, NO, HW = (inp[k] for k in ("B", "T", "D", "C", "P", "M", "NO", "HW"))
    d = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    es, ld = d["mod"].element_size(), d["mod"].shape[1]
    shift, scale = d["mod"].data_ptr(), d["mod"].data_ptr() + D * es
    forms, res, first = set(), {}, None
    for residue in _placements(kind):
        w = _at(d["w"], residue, dev)
        f_fwd, f_bwd = A.final_form(kind, C, P, D, False, residue == 0), A.final_form(kind, C, P, D, True, residue == 0)
        assert residue == 0 or (f_fwd, f_bwd) == ("rows", "rows")
        forms |= {("fwd", f_fwd), ("bwd", f_bwd)}

        def run():
            out, mean, rstd = Guarded(B * C * HW * HW, F32, dev), Guarded(M, F32, dev), Guarded(M, F32, dev)
            hbuf, dlin, dh = Guarded(M * D, dt, dev), Guarded(M * NO, dt, dev), Guarded(M * D, dt, dev)
            ops.final_layer_fwd(d["x"], shift, scale, ld, w, d["bias"] if bias else None, out.t, mean.t, rstd.t, B, T, D, C, P)
            ops.final_layer_bwd_rows(d["dout"], d["x"], d["mean"], d["rstd"], shift, scale, ld, w, hbuf.t, dlin.t, dh.t, B, T, D, C, P)
            return out, mean, rstd, hbuf, dlin, dh

        outs = twice(run)
        got = dict(zip(("out", "mean", "rstd", "hbuf", "dlin", "dh"), outs))
        r = {k: inside(f"{tag} w % 16 = {residue} ({f_fwd} / {f_bwd}) {k}", got[k].t, ref[k], ref["b_" + k]) for k in A.FINAL_OUTPUTS}
        assert torch.equal(bits(got["dlin"].t), bits(ref["dlin"].to(dt).to(dev).flatten())), "dlin = round(dout), (pi, pj, c) order"
        print(f"[{tag}, weight at {residue} (mod 16): forward {f_fwd}, backward rows {f_bwd}] worst error / budget: "
              + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        if first is None:
            first = outs
        else:       # the two forms share one formula: bit-identical
            for a, b in zip(first, outs):
                assert torch.equal(bits(a.t), bits(b.t))
        res[residue] = r
    return forms


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,T,D,C,P", A.FINAL_SHAPES)
def test_final_layer_fwd_and_bwd_rows(dev, build, B, T, D, C, P, bias):
    kind = build
    inp = A.final_inputs(B, T, D, C, P, kind)
    ref = A.final_reference(inp, bias=bias)
    forms = _run_case(dev, kind, inp, ref, bias, f"final layer {kind} {(B, T, D, C, P)} bias={bias}")
    # the form the size rules pick for this (build, C, D) with an aligned weight: an XL-width weight leaves the LDS form in the
    # fp32 build, and in the 16-bit builds once P P C = 32
    NO = P * P * C
    fits = NO * D * (4 if kind == "fp32" else 2) <= 64 * 1024
    assert ("fwd", "lds" if fits else "rows") in forms
    assert fits == (not (D == 1152 and (kind == "fp32" or NO == 32)))


def test_both_forms_are_reached_in_every_build():
    for kind in KINDS:
        seen = set()
        for _, _, D, C, P in A.FINAL_SHAPES:
            for residue in _placements(kind):
                for backward in (False, True):
                    seen.add((backward, A.final_form(kind, C, P, D, backward, residue == 0)))
        assert seen == {(False, "lds"), (False, "rows"), (True, "lds"), (True, "rows")}, (kind, seen)


def test_final_layer_at_the_golden_unpatchify_size(dev, build):
    """T = 256, C = 4, P = 2: the size the reference's own unpatchify map (golden `unpatchify_idx`) covers.  The expected output is
    laid out through that map, not through the restatement."""
    kind = build
    B, T, D, C, P = 1, 256, 384, 4, 2
    inp = A.final_inputs(B, T, D, C, P, kind)
    ref = A.final_reference(inp)
    un = torch.from_numpy(load("static")["unpatchify_idx"]).flatten().long()      # out.flat[i] = lin.flat[un[i]]
    for k in ("out", "b_out"):
        lin = A.patchify_out(ref[k], C, P)
        ref[k] = lin.flatten()[un].reshape(ref[k].shape)
    dl = torch.zeros(T * P * P * C, dtype=torch.float64)
    dl[un] = A.rnd(inp["dout"].double(), kind).flatten()                           # lin.flat[un[i]] = out.flat[i]
    assert torch.equal(dl.reshape(T, -1), ref["dlin"])
    _run_case(dev, kind, inp, ref, True, f"final layer {kind} golden map {(B, T, D, C, P)}")


def test_final_layer_bwd_rows_refuses_bad_shapes(dev, build):
    """A non-square T would read dout through HW = round(sqrt(T)) * P; B or T <= 0 is a zero-sized grid."""
    from reed_amd import ops
    dt, D, C, P = DTYPE[build], 8, 4, 2
    x = torch.ones(16, D, device=dev)
    dout = torch.ones(16 * C * P * P, device=dev)
    st = torch.ones(16, device=dev)
    mod = torch.zeros(2, 6 * D + 8, dtype=dt, device=dev)
    w = torch.zeros(C * P * P, D, dtype=dt, device=dev)
    outs = [Guarded(16 * D, dt, dev, fill=7.0), Guarded(16 * C * P * P, dt, dev, fill=7.0), Guarded(16 * D, dt, dev, fill=7.0)]
    for B, T, what in ((2, 8, "square"), (1, 15, "square"), (0, 4, "bad B"), (2, 0, "bad B"), (-1, 4, "bad B"), (2, -4, "bad B")):
        with pytest.raises(RuntimeError, match=what):
            ops.final_layer_bwd_rows(dout, x, st, st, mod.data_ptr(), mod.data_ptr() + D * mod.element_size(), mod.shape[1], w,
                                     outs[0].t, outs[1].t, outs[2].t, B, T, D, C, P)
    torch.cuda.synchronize()
    for o in outs:                                              # nothing was launched
        assert o.intact() and (o.t == 7.0).all()
