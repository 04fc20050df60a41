"""The embedders, the conditioning kernels and the small-K weight gradient of csrc/embed.hip against fp64, in all three builds:
reed_smallk_wgrad (four instantiations, two layouts, the K walk over blockIdx.z, the clamped and masked row tail, null outputs),
reed_patch_embed_fwd (the register form and the generic kernel at K = 8, 16, 64, 256), reed_patchify_bf16 (both orders, exact),
reed_timestep_sinusoid, reed_label_cond and reed_label_cond_bwd.  tests/embed_ref.py holds the references and the budgets (proven on
the CPU in tests/test_embed_budgets_cpu.py).  Every output lives in a NaN pre-filled buffer with a canary band behind it, every call
runs twice and must give the same bits, every element is held to its budget and the worst one is named
(tests/test_final_layer_gpu.py, tests/test_reductions_gpu.py).  profiles/embed_tests.txt records the measured ratios.

Small-K shapes (M, Dw, KS), per = ceil(M / 256) rows per slice, RG rows per load group:
  (1, 2, 8)        one row, one column pair, the smallest KS; 255 empty slices
  (255, 130, 16)   M < 256 slices; a second column block with one live lane
  (257, 128, 32)   per = 2, one half-filled slice, slices starting past M
  (2309, 66, 16)   per = 10 with RG = 8: a masked tail of 6 rows in every slice
  (2309, 130, 40)  RG = 4; two z blocks, the second with one live 8-chunk
  (700, 34, 24)    KSP = 32 with a partial last chunk in a single z block
  (320, 384, 64)   patch 4
  (80, 128, 256)   patch 8; 8 z blocks
Patch-embed shapes (B, C, HW, P, D):
  (1, 4, 2, 2, 4)      one token, one live thread of the register form
  (5, 4, 18, 2, 1280)  405 tokens = 6 x 64 + 21; every one of the 320 threads live
  (5, 4, 18, 2, 1284)  past the register form's width: the generic kernel at K = 16
  (3, 4, 12, 4, 260)   K = 64; 27 tokens (a tail of 3 in a block of 8); a second trip of the column loop with 4 live threads
  (3, 2, 6, 2, 72)     K = 8
  (1, 4, 16, 8, 128)   K = 256
"""
import pytest
import torch

from tests import embed_ref as E
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits
from tests.test_final_layer_gpu import _at, inside

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(params=KINDS)
def build(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def _bits(t):
    return t.contiguous().view(torch.int64) if t.element_size() == 8 else bits(t)


def _intact(g):
    return torch.equal(_bits(g.full[g.n:]), _bits(g.band))


def twice(fn):
    """Run fn() -> tuple of Guarded (or None) twice: canaries intact, the same bits both times.  Returns the first run's outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is None:
            assert y is None
            continue
        assert _intact(x) and _intact(y), "written past the end of an output"
        assert torch.equal(_bits(x.full), _bits(y.full)), "two runs differ"
    return a


def _show(tag, r):
    print(f"[{tag}] worst error / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ------------------------------------------------------------------------------------------------------- small-K wgrad
@pytest.mark.parametrize("M,Dw,KS", E.SMALLK_SHAPES)
def test_smallk_wgrad(dev, build, M, Dw, KS):
    from reed_amd import ops
    kind = build
    nws = ops.smallk_ws_floats(Dw, KS)
    assert nws == E.NSL * (KS * Dw + Dw + KS)
    seen = set()
    for wide_f32 in (True, False):
        inp = E.smallk_inputs(M, Dw, KS, kind, wide_f32)
        wide, small = inp["wide"].to(dev), inp["small"].to(dev)
        priors = [inp[k].to(dev) for k in ("prior_out", "prior_cw", "prior_cs")]
        form, nz = E.smallk_form(KS, wide_f32)
        seen.add(form)
        for layout in (0, 1):
            for accumulate in (False, True):
                ref = E.smallk_reference(inp, layout, accumulate)

                def run(skip=None):
                    ws = Guarded(nws, F32, dev)               # NaN: a slot the reduce reads but stage 1 never wrote shows
                    outs = []
                    for i, n in enumerate((Dw * KS, Dw, KS)):
                        if i == skip:
                            outs.append(None)
                            continue
                        o = Guarded(n, F32, dev)
                        if accumulate:
                            o.t.copy_(priors[i])
                        outs.append(o)
                    ops.smallk_wgrad(wide, wide_f32, small, ws.t, *(o.t if o is not None else None for o in outs), M, Dw, KS, layout,
                                     accumulate)
                    return (*outs, ws)

                full = twice(run)
                tag = f"small-K {kind} {(M, Dw, KS)} {form} z={nz} layout {layout} accumulate={accumulate}"
                r = {k: inside(f"{tag} {k}", o.t, ref[k], ref["b_" + k]) for k, o in zip(E.SMALLK_OUTPUTS, full)}
                assert bool(torch.isfinite(full[3].t).all()), "a workspace slot was left unwritten"
                _show(tag, r)
                for skip in range(3):                          # one output null: the others come out bit for bit the same
                    part = twice(lambda: run(skip))            # noqa: B023
                    assert part[skip] is None
                    for i in range(3):
                        if i != skip:
                            assert torch.equal(bits(part[i].t), bits(full[i].t)), (tag, "null output", skip, i)
    assert len(seen) == 2


# ------------------------------------------------------------------------------------------- patchify and patch embed
ALIGNED_FORM = {(1, 4, 2, 2, 4): "reg16", (5, 4, 18, 2, 1280): "reg16", (5, 4, 18, 2, 1284): "generic", (3, 4, 12, 4, 260): "generic",
                (3, 2, 6, 2, 72): "generic", (1, 4, 16, 8, 128): "generic"}


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,C,HW,P,D", E.PATCH_SHAPES)
def test_patch_embed_fwd(dev, build, B, C, HW, P, D, bias):
    from reed_amd import ops
    kind = build
    inp = E.patch_inputs(B, C, HW, P, D, kind)
    ref = E.patch_reference(inp, bias)
    T, K = inp["T"], inp["K"]
    x, pos = inp["x"].to(dev), inp["pos"].to(dev)
    bv = inp["bias"].to(dev) if bias else None
    first = None
    for residue in ((0, 8) if K == 16 else (0,)):              # 8 (mod 16): the entry point falls back to the generic kernel
        w = _at(inp["w"].to(dev), residue, dev)
        form = E.embed_form(kind, K, D, residue == 0)
        assert form == (ALIGNED_FORM[(B, C, HW, P, D)] if residue == 0 else "generic")

        def run():
            tok = Guarded(B * T * D, F32, dev)
            assert tok.t.data_ptr() % 16 == 0 and pos.data_ptr() % 16 == 0
            ops.patch_embed_fwd(x, w, bv, pos, tok.t, B, C, HW, P, D)
            return (tok,)

        (tok,) = twice(run)
        tag = f"patch embed {kind} {(B, C, HW, P, D)} K={K} bias={bias} weight at {residue} (mod 16): {form}"
        _show(tag, {"tok": inside(tag, tok.t, ref["tok"], ref["b_tok"])})
        if first is None:
            first = tok
        else:                                                  # one chain over k in both kernels: bit-identical
            assert torch.equal(bits(first.t), bits(tok.t)), tag


@pytest.mark.parametrize("B,C,HW,P,D", E.PATCH_SHAPES)
def test_patchify_exact(dev, build, B, C, HW, P, D):
    from reed_amd import ops
    kind = build
    dt = DTYPE[kind]
    inp = E.patch_inputs(B, C, HW, P, D, kind)
    x = inp["x"].to(dev)
    n = B * C * HW * HW
    for order in (0, 1):
        want = inp["x"].flatten()[E.patch_src_index(B, C, HW, P, order)].to(dt)

        def run():
            out = Guarded(n, dt, dev)
            ops.patchify_bf16(x, out.t, B, C, HW, P, order)
            return (out,)

        (out,) = twice(run)
        assert torch.equal(bits(out.t.cpu()), bits(want)), (kind, order)
    print(f"[patchify {kind} {(B, C, HW, P)}] orders 0 and 1 exact")


# ------------------------------------------------------------------------------------------------------------ sinusoid
@pytest.mark.parametrize("dim,max_period", E.SIN_CASES)
def test_timestep_sinusoid(dev, build, dim, max_period):
    from reed_amd import ops
    kind = build
    inp = E.sin_inputs(kind)
    ref = E.sin_reference(inp, dim, max_period)
    t = inp["t"].to(dev)
    B = len(t)

    def run():
        out = Guarded(B * dim, DTYPE[kind], dev)
        ops.timestep_sinusoid(t, out.t, B, dim, max_period)
        return (out,)

    (out,) = twice(run)
    tag = f"sinusoid {kind} dim {dim} max_period {max_period:g}"
    _show(tag, {"out": inside(tag, out.t, ref["out"], ref["b_out"])})
    if dim % 2:
        assert bool((out.t.view(B, dim)[:, -1] == 0).all()), "the odd column is an exact 0"


# -------------------------------------------------------------------------------------------------- label conditioning
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("B,D,NC", E.LABEL_SHAPES)
def test_label_cond_fwd_and_bwd(dev, build, B, D, NC, drop):
    from reed_amd import ops
    kind = build
    dt = DTYPE[kind]
    inp = E.label_inputs(B, D, NC, kind, drop)
    ref = E.label_reference(inp)
    labels, table, temb = inp["labels"].to(dev), inp["table"].to(dev), inp["t_emb"].to(dev)
    mask = inp["drop"].to(dev) if drop else None

    def fwd(with_labels_out=True):
        lo = Guarded(B, torch.int64, dev, fill=-7) if with_labels_out else None
        c, sc = Guarded(B * D, F32, dev), Guarded(B * D, dt, dev)
        ops.label_cond(labels, mask, NC, table, temb, lo.t if lo is not None else None, c.t, sc.t, B, D)
        return lo, c, sc

    lo, c, sc = twice(fwd)
    tag = f"label conditioning {kind} {(B, D, NC)} drop={drop}"
    assert lo.t.tolist() == ref["eff"].tolist(), tag
    assert torch.equal(bits(c.t.cpu()), bits(ref["c32"].flatten())), f"{tag}: c is one fp32 addition, exact"
    r = {"silu_c": inside(f"{tag} silu_c", sc.t, ref["silu_c"], ref["b_silu_c"])}
    _, c2, sc2 = twice(lambda: fwd(False))                     # labels_out = None: the same c and silu_c
    assert torch.equal(bits(c2.t), bits(c.t)) and torch.equal(bits(sc2.t), bits(sc.t))

    dsilu, prior = inp["dsilu"].to(dev), inp["prior"].to(dev)

    def bwd():
        dte, dtab = Guarded(B * D, dt, dev), Guarded((NC + 1) * D, F32, dev)
        dtab.t.copy_(prior.flatten())
        ops.label_cond_bwd(dsilu, c.t, lo.t, dte.t, dtab.t, B, D)
        return dte, dtab

    dte, dtab = twice(bwd)
    r["dt_emb"] = inside(f"{tag} dt_emb", dte.t, ref["dt_emb"], ref["b_dt_emb"])
    r["dtable"] = inside(f"{tag} dtable", dtab.t, ref["dtable"], ref["b_dtable"])
    un = ref["untouched"].to(dev)
    assert torch.equal(bits(dtab.t.view(NC + 1, D)[un]), bits(prior[un])), f"{tag}: a row no label selects comes back bit for bit"
    assert int(ref["untouched"].sum()) == NC + 1 - len(set(ref["eff"].tolist()))
    _show(tag, r)
