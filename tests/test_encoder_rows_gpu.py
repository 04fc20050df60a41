"""The frozen encoders' row kernels (csrc/encoder.hip) against fp64 in all three builds: ln_affine_bf16, the three forms of
ln_affine_f32, clip_im2col, clip_tokens, vit_tokens, preprocess_image.  (swiglu_rows has its fp64 test in
tests/test_tower_precision_gpu.py.)

Rules for every case (tests/encoder_ref.py; the budgets are proven on the CPU in tests/test_encoder_budgets_cpu.py): the
reference is fp64 from the inputs exactly as the kernel reads them, or the same fp32 chain where the kernel is a gather with at
most one addition (then the comparison is bit for bit); every output is pre-filled with NaN, a canary band follows it, every
case runs twice and must give the same bits.  Every base pointer is a fresh allocation (a multiple of 32 bytes: the fp32
build stores 8 floats per chunk).

ln_affine_kernel is one wave per row, lane l owning the 8-element chunks l, l + 64, l + 128, l + 192.  The widths: 8 (one live lane),
384 (lanes 48-63 idle), 512 (exactly one chunk per lane), 1024, 1280 (ViT-H: the third chunk exists for lanes 0-31 only; the
`ok ? ... : 0.f` loads and the guard on the variance sum keep it right), 1536 (ViT-g), 2048 (the limit).
"""
import pytest
import torch

from tests import encoder_ref as E
from tests.rowpass_ref import DTYPE, KINDS, Guarded, bits

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


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


def same_bits(tag, got, want):
    """Bit for bit: got (device) against want (CPU), the first differing element named."""
    g, w = bits(got.cpu()).flatten(), bits(want).flatten()
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, (f"{tag}: {bad.shape[0]} elements differ, the first at {int(bad[0])}: got "
                              f"{float(got.flatten()[int(bad[0])])!r}, want {float(want.flatten()[int(bad[0])])!r}")


def twice(fn):
    """Run fn() -> tuple of Guarded twice: canaries intact, the same bits both times.  Returns the first run's outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.intact() and y.intact(), "written past the end of an output"
        assert torch.equal(bits(x.full), bits(y.full)), "two runs differ"
    return a


def untouched(g):
    """The whole buffer still holds the NaN pre-fill (bit for bit) and its canary."""
    fresh = torch.full((g.n,), NAN, dtype=g.t.dtype, device=g.t.device)
    return g.intact() and torch.equal(bits(g.t), bits(fresh))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("M,D", E.LN_WIDTHS)
def test_ln_affine(dev, build, M, D):
    """ln_affine_bf16 (operand type in and out, eps 1e-5) and ln_affine_f32 (fp32 in, eps 1e-6; out = operand type or fp32; at
    D = 384 and 1280 also ldo = D + 8, whose 8 gap columns keep their NaN bits)."""
    from reed_amd import ops
    kind, dt = build, DTYPE[build]
    top = {}
    for entry, out_f32, gap in E.LN_FORMS:
        if gap and D not in E.LN_GAP_WIDTHS:
            continue
        inp = E.ln_inputs(M, D, kind, entry)
        ref = E.ln_reference(inp, out_f32)
        x, w, b = inp["x"].to(dev), inp["w"].to(dev), inp["b"].to(dev)
        odt, ldo = (F32 if out_f32 else dt), D + gap

        def run():
            out = Guarded(M * ldo, odt, dev)
            if entry == "bf16":
                ops.ln_affine_bf16(x, w, b, out.t, M, D, eps=E.LN_EPS["bf16"])
            else:
                ops.ln_affine_f32(x, w, b, out.t, out_f32, M, D, ldo=ldo, eps=E.LN_EPS["f32"])
            return (out,)

        out, = twice(run)
        o = out.t.view(M, ldo)
        form = f"ln_affine_{entry} -> {'fp32' if out_f32 else 'operand type'}"
        tag = f"{form} {kind} {(M, D)} ldo={ldo}"
        r = inside(tag, o[:, :D], ref["out"], ref["b_out"])
        top[form] = max(top.get(form, 0.0), r)
        if gap:
            assert torch.equal(bits(o[:, D:]), bits(torch.full((M, gap), NAN, dtype=odt, device=dev))), f"{tag}: gap written"
        if M > 1:         # the constant row: xhat is exactly 0, the output is b rounded to the output type, bit for bit
            same_bits(tag + " constant row", o[0, :D], inp["b"].to(odt))
    print(f"[ln_affine {kind} {(M, D)}] worst error / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in top.items()))


def test_ln_affine_refuses_bad_arguments(dev, build):
    from reed_amd import ops
    dt = DTYPE[build]
    M = 2
    x16, x32 = torch.ones(M * 2056, dtype=dt, device=dev), torch.ones(M * 2056, device=dev)
    w = torch.ones(2056, device=dev)
    for odt in (dt, F32):
        out = Guarded(M * 2064, odt, dev)
        for D in (12, 2056):
            if odt is dt:
                with pytest.raises(RuntimeError, match="ln_affine_bf16"):
                    ops.ln_affine_bf16(x16, w, w, out.t, M, D)
            with pytest.raises(RuntimeError, match="ln_affine_f32"):
                ops.ln_affine_f32(x32, w, w, out.t, odt is F32, M, D)
        for ldo in (384 - 8, 384 + 4):
            with pytest.raises(RuntimeError, match="ln_affine_f32"):
                ops.ln_affine_f32(x32, w, w, out.t, odt is F32, M, 384, ldo=ldo)
        torch.cuda.synchronize()
        assert untouched(out)                                # nothing was launched


# ------------------------------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("B,S,P,Kp", E.IM2COL_SHAPES)
def test_clip_im2col_bit_exact(dev, build, B, S, P, Kp):
    """(2, 28, 14, 592): K = 588, the last chunk straddles K; 640: whole padded chunks; (1, 32, 16, 768): no padding; (3, 6, 2, 16):
    K = 12 inside a second chunk.  The operand-type rounding of the gathered pixel, and +0 in every pad column."""
    from reed_amd import ops
    kind, dt = build, DTYPE[build]
    inp = E.im2col_inputs(B, S, P, Kp)
    img = inp["img"].to(dev)
    rows = B * (S // P) ** 2

    def run():
        out = Guarded(rows * Kp, dt, dev)
        ops.clip_im2col(img, out.t, B, S, P, Kp)
        return (out,)

    out, = twice(run)
    same_bits(f"clip_im2col {kind} {(B, S, P, Kp)}", out.t.view(rows, Kp), E.im2col_reference(inp, kind))


# ----------------------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("B,T,D", E.TOK_SHAPES)
def test_clip_tokens_bit_exact(dev, build, B, T, D):
    from reed_amd import ops
    kind, dt = build, DTYPE[build]
    inp = E.tok_inputs(B, T, D, kind, 1)
    patches, cls, pos = inp["patches"].to(dev), inp["cls"].to(dev), inp["pos"].to(dev)

    def run():
        out = Guarded(B * T * D, dt, dev)
        ops.clip_tokens(patches, cls, pos, out.t, B, T, D)
        return (out,)

    out, = twice(run)
    same_bits(f"clip_tokens {kind} {(B, T, D)}", out.t.view(B, T, D), E.clip_tokens_reference(inp))


@pytest.mark.parametrize("B,T,D,nprefix", E.vit_shapes())
def test_vit_tokens_bit_exact(dev, build, B, T, D, nprefix):
    """0 prefix rows (cls = None: I-JEPA), 1 (class token) and 5 (DINOv2 with registers), the prefix rows' pos non-zero."""
    from reed_amd import ops
    kind = build
    inp = E.tok_inputs(B, T, D, kind, nprefix)
    patches, pos = inp["patches"].to(dev), inp["pos"].to(dev)
    cls = inp["cls"].to(dev) if nprefix else None

    def run():
        out = Guarded(B * T * D, F32, dev)
        ops.vit_tokens(patches, cls, pos, out.t, B, T, D, nprefix=nprefix)
        return (out,)

    out, = twice(run)
    same_bits(f"vit_tokens {kind} {(B, T, D)} nprefix={nprefix}", out.t.view(B, T, D), E.vit_tokens_reference(inp))


def test_gathers_refuse_bad_arguments(dev, build):
    from reed_amd import ops
    dt = DTYPE[build]
    src32, src16 = torch.ones(4096, device=dev), torch.ones(4096, dtype=dt, device=dev)
    o16, o32 = Guarded(4096, dt, dev), Guarded(4096, F32, dev)
    for S, P, Kp in ((27, 14, 592), (28, 14, 584), (28, 14, 596)):       # S % P != 0, Kp < 3 P^2, Kp % 8 != 0
        with pytest.raises(RuntimeError, match="clip_im2col"):
            ops.clip_im2col(src32, o16.t, 1, S, P, Kp)
    for T, D in ((1, 8), (2, 12)):
        with pytest.raises(RuntimeError, match="clip_tokens"):
            ops.clip_tokens(src16, src32, src32, o16.t, 2, T, D)
    with pytest.raises(RuntimeError, match="vit_tokens"):                # T = nprefix
        ops.vit_tokens(src16, src32, src32, o32.t, 2, 5, 8, nprefix=5)
    with pytest.raises(RuntimeError, match="vit_tokens"):                # prefix rows asked for, none given
        ops.vit_tokens(src16, None, src32, o32.t, 2, 5, 8, nprefix=1)
    torch.cuda.synchronize()
    assert untouched(o16) and untouched(o32)                 # nothing was launched


# --------------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("case", E.PRE_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}o{c[3]}{'odd' if c[4] is E.ODD_MEAN else ''}")
def test_preprocess_image(dev, build, case):
    """16 -> 16: the S == R branch; 16 -> 8: every coordinate exact in fp32 (no coordinate term); 16 -> 14; 8 -> 12: upsampling,
    negative source coordinates and taps two outside the image at both edges.  Image 1 of a pair is a 0 / 255 checkerboard."""
    from reed_amd import ops
    B, R, S, order, mean, std = case
    inp = E.pre_inputs(B, R)
    ref = E.pre_reference(inp, S, order, mean, std)
    raw = inp["raw"].to(dev)

    def run():
        out = Guarded(B * 3 * S * S, F32, dev)
        ops.preprocess_image(raw, out.t, B, R, S, mean, std, order)
        return (out,)

    out, = twice(run)
    r = inside(f"preprocess_image {build} {case[:4]}", out.t.view(B, 3, S, S), ref["out"], ref["b_out"])
    print(f"[preprocess_image {build} {case[:4]} mean {mean[0]:.2f}..] worst error / budget: out {r:.3f}")


def test_preprocess_refuses_bad_order(dev, build):
    from reed_amd import ops
    raw = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device=dev)
    out = Guarded(3 * 14 * 14, F32, dev)
    with pytest.raises(RuntimeError, match="preprocess_image"):
        ops.preprocess_image(raw, out.t, 1, 16, 14, E.CLIP_MEAN, E.CLIP_STD, 2)
    torch.cuda.synchronize()
    assert untouched(out)
