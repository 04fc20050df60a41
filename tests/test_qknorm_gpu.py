"""reed_qk_norm_fwd / reed_qk_norm_bwd (csrc/qknorm.hip) against fp64, in every build and at both head sizes, and the first
runs of qk-norm at head_dim 72 through the engine.

Kernel level: every output is held to the per-element budgets of tests/rowpass_ref.py (derived from the arithmetic and proven on
the CPU by tests/test_rowpass_budgets_cpu.py), the layouts of `stats` and `part` are the ones include/reed_hip.h documents, v
passes through bit for bit, nothing is written past an output, and two runs give the same bits.  Path level: losses and every
parameter's gradient against the oracle at the bars the existing tiny cases use.
"""
import numpy as np
import pytest
import torch

from oracle import detfill
from oracle import loss as oloss
from oracle import sit as osit
from tests.rowpass_ref import DTYPE, KINDS, QK_SHAPES, U, Guarded, bits, qk_inputs, qk_reference, worst
from tests.test_model_gpu import GRAD_BAR, build_hip_model, cos
from tests.test_oracle_golden import inputs, tiny_cfg

pytestmark = pytest.mark.gpu

_REF = {}


def _case(kind, shape):
    """(inputs, fp64 reference) of one (build, shape): computed once on the CPU, shared, never modified."""
    if (kind, shape) not in _REF:
        inp = qk_inputs(*shape, kind)
        _REF[(kind, shape)] = (inp, qk_reference(inp))
    return _REF[(kind, shape)]


@pytest.fixture(params=KINDS)
def build(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def check(name, got, ref, budget, tag, describe=None):
    """got within budget of ref, element by element; prints the worst error / budget and, outside, names the element."""
    got = got.double().cpu().reshape(ref.shape)
    r, i = worst((got - ref).abs(), budget)
    print(f"[{tag}] {name}: worst error / budget {r:.3f}")
    if not r <= 1.0:
        idx = tuple(int(v) for v in np.unravel_index(i, ref.shape))
        b = float(budget.expand(ref.shape).flatten()[i])
        extra = describe(idx) if describe else ""
        raise AssertionError(f"{tag} {name}{list(idx)}: got {float(got.flatten()[i])!r}, fp64 {float(ref.flatten()[i])!r}, "
                             f"budget {b:.3e}, ratio {r:.3g} {extra}")
    return r


def run_qk(ops, inp, dev, with_stats=True):
    M, H, hd, dt = inp["M"], inp["H"], inp["hd"], DTYPE[inp["kind"]]
    d = {k: inp[k].to(dev) for k in ("qkv", "dn", "qw", "qb", "kw", "kb")}
    n = M * 3 * H * hd
    nb = (M * 3 * H + 255) // 256
    out, dpre = Guarded(n, dt, dev), Guarded(n, dt, dev)
    stats, part = Guarded(M * 2 * H * 2, torch.float32, dev), Guarded(nb * 4 * hd, torch.float32, dev)
    ops.qk_norm_fwd(d["qkv"], d["qw"], d["qb"], d["kw"], d["kb"], out.t, stats.t if with_stats else None, M, H, hd)
    if with_stats:
        ops.qk_norm_bwd(d["dn"], d["qkv"], stats.t, d["qw"], d["kw"], dpre.t, part.t, M, H, hd)
    torch.cuda.synchronize()
    return d, out, stats, dpre, part


@pytest.mark.parametrize("shape", QK_SHAPES)
def test_qk_norm_kernels_vs_fp64(dev, build, shape):
    from reed_amd import _lib, ops
    kind = build
    M, H, hd = shape
    inp, ref = _case(kind, shape)
    tag = f"qk-norm {kind} {shape}"
    nb = -(-3 * M * H // 256)
    assert int(_lib.load(kind).reed_qk_norm_bwd_part_floats(M, H, hd)) == nb * 4 * hd and ref["nblocks"] == nb
    d, out, stats, dpre, part = run_qk(ops, inp, dev)

    def seg(idx):   # the segment an element of out / dpre belongs to, with its terms
        m, w, h = idx[0], idx[1], idx[2]
        x = inp["qkv"][m, w, h].double()
        return (f"(token {m}, {'qk'[w]}, head {h}, block {((m * 3 + w) * H + h) // 256}; segment mean {float(x.mean()):.6g}, "
                f"std {float(x.std(unbiased=False)):.6g}, rstd {float(ref['stats'][m, w, h, 1]):.6g})")

    o = out.t.view(M, 3, H, hd)
    dp = dpre.t.view(M, 3, H, hd)
    check("out", o[:, :2], ref["out"], ref["b_out"], tag, seg)
    check("stats", stats.t.view(M, 2, H, 2), ref["stats"], ref["b_stats"], tag)       # [M, 2 (q,k), H, 2 (mean, rstd)]
    check("dpre", dp[:, :2], ref["dpre"], ref["b_dpre"], tag, seg)
    p = part.t.view(nb, 2, 2, hd)                                                    # [nblocks, 2 (q,k), 2 (dw,db), hd]
    assert not torch.isnan(p).any(), "a slot of part was not written"
    check("part", p, ref["part"], ref["b_part"], tag, lambda i: f"(block {i[0]}, {'qk'[i[1]]}, {('dw', 'db')[i[2]]})")
    # the constant segment: variance 0, eps decides, the output is the bias rounded to the output type
    assert torch.equal(o[0, 1, H - 1].cpu(), inp["kb"].to(DTYPE[kind]))
    # v passes through bit for bit, forward and backward
    assert torch.equal(bits(o[:, 2]), bits(d["qkv"][:, 2]))
    assert torch.equal(bits(dp[:, 2]), bits(d["dn"][:, 2]))
    for g in (out, stats, dpre, part):
        assert g.intact(), "written past the end of an output"
    # stats = NULL: the same forward bits; a second run: the same bits everywhere (deterministic)
    _, out_ns, stats_ns, _, _ = run_qk(ops, inp, dev, with_stats=False)
    assert torch.equal(bits(out_ns.t), bits(out.t)) and torch.isnan(stats_ns.t).all() and out_ns.intact()
    _, out2, stats2, dpre2, part2 = run_qk(ops, inp, dev)
    for a, b in ((out, out2), (stats, stats2), (dpre, dpre2), (part, part2)):
        assert torch.equal(bits(a.full), bits(b.full))

    # the engine's contract: rowsum_f32 over the blocks lands [q dw | q db | k dw | k db] (the four gradient vectors are
    # contiguous in the arena), accumulating onto what is there; the one extra rounding of that last addition is the u term
    base = (torch.arange(4 * hd, dtype=torch.float32) * 0.01 - 1.0)
    want = base.double() + ref["total"].flatten()
    budget = ref["b_total"].flatten() + U * want.abs()
    ws = torch.empty((nb + 63) // 64 * 4 * hd, device=dev)
    res = []
    for w in (None, ws):
        acc = Guarded(4 * hd, torch.float32, dev)
        acc.t.copy_(base)
        ops.rowsum_f32(part.t, nb, acc.t, 4 * hd, True, ws=w)
        torch.cuda.synchronize()
        check("rowsum(part) onto the gradient" + (" with ws" if w is not None else ""), acc.t, want, budget, tag,
              lambda i: f"({('q dw', 'q db', 'k dw', 'k db')[i[0] // hd]}[{i[0] % hd}])")
        assert acc.intact()
        res.append(acc.t.clone())
    assert torch.equal(bits(res[0]), bits(res[1]))


def test_qk_norm_refuses_what_it_cannot_do(dev, build):
    from reed_amd import ops
    dt = DTYPE[build]
    M, H = 4, 2
    for hd in (80, 64):
        qkv = torch.zeros(M * 3 * H * hd, dtype=dt, device=dev)
        out = torch.full_like(qkv, 7.0)
        v = torch.ones(hd, device=dev)
        stats, part = torch.zeros(M * 2 * H * 2, device=dev), torch.full((4 * hd,), 7.0, device=dev)
        if hd == 80:      # neither instantiation exists
            with pytest.raises(RuntimeError, match="head_dim 80"):
                ops.qk_norm_fwd(qkv, v, v, v, v, out, stats, M, H, hd)
            with pytest.raises(RuntimeError, match="head_dim 80"):
                ops.qk_norm_bwd(qkv, qkv, stats, v, v, out, part, M, H, hd)
        else:             # null pointers
            for miss in range(6):
                a = [qkv, v, v, v, v, out]
                a[miss] = None
                with pytest.raises(RuntimeError, match="null pointer"):
                    ops.qk_norm_fwd(*a, stats, M, H, hd)
            for miss in range(7):
                a = [qkv, qkv, stats, v, v, out, part]
                a[miss] = None
                with pytest.raises(RuntimeError, match="null pointer"):
                    ops.qk_norm_bwd(*a, M, H, hd)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (part == 7.0).all()     # nothing was launched


# ---------------------------------------------------------------------------------------------------------- path level
def _run_pair(cfg, dev, precision, zdim):
    """One loss + backward of the HIP model and of the oracle at the same precision on the same seeded inputs."""
    from reed_amd.loss import SILoss
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, noise, t, y, drop_u, zs = inputs(4, 4, cfg["input_size"], 11, [(zdim, "i")], T, cfg["num_classes"])
    drop = drop_u < cfg["class_dropout_prob"]
    m = build_hip_model(cfg, dev, 11)
    m.precision = precision
    m.train()
    m.force_drop_mask = drop
    lf = SILoss(enc_names=["dinov2"], loss_weights={"dinov2": 1.0})
    out = lf(m, x.to(dev), dict(y=y.to(dev)), zs=[z.to(dev) for z in zs], time_input=t, noises=noise)
    total = out["denoising_loss"].mean() + 0.5 * out["proj_loss"]
    total.backward()
    torch.cuda.synchronize()
    P = detfill.fill_state_dict(osit.init_params(cfg), base_seed=11)
    P = {k: v.requires_grad_(k != "pos_embed") for k, v in P.items()}
    om = osit.OracleModel(P, cfg, autocast_bf16=(precision == "bf16"), training=True)
    om.drop_mask = drop
    oo = oloss.si_loss(om, x, dict(y=y), zs, enc_names=["dinov2"], loss_weights={"dinov2": 1.0}, t=t, noise=noise)
    ototal = oo["denoising_loss"].mean() + 0.5 * oo["proj_loss"]
    ototal.backward()
    return m, out, total, P, oo, ototal


def test_qk_norm_hd72_through_the_engine_bf16(dev):
    """SiT-XL's head layout (16 heads of 72) with --qk-norm, two blocks, against the bf16-autocast oracle at the bars of
    test_tiny_vs_reference_and_oracle (imported, not copied)."""
    cfg = tiny_cfg(D=1152, heads=16, depth=2, input_size=8, projector_dim=256, qk_norm=True)
    m, out, total, P, oo, ototal = _run_pair(cfg, dev, "bf16", 128)
    np.testing.assert_allclose(out["denoising_loss"].detach().cpu().numpy(), oo["denoising_loss"].detach().numpy(), rtol=5e-3)
    np.testing.assert_allclose(float(out["proj_loss"]), float(oo["proj_loss"]), rtol=2e-2, atol=2e-3)
    bad, worst_c, worst_n, seen = [], (1.0, ""), (0.0, ""), 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        gh, go = p.grad.detach().cpu().float(), P[k].grad
        nh, no = gh.norm().item(), go.norm().item()
        if no < 5e-5:   # analytically zero (k_norm.bias: softmax is invariant to a common key shift)
            assert nh < 5e-4, (k, nh, no)
            continue
        cs, dn = cos(gh, go), abs(nh / no - 1)
        seen += "_norm." in k
        worst_c, worst_n = min(worst_c, (cs, k)), max(worst_n, (dn, k))
        if "_norm." in k:
            print(f"[qk-norm engine, bf16, hd 72] {k}: cosine {cs:.6f}, |norm ratio - 1| {dn:.5f}")
        if cs < GRAD_BAR[0] or dn > GRAD_BAR[1]:
            bad.append((k, cs, dn))
    print(f"[qk-norm engine, bf16, hd 72] worst cosine {worst_c[0]:.6f} ({worst_c[1]}), worst |norm ratio - 1| {worst_n[0]:.5f} "
          f"({worst_n[1]})")
    assert seen >= 6, "the q_norm / k_norm gradients were not compared"
    assert not bad, bad[:8]


def test_qk_norm_hd72_through_the_engine_fp32(dev):
    """The fp32 build at D = 144 (two heads of 72) with qk-norm against the fp32 oracle, at the bars of
    test_tiny_fp32_vs_reference: losses to 2e-5, every gradient norm to 1e-4, gradient elements at cosine 1 - 1e-6."""
    cfg = tiny_cfg(D=144, z_dims=[64], qk_norm=True)
    m, out, total, P, oo, ototal = _run_pair(cfg, dev, "fp32", 64)
    np.testing.assert_allclose(out["denoising_loss"].detach().cpu().numpy(), oo["denoising_loss"].detach().numpy(), rtol=2e-5)
    np.testing.assert_allclose(float(total), float(ototal), rtol=2e-5, atol=2e-6)
    params = dict(m.named_parameters())
    worst_n, worst_c = 0.0, 1.0
    for k, p in params.items():
        if not p.requires_grad:
            continue
        ref_n, nh = P[k].grad.double().norm().item(), p.grad.float().norm().item()
        if ref_n < 5e-5:
            assert nh < 5e-5, (k, nh, ref_n)
            continue
        worst_n = max(worst_n, abs(nh / ref_n - 1))
        assert abs(nh / ref_n - 1) < 1e-4, (k, nh, ref_n)
    for k in ("final_layer.linear.bias", "x_embedder.proj.bias", "projectors.0.4.bias", "final_layer.linear.weight",
              "blocks.0.attn.qkv.bias", "x_embedder.proj.weight", "blocks.1.adaLN_modulation.1.bias", "blocks.2.mlp.fc1.bias",
              "blocks.0.attn.q_norm.weight", "blocks.0.attn.q_norm.bias", "blocks.0.attn.k_norm.weight",
              "blocks.2.attn.q_norm.weight", "blocks.2.attn.k_norm.weight"):
        cs = cos(params[k].grad.detach().cpu(), P[k].grad)
        worst_c = min(worst_c, cs)
        assert cs > 1 - 1e-6, (k, cs)
    print(f"[qk-norm engine, fp32, hd 72] worst |gradient norm ratio - 1| vs the fp32 oracle {worst_n:.2e}, worst element cosine "
          f"{worst_c:.8f}")
