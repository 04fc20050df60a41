"""LoRA through reed_amd.SiT on the GPU (reed_amd/lora.py, csrc/lora.hip), on the tiny cases of tests/test_oracle_golden.py:
a fresh adapted model computes what the model without adapters computes; the adapters' gradients against oracle/sit.py at fp64 with
P[weight] = W + s B A and A, B as leaves of plain autograd; three fused optimiser steps of adapters-only training; gradient
accumulation; the merged export and the adapter file.

Setup of the gradient test: functional, inputs and base fill of tests/test_input_grad_model_gpu.py (seed 11, inference=False);
A = detfill.normal((R, K), 9000 + k) / sqrt(K), B = 0.02 detfill.normal((N, R), 9500 + k), k counting the adapted linears block by
block in the order qkv, proj, fc1, fc2; alpha = 2 R.  Bars: 16-bit builds per-tensor cosine >= 0.9999 and |norm ratio - 1| <= 0.012
(GRAD_BAR's cosine and 3 x its norm bar: the project's bars against a higher-precision reference); fp32 build cosine > 1 - 1e-6 and
norm gap < 1e-4.  The gap to the bf16-autocast oracle is printed, not asserted: the kernels round u / v where autocast does not.
"""
import copy

import pytest
import torch

from oracle import detfill
from oracle import sit as osit
from reed_amd import lora
from tests.rowpass_ref import KINDS, bits
from tests.test_input_grad_model_gpu import _case, functional
from tests.test_model_gpu import GRAD_BAR, build_hip_model, cos
from tests.test_oracle_golden import TINY_CASES, inputs

pytestmark = pytest.mark.gpu
CASES_16 = ("hd64", "patch4", "two_split", "qknorm")
_REF = {}


def adapter_fill(shapes, R):
    """{name: tensor} of the deterministic adapters for the adapted linears in `shapes` (name -> (n_out, k_in)), in order."""
    out = {}
    for k, (lin, (N, K)) in enumerate(shapes.items()):
        out[lin + ".lora_A"] = detfill.normal((R, K), 9000 + k) / K ** 0.5
        out[lin + ".lora_B"] = 0.02 * detfill.normal((N, R), 9500 + k)
    return out


def linear_shapes(cfg):
    D = cfg["hidden_size"]
    Hm = int(D * cfg["mlp_ratio"])
    return {f"blocks.{i}.{lin}": s for i in range(cfg["depth"])
            for lin, s in (("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("mlp.fc1", (Hm, D)), ("mlp.fc2", (D, Hm)))}


def build_lora_model(cfg, dev, seed, R, alpha=None, fill=True, **kw):
    from reed_amd.models.sit import SiT
    m = SiT(input_size=cfg["input_size"], patch_size=cfg["patch_size"], in_channels=cfg["in_channels"],
            hidden_size=cfg["hidden_size"], decoder_hidden_size=cfg["hidden_size"], depth=cfg["depth"],
            num_heads=cfg["num_heads"], num_classes=cfg["num_classes"], z_dims=cfg["z_dims"], z_types=cfg["z_types"],
            encoder_depth=cfg["encoder_depth"], encoder_depth_text=cfg["encoder_depth_text"],
            projector_dim=cfg["projector_dim"], class_dropout_prob=cfg["class_dropout_prob"],
            fused_attn=cfg["fused_attn"], qk_norm=cfg["qk_norm"], lora_rank=R, lora_alpha=alpha, **kw)
    sd = m.state_dict()
    detfill.fill_state_dict(sd, base_seed=seed)
    if fill:
        with torch.no_grad():
            for k, v in adapter_fill(linear_shapes(cfg), R).items():
                sd[k].copy_(v)
    return m.to(dev)


def run(m, dev, name, inference=False):
    cfg, x, t, y, drop = _case(name)
    m.train()
    m.force_drop_mask = drop
    out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=inference)
    return out, zs


def oracle_adapter_grads(name, R):
    """{"f64": {adapter: grad}, "bf16": {...}} of the oracle with P[weight] = W + s B A: once per (case, R), shared, never modified."""
    key = (name, R)
    if key not in _REF:
        cfg, x, t, y, drop = _case(name)
        res = {}
        for tag, dt_, auto in (("f64", torch.float64, False), ("bf16", torch.float32, True)):
            P = detfill.fill_state_dict(osit.init_params(cfg, dtype=dt_), base_seed=11)
            ad = {k: v.to(dt_).requires_grad_(True) for k, v in adapter_fill(linear_shapes(cfg), R).items()}
            for lin in linear_shapes(cfg):
                P[lin + ".weight"] = P[lin + ".weight"] + 2.0 * (ad[lin + ".lora_B"] @ ad[lin + ".lora_A"])
            om = osit.OracleModel(P, cfg, autocast_bf16=auto, training=True)
            om.drop_mask = drop
            out, zs = om(x.to(dt_), t.to(dt_), y, False)
            functional(out, zs).backward()
            res[tag] = {k: v.grad.double() for k, v in ad.items()}
        _REF[key] = res
    return _REF[key]


@pytest.mark.parametrize("kind", KINDS)
def test_fresh_adapters_change_nothing(dev, kind):
    cfg = TINY_CASES["hd64"]["cfg"]
    plain = build_hip_model(cfg, dev, 11)
    fresh = build_lora_model(cfg, dev, 11, 8, 16, fill=False)
    plain.precision = fresh.precision = kind
    o0, z0 = run(plain, dev, "hd64")
    o1, z1 = run(fresh, dev, "hd64")
    assert torch.equal(bits(o0), bits(o1)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(z0, z1))
    functional(o0, z0).backward()
    functional(o1, z1).backward()
    torch.cuda.synchronize()
    g0 = {n: p.grad for n, p in plain.named_parameters()}
    seen = 0
    for n, p in fresh.named_parameters():
        base = any(n == w or n == w[:-6] + "bias" for _, w, _, _ in fresh._layout.lora)
        if base or n == "pos_embed":
            assert p.grad is None, n
        elif lora.is_adapter_key(n):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
            assert n.endswith("lora_A") == (float(p.grad.abs().max()) == 0.0), n     # B = 0: dA = 0, dB is not
        else:
            assert torch.equal(bits(p.grad), bits(g0[n])), n
            seen += 1
    assert seen > 10
    with torch.no_grad():
        assert torch.equal(bits(plain(*[v.to(dev) for v in _case("hd64")[1:4]])[0]), bits(fresh(*[v.to(dev) for v in _case("hd64")[1:4]])[0]))


@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("kind,name", [(k, n) for k in KINDS for n in CASES_16 + (("hd72",) if k == "fp32" else ())])
def test_adapter_gradients_vs_oracle(dev, kind, name, R):
    ref = oracle_adapter_grads(name, R)
    m = build_lora_model(TINY_CASES[name]["cfg"], dev, 11, R, 2 * R)
    m.precision = kind
    out, zs = run(m, dev, name)
    functional(out, zs).backward()
    torch.cuda.synchronize()
    worst = [1.0, 0.0, 1.0, 0.0]
    for n, p in m.named_parameters():
        if not lora.is_adapter_key(n):
            continue
        g, g64, gb = p.grad.cpu().double(), ref["f64"][n], ref["bf16"][n]
        assert float(g64.norm()) >= 0.95, (n, float(g64.norm()))
        cs, dn = cos(g, g64), abs(float(g.norm() / g64.norm()) - 1)
        worst = [min(worst[0], cs), max(worst[1], dn), min(worst[2], cos(g, gb)), max(worst[3], abs(float(g.norm() / gb.norm()) - 1))]
        if kind == "fp32":
            assert cs > 1 - 1e-6 and dn < 1e-4, (n, cs, dn)
        else:
            assert cs >= GRAD_BAR[0] and dn <= 0.012, (n, cs, dn)
    for n, p in m.named_parameters():
        if any(n == w or n == w[:-6] + "bias" for _, w, _, _ in m._layout.lora):
            assert p.grad is None, n
    print(f"[lora grads {kind} {name} R={R}] vs fp64 oracle: worst cosine {worst[0]:.8f}, worst |norm ratio - 1| {worst[1]:.2e} || vs "
          f"bf16-autocast oracle: worst cosine {worst[2]:.8f}, norm {worst[3]:.2e}")


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_three_optimizer_steps_adapters_only(dev, kind, overlap):
    from reed_amd import ops
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.train import apply_lora_freeze
    cfg = TINY_CASES["hd64"]["cfg"]
    m = build_lora_model(cfg, dev, 11, 8, 16)
    m.precision = kind
    apply_lora_freeze(m)
    ema = copy.deepcopy(m).requires_grad_(False).eval()
    ema.precision = kind
    opt = FusedAdamWEMA(m, ema, lr=1e-3, overlap=overlap)
    m.engine().dgrad_nt = True
    L, A = m._layout, m._arena
    before = A.master.clone()
    for _ in range(3):
        out, zs = run(m, dev, "hd64")
        functional(out, zs).backward()
        opt.step()
        opt.zero_grad()
    opt.flush()
    torch.cuda.synchronize()
    adapters = {n for n, _ in m.named_parameters() if lora.is_adapter_key(n)}
    for n, p in m.named_parameters():
        off, num = L.off(n), L.numel(n)
        same = torch.equal(bits(A.master[off:off + num]), bits(before[off:off + num]))
        assert same == (n not in adapters), n
        if n not in adapters and n != "pos_embed":
            assert float(opt.exp_avg[off:off + num].abs().max()) == 0.0 and float(opt.exp_avg_sq[off:off + num].abs().max()) == 0.0, n
    hdt = ops.half_dtype(kind)
    prev = ops.use(kind)
    try:
        if kind != "fp32":      # the transposed copies follow by their own mechanism: behind the optimiser's merges when it overlaps
            A.ensure_shadow_t(kind)     # (fresh already), rebuilt from the merged shadow on demand otherwise
        for arena in (A, ema._arena):
            if arena is ema._arena:
                with torch.no_grad():
                    run(ema.train(), dev, "hd64")
            for _, w, a, b in L.lora:
                n_out, k_in = L.seg[w][1]
                w32 = torch.empty(n_out, k_in, dtype=torch.float32, device=dev)
                ops.lora_merge(arena.view(arena.master, w), arena.view(arena.master, a), arena.view(arena.master, b), L.lora_scale, None,
                               w32, n_out, k_in, 8)
                assert torch.equal(bits(arena.view(arena.shadow, w)), bits(w32.to(hdt))), w
                assert not torch.equal(bits(arena.view(arena.shadow, w)), bits(arena.view(arena.master, w).to(hdt))), w
                if arena is A and kind != "fp32":
                    assert A.shadow_t is not None and A.shadow_t_gen == A.shadow_gen
                    toff = A.t_seg[w][0]
                    assert torch.equal(A.shadow_t[toff:toff + n_out * k_in].view(k_in, n_out), A.view(A.shadow, w).t()), w
    finally:
        ops.use(prev)
    # the EMA copy computes with ITS adapters: a plain model loaded with the EMA's merged weights gives the same bits
    plain = build_hip_model(cfg, dev, 11)
    plain.precision = kind
    plain.load_state_dict(lora.merged_state_dict(ema))
    with torch.no_grad():
        oe, om_, op_ = run(ema, dev, "hd64")[0], run(m, dev, "hd64")[0], run(plain, dev, "hd64")[0]
    assert torch.equal(bits(oe), bits(op_)) and not torch.equal(bits(oe), bits(om_))


def test_gradient_accumulation_matches_full_batch_with_adapters(dev):
    from reed_amd.loss import SILoss
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.train import apply_lora_freeze
    from reed_amd.trainer import TrainStep
    c = TINY_CASES["hd64"]
    cfg = c["cfg"]
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, noise, t, y, drop_u, zs = inputs(8, 4, cfg["input_size"], 31, c["zspec"], T, cfg["num_classes"])
    drop = drop_u < cfg["class_dropout_prob"]
    out = {}
    for accum in (1, 2):
        m = build_lora_model(cfg, dev, 31, 8, 16).train()
        apply_lora_freeze(m)
        ema = copy.deepcopy(m).requires_grad_(False).eval()
        opt = FusedAdamWEMA(m, ema, lr=1e-3)
        step = TrainStep(m, SILoss(enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"]))), opt, None,
                         proj_coeff=0.5, diffusion_warm_up_steps=0, grad_accum=accum)
        n = 8 // accum
        for k in range(accum):
            sl = slice(k * n, (k + 1) * n)
            m.force_drop_mask = drop[sl]
            res = step(x[sl].to(dev), y[sl].to(dev), [z[sl].to(dev) for z in zs], time_input=t[sl], noises=noise[sl])
            assert ("grad_norm" in res) == (k == accum - 1)
        m.state_dict()
        torch.cuda.synchronize()
        L = m._layout
        g = torch.cat([m._arena.grad[L.off(n_):L.off(n_) + L.numel(n_)] for n_, _ in m.named_parameters() if lora.is_adapter_key(n_)])
        out[accum] = (g.clone(), float(res["grad_norm"]))
    g1, g2 = out[1][0], out[2][0]
    assert float(g1.norm()) > 0
    assert torch.nn.functional.cosine_similarity(g1, g2, dim=0).item() > 0.9995
    torch.testing.assert_close(g2.norm(), g1.norm(), rtol=5e-3, atol=0)
    assert abs(out[2][1] / out[1][1] - 1) <= 5e-3


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_merged_export_and_adapter_file(dev, kind, tmp_path):
    from reed_amd.samplers import euler_sampler
    cfg = TINY_CASES["hd64"]["cfg"]
    m = build_lora_model(cfg, dev, 11, 8, 16)
    m.precision = kind
    msd = lora.merged_state_dict(m)
    plain = build_hip_model(cfg, dev, 3)
    plain.precision = kind
    assert list(msd) == list(plain.state_dict()) and all(v.dtype == torch.float32 for v in msd.values())
    plain.load_state_dict(msd)
    with torch.no_grad():
        (o1, z1), (o0, z0) = run(m, dev, "hd64"), run(plain, dev, "hd64")
        assert torch.equal(bits(o1), bits(o0)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(z1, z0))
        _, x, t, y, _ = _case("hd64")
        m.eval(), plain.eval()
        m.force_drop_mask = plain.force_drop_mask = None
        s1 = euler_sampler(m, x.to(dev), y.to(dev), num_steps=3, heun=True, cfg_scale=1.0)
        s0 = euler_sampler(plain, x.to(dev), y.to(dev), num_steps=3, heun=True, cfg_scale=1.0)
    assert torch.equal(s1, s0) and bool(torch.isfinite(s1).all())
    # the adapter file: through torch.save and load_adapter bit for bit, and the loaded model computes the same
    path = tmp_path / "adapter.pt"
    torch.save(lora.adapter_state_dict(m), path)
    other = build_lora_model(cfg, dev, 11, 8, 16, fill=False)
    other.precision = kind
    with torch.no_grad():
        assert not torch.equal(bits(run(other, dev, "hd64")[0]), bits(o1))      # (its shadow exists now: load_adapter must refresh it)
    sd = torch.load(path, map_location="cpu")
    assert sd and all(lora.is_adapter_key(k) for k in sd)
    lora.load_adapter(other, sd)
    a, b = m.state_dict(), other.state_dict()
    assert all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
    with torch.no_grad():
        assert torch.equal(bits(run(other, dev, "hd64")[0]), bits(o1))
    with pytest.raises(KeyError):
        lora.load_adapter(other, {k: v for k, v in sd.items() if "blocks.0.attn.qkv" not in k})
