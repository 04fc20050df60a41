"""The split fp32 GEMM (ops.f32_split; SiT.tf32, --allow-tf32, --sample-precision tf32, precision="tf32" of the VAE passes) at
the level of the model: the tiny cases and the samplers against the reference's own fp32 outputs (tests/golden), a train.py step,
the SD-VAE encoder against fp64.  "TF32's mantissa" has a number in this project already — the bars the IEEE-half build is held
to in tests/test_model_gpu.py::test_fp16_training_gradients_vs_reference — and the split mode is held to those, and in the same
test to lying between the exact fp32 build and the fp16 build."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import detfill
from tests.test_model_gpu import FP16_TRAIN_COS_BAR, FP16_TRAIN_LOSS_BAR, FP16_TRAIN_NORM_BAR, build_hip_model, cos
from tests.test_oracle_golden import TINY_CASES, inputs, load, tiny_cfg
from tests.test_vae_encoder_gpu import _err, _random_encoder, _raw

pytestmark = pytest.mark.gpu

PROBES = ("final_layer.linear.weight", "blocks.0.attn.qkv.bias", "x_embedder.proj.weight", "projectors.0.4.bias",
          "blocks.1.adaLN_modulation.1.bias")


def _tiny(dev, name, precision, tf32):
    """One loss + backward + eval forward of a tiny case -> its errors against the reference's fp32 golden."""
    from reed_amd.loss import SILoss
    g = load("tiny")
    c = TINY_CASES[name]
    cfg = c["cfg"]
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, noise, t, y, drop_u, zs = inputs(4, 4, cfg["input_size"], 11, c["zspec"], T, cfg["num_classes"])
    m = build_hip_model(cfg, dev, 11)
    m.precision, m.tf32 = precision, tf32
    m.train()
    m.force_drop_mask = drop_u < cfg["class_dropout_prob"]
    lf = SILoss(enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"])))
    out = lf(m, x.to(dev), dict(y=y.to(dev)), zs=[z.to(dev) for z in zs], time_input=t, noises=noise)
    total = out["denoising_loss"].mean() + 0.5 * out["proj_loss"]
    scale = 1024.0 if precision == "fp16" else 1.0      # (half gradients underflow unscaled: as the fp16 training test)
    (total * scale).backward()
    torch.cuda.synchronize()
    e = dict(loss=abs(float(total.detach()) / float(g[f"{name}.total"]) - 1),
             den=float(np.abs(out["denoising_loss"].detach().cpu().numpy() / g[f"{name}.denoising_loss"] - 1).max()), norm=0.0, cos=1.0)
    params = dict(m.named_parameters())
    for k, p in params.items():
        if not p.requires_grad:
            continue
        ref = float(g[f"{name}.gnorm.{k}"])
        nh = p.grad.detach().double().norm().item() / scale
        if ref < 5e-5:
            assert nh < 5e-4, (k, nh, ref)
            continue
        e["norm"] = max(e["norm"], abs(nh / ref - 1))
    for k in PROBES:
        e["cos"] = min(e["cos"], cos(params[k].grad.detach().cpu() / scale, torch.from_numpy(g[f"{name}.grad.{k}"])))
    m.eval()
    m.force_drop_mask = None
    xi, _, ti, yi, _, _ = inputs(4, 4, cfg["input_size"], 11, [], 0, 10)
    with torch.no_grad():
        o, _ = m(xi.to(dev), ti.to(dev), yi.to(dev))
    ref = torch.from_numpy(g[f"{name}.infer"])
    e["infer"] = (o.float().cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    return e


@pytest.mark.parametrize("name", ["hd64", "hd72"])
def test_tiny_split_vs_reference(dev, name):
    """hd64 and hd72 at precision "fp32" with the split on against the reference's fp32 goldens, at the bars of the fp16 training
    test (loss 1e-3, every gradient norm 1e-3, probe cosines 0.9999; the eval forward at the loss bar), and between the exact fp32
    build and the fp16 build on the loss and on the worst gradient-norm ratio.  (hd72 has D = 144, which the 16-bit tiles do not
    take — TINY_CASES marks it so: there the fp16 column is absent and the order is checked against fp32 alone.)"""
    from reed_amd import ops
    errs = {"fp32": _tiny(dev, name, "fp32", False), "split": _tiny(dev, name, "fp32", True)}
    if TINY_CASES[name]["hip"]:
        errs["fp16"] = _tiny(dev, name, "fp16", False)
    assert not ops.f32_split_on() and ops._PRECISION == "bf16"
    for k, e in errs.items():
        print(f"[tf32 {name}] {k:5}: loss {e['loss']:.3e}  denoising {e['den']:.3e}  worst |gradient norm ratio - 1| {e['norm']:.3e}  "
              f"worst probe cosine {e['cos']:.8f}  eval forward {e['infer']:.3e}")
    s = errs["split"]
    assert s["loss"] <= FP16_TRAIN_LOSS_BAR and s["den"] <= FP16_TRAIN_LOSS_BAR and s["infer"] <= FP16_TRAIN_LOSS_BAR, s
    assert s["norm"] <= FP16_TRAIN_NORM_BAR and s["cos"] >= FP16_TRAIN_COS_BAR, s
    for k in ("loss", "norm"):
        assert errs["fp32"][k] <= s[k], (k, errs)
        if "fp16" in errs:
            assert s[k] <= errs["fp16"][k], (k, errs)


def test_samplers_split_vs_reference(dev):
    """Euler and Heun + CFG, 6 steps on the tiny SiT: with the split on, the deviation from the reference's outputs in units of the
    latents' scale is below the fp16 build's in the same test."""
    from reed_amd import ops, samplers
    g = load("samplers")
    m = build_hip_model(tiny_cfg(num_classes=1000), dev, 5).eval()
    z = detfill.normal((3, 4, 8, 8), 41).to(dev)
    y = torch.tensor([3, 500, 999], device=dev)
    cfgs = {"euler": dict(heun=False, cfg_scale=1.0), "heun_cfg": dict(heun=True, cfg_scale=1.5)}
    worst = {}
    for mode, (prec, tf32) in {"split": ("fp32", True), "fp16": ("fp16", False)}.items():
        m.precision, m.tf32 = prec, tf32
        for name, c in cfgs.items():
            out = samplers.euler_sampler(m, z, y, num_steps=6, prediction="v", **c)
            ref = torch.from_numpy(g[name])
            assert torch.isfinite(out).all()
            worst[mode, name] = (out.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert not ops.f32_split_on()
    for name in cfgs:
        print(f"[tf32 sampler {name}] deviation of the latents' scale: split {worst['split', name]:.2e}, fp16 {worst['fp16', name]:.2e}")
        assert worst["split", name] < worst["fp16", name], (name, worst)


def test_train_step_with_allow_tf32(dev, tmp_path):
    """`train.py --mixed-precision no --allow-tf32 --synthetic 8`, one step of SiT-S/2: the loss is finite, every GEMM of the step
    is planned as kernel 10 at the moment it is launched, args.json carries the setting and the process-wide mode is off after."""
    from reed_amd import ops, train
    a = train.parse_args(["--exp-name", "tf32", "--model", "SiT-S/2", "--output-dir", str(tmp_path / "exps"), "--batch-size", "8",
                          "--synthetic", "8", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
                          "--enc-type", "None", "--max-train-steps", "1", "--checkpointing-steps", "100",
                          "--mixed-precision", "no", "--allow-tf32"])
    assert a.gemm_tf32 is True
    seen = []

    def probe(lay, epi, M, N, K):
        rc, launches = ops.gemm_plan(lay, epi, M, N, K, precision="fp32")
        seen.append((ops._PRECISION, rc, [l["kernel"] for l in launches]))
        return None

    ops.gemm_probe = probe
    try:
        d = train.main(a)
    finally:
        ops.gemm_probe = None
        torch.set_grad_enabled(True)
    logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    assert len(logs) == 1 and np.isfinite(logs[0]["training_denoising_loss"]) and np.isfinite(logs[0]["grad_norm"])
    assert len(seen) > 50 and all(s == ("fp32", 0, ["f32_split"]) for s in seen), [s for s in seen if s != ("fp32", 0, ["f32_split"])][:5]
    assert json.load(open(os.path.join(d, "args.json")))["gemm_tf32"] is True
    assert not ops.f32_split_on()
    assert ops.gemm_plan(ops.NT, ops.EPI_BF16, 256, 384, 384, precision="fp32")[1][0]["kernel"] == "f32"


def test_vae_encoder_tf32_vs_fp64(dev):
    """SDVAEEncoder.encode(precision="tf32") on a small encoder whose channel counts the fp16 kernels also take, against the module
    on torch operators in fp64: within the bar tests/test_vae_encoder_gpu.py holds fp16 operands to (3e-3 of each half's scale),
    and closer to the oracle than the fp16 result."""
    from reed_amd import ops
    enc = _random_encoder(dict(block_out_channels=(128, 128), layers_per_block=1, norm_num_groups=32), 4, 0.03)
    raw = _raw((2, 3, 24, 16), 6)
    want = enc.double().encode_torch(raw.double() / 127.5 - 1)
    enc = enc.float().to(dev)
    got = {p: enc.encode(raw.to(dev), precision=p).cpu() for p in ("fp32", "tf32", "fp16")}
    assert not ops.f32_split_on() and ops._PRECISION == "bf16"
    assert not torch.equal(got["tf32"], got["fp32"])
    for half, i in (("mean", 0), ("std", 1)):
        e = {p: _err(g, want)[i] for p, g in got.items()}
        print(f"[tf32 vae encoder, {half}] max abs error of scale {e['tf32'][1]:.3f}: " + ", ".join(f"{p} {v[0] / v[1]:.2e}" for p, v in e.items()))
        assert e["tf32"][0] <= 3e-3 * e["tf32"][1]
        assert e["tf32"][0] < e["fp16"][0]
