"""Training at 512^2 (latent 64, T = 1024 tokens): the whole forward and backward of the HIP path through the 16-bit attention
backward past 256 tokens (csrc/attention.hip:attn_bwd_long_kernel), against the same-precision oracle and the reference's own fp32
outputs at that size (tests/golden/tiny512.npz, tools/gen_golden.py --only tiny512); a short trajectory; the CLI end to end."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import detfill
from oracle import loss as oloss
from oracle import sit as osit
from tests.test_model_gpu import FP16_TRAIN_COS_BAR, GRAD_BAR, GRAD_BAR_REF_COS, build_hip_model, cos
from tests.test_oracle_golden import TINY_CASES, inputs, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B512 = 2
PROBES = ("final_layer.linear.weight", "final_layer.linear.bias", "blocks.0.attn.qkv.bias", "x_embedder.proj.weight",
          "x_embedder.proj.bias", "blocks.1.adaLN_modulation.1.bias", "blocks.2.mlp.fc1.bias", "projectors.0.4.bias")


def _case(name):
    """The tiny case at input_size 64: hd64 (2 heads of 64) and xl3 (D 1152, 16 heads of 72).  (The tiny hd72 case's D = 144 is
    not a width the 16-bit GEMM tiles take, test_fp32_gpu.py; head_dim 72 is xl3's.)"""
    c = dict(TINY_CASES[name])
    c["cfg"] = dict(c["cfg"], input_size=64)
    return c


def _hip_fwd_bwd(dev, c, precision, scale=1.0):
    from reed_amd.loss import SILoss
    cfg = c["cfg"]
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    assert T == 1024
    x, noise, t, y, drop_u, zs = inputs(B512, 4, cfg["input_size"], 11, c["zspec"], T, cfg["num_classes"])
    drop = drop_u < cfg["class_dropout_prob"]
    m = build_hip_model(cfg, dev, 11)
    m.precision = precision
    m.train()
    m.force_drop_mask = drop
    lf = SILoss(enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"])))
    out = lf(m, x.to(dev), dict(y=y.to(dev)), zs=[z.to(dev) for z in zs], time_input=t, noises=noise)
    total = out["denoising_loss"].mean() + 0.5 * out["proj_loss"]
    (total * scale).backward()
    torch.cuda.synchronize()
    return m, out, total, (x, noise, t, y, drop, zs)


@pytest.mark.parametrize("name", ["hd64", "xl3"])
def test_tiny512_vs_reference_and_oracle(dev, name):
    """bf16: loss and every parameter's gradient (cosine and norm at GRAD_BAR) against the bf16-autocast oracle; the loss, every
    gradient norm and the element probes against the fp32 reference at 512^2, at the bars of test_tiny_vs_reference_and_oracle."""
    g = load("tiny512")
    c = _case(name)
    cfg = c["cfg"]
    m, out, total, (x, noise, t, y, drop, zs) = _hip_fwd_bwd(dev, c, "bf16")
    P = detfill.fill_state_dict(osit.init_params(cfg), base_seed=11)
    P = {k: v.requires_grad_(k != "pos_embed") for k, v in P.items()}
    om = osit.OracleModel(P, cfg, autocast_bf16=True, training=True)
    om.drop_mask = drop
    oo = oloss.si_loss(om, x, dict(y=y), zs, enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"])), t=t, noise=noise)
    (oo["denoising_loss"].mean() + 0.5 * oo["proj_loss"]).backward()
    np.testing.assert_allclose(out["denoising_loss"].detach().cpu().numpy(), oo["denoising_loss"].detach().numpy(), rtol=5e-3)
    np.testing.assert_allclose(float(out["proj_loss"]), float(oo["proj_loss"]), rtol=2e-2, atol=2e-3)
    np.testing.assert_allclose(out["denoising_loss"].detach().cpu().numpy(), g[f"{name}.denoising_loss"], rtol=2e-2)
    np.testing.assert_allclose(float(total), float(g[f"{name}.total"]), rtol=2e-2)
    cmin, nmax = GRAD_BAR
    bad, worst = [], [1.0, 0.0, 0.0]
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        gh, go = p.grad.detach().cpu().float(), P[k].grad
        assert torch.isfinite(gh).all(), k
        nh, no = gh.norm().item(), go.norm().item()
        if no < 5e-5:
            assert nh < 5e-4, (k, nh, no)
            continue
        cs, dn = cos(gh, go), abs(nh / no - 1)
        dref = abs(nh / float(g[f"{name}.gnorm.{k}"]) - 1)
        worst = [min(worst[0], cs), max(worst[1], dn), max(worst[2], dref)]
        if cs < cmin or dn > nmax or dref > 3 * nmax:
            bad.append((k, cs, dn, dref))
    print(f"[512 {name}] worst cosine {worst[0]:.6f}, |norm ratio - 1| vs bf16 oracle {worst[1]:.5f}, vs fp32 reference {worst[2]:.5f}")
    assert not bad, bad[:8]
    params = dict(m.named_parameters())
    for k in PROBES:
        cs = cos(params[k].grad.detach().cpu(), torch.from_numpy(g[f"{name}.grad.{k}"]))
        assert cs > GRAD_BAR_REF_COS, (k, cs)


@pytest.mark.parametrize("name", ["hd64", "xl3"])
def test_tiny512_fp16_vs_reference(dev, name):
    """--mixed-precision fp16 (the IEEE-half library, loss x 1024 as the scaler does): the loss, every parameter's unscaled gradient
    norm and the element probes against the fp32 reference at 512^2 — fp16 carries 3 more mantissa bits than bf16, so the bf16
    path's bars against the same reference hold."""
    g = load("tiny512")
    c = _case(name)
    m, out, total, _ = _hip_fwd_bwd(dev, c, "fp16", scale=1024.0)
    np.testing.assert_allclose(float(total.detach()), float(g[f"{name}.total"]), rtol=2e-2)
    np.testing.assert_allclose(out["denoising_loss"].detach().cpu().numpy(), g[f"{name}.denoising_loss"], rtol=2e-2)
    worst = [0.0, ""]
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert torch.isfinite(p.grad).all(), k
        ref = float(g[f"{name}.gnorm.{k}"])
        nh = p.grad.detach().double().norm().item() / 1024.0
        if ref < 5e-5:
            assert nh < 5e-4, (k, nh, ref)
            continue
        d = abs(nh / ref - 1)
        if d > worst[0]:
            worst = [d, k]
    params = dict(m.named_parameters())
    worst_c = min(cos(params[k].grad.detach().cpu() / 1024.0, torch.from_numpy(g[f"{name}.grad.{k}"])) for k in PROBES)
    print(f"[512 fp16 {name}] worst |norm ratio - 1| vs fp32 reference {worst[0]:.5f} ({worst[1]}), worst probe cosine {worst_c:.6f}")
    assert worst[0] <= 3 * GRAD_BAR[1], worst
    assert worst_c >= FP16_TRAIN_COS_BAR, worst_c


def _trajectory(dev, precision):
    from reed_amd.loss import SILoss
    from reed_amd.optim import FusedAdamWEMA
    c = _case("xl3")
    cfg = c["cfg"]
    m = build_hip_model(cfg, dev, 3)
    m.precision = precision
    m.train()
    opt = FusedAdamWEMA(m, None, lr=1e-4, max_grad_norm=1.0)
    lf = SILoss(enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"])))
    losses = []
    x, noise, t, y, drop_u, zs = inputs(4, 4, 64, 40, c["zspec"], 1024, cfg["num_classes"])   # one batch: the loss must not rise
    m.force_drop_mask = drop_u < cfg["class_dropout_prob"]
    for _ in range(3):
        out = lf(m, x.to(dev), dict(y=y.to(dev)), zs=[z.to(dev) for z in zs], time_input=t, noises=noise)
        total = out["denoising_loss"].mean() + 0.5 * out["proj_loss"]
        total.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(total.detach()))
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_trajectory512_is_finite_bounded_and_deterministic(dev, precision):
    """3 FusedAdamWEMA steps (lr 1e-4) of the tiny xl3 model at 512^2 on one batch of 4 (same t and noise): finite losses, none above
    the first (within 2 %), and a second run from the same start gives identical losses and parameters, bit for bit."""
    l1, p1 = _trajectory(dev, precision)
    l2, p2 = _trajectory(dev, precision)
    print(f"[512 trajectory {precision}] losses {l1}")
    assert all(np.isfinite(v) for v in l1)
    assert max(l1[1:]) <= l1[0] * 1.02
    assert l1 == l2
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))


def test_train512_cli_and_generate(dev, tmp_path):
    """`python -m reed_amd.train --resolution 512` (SiT-S/2, fp16 by default as the reference, synthetic latents with alignment)
    in a child process writes a checkpoint; generate.py --resolution 512 loads it and samples 2 latents without the VAE."""
    out = tmp_path / "exps"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "reed_amd.train", "--exp-name", "r512", "--resolution", "512", "--model", "SiT-S/2",
                        "--output-dir", str(out), "--synthetic", "8", "--batch-size", "4", "--max-train-steps", "2",
                        "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none", "--checkpointing-steps", "2",
                        "--enc-type", "dinov2-vit-b"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    ck = sorted(glob.glob(str(out / "*" / "checkpoints" / "*.pt")))
    assert ck and os.path.basename(ck[-1]) == "0000002.pt", ck
    c = torch.load(ck[-1], map_location="cpu", weights_only=False)
    assert c["args"]["resolution"] == 512 if isinstance(c["args"], dict) else c["args"].resolution == 512
    assert c["model"]["pos_embed"].shape[1] == 1024
    r = subprocess.run([sys.executable, "-m", "reed_amd.generate", "--ckpt", ck[-1], "--model", "SiT-S/2", "--resolution", "512",
                        "--sample-dir", str(tmp_path / "samples"), "--per-proc-batch-size", "2", "--num-fid-samples", "2",
                        "--num-steps", "3", "--save-latents"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lat = glob.glob(str(tmp_path / "samples" / "*_latents.npz"))
    assert len(lat) == 1
    a = np.load(lat[0])["arr_0"]
    assert a.shape == (2, 4, 64, 64) and np.isfinite(a).all()
