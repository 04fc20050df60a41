"""The frozen DINOv2 towers at --resolution 512 (448-pixel input, T = 1025 / 1029), in one process, device events after every
shape is warmed:
  (a) the attention forward at (32, 1025, 16, 64) and (32, 1029, 16, 64) beside (32, 1024, 16, 64), the shapes alternating over
      several repeats; the ratio to T = 1024 is the cost of the <= 16-row query tail;
  (b) DINOv2-B / -L towers (registers on) at 448 px, full depth, b = 32 and 64: images/s and the share of the bf16 MFMA peak from
      the FLOPs of the shapes (the four linears 24 T E^2 and attention 4 T^2 E per block, the patch embedding);
  (c) one 512^2 SiT-XL/2 training step at local batch 32 with the DINOv2-B tower run on the raw images every step, against the
      same step with synthetic features.
usage (GPU box): python tools/time_encoder512.py [--attn-only] [--reps N]"""
import argparse
import copy
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reed_amd import ops  # noqa: E402

PEAK_BF16 = 2.5e15   # dense 16-bit MFMA peak, MI355X


def event_time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def attention(reps, iters, B=32, H=16, hd=64):
    fns = {}
    for T in (1024, 1025, 1029):
        g = torch.Generator(device="cuda").manual_seed(T)
        qkv = (torch.randn(B * T, 3 * H * hd, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        o = torch.empty(B * T, H * hd, dtype=torch.bfloat16, device="cuda")
        fns[T] = (lambda qkv=qkv, o=o, T=T: ops.attention_fwd(qkv, o, None, B, T, H, hd))
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {T: [] for T in fns}
    for _ in range(reps):
        for T, f in fns.items():
            times[T].append(event_time(f, iters))
    out = {}
    for T, ts in times.items():
        t = statistics.median(ts)
        out[f"fwd_T{T}"] = {"B": B, "T": T, "H": H, "hd": hd, "us": round(t * 1e6, 1), "us_all": [round(x * 1e6, 1) for x in ts],
                            "tflops": round(4.0 * B * H * T * T * hd / t / 1e12, 1)}
    for T in (1025, 1029):
        out[f"ratio_T{T}_over_T1024"] = round(out[f"fwd_T{T}"]["us"] / out["fwd_T1024"]["us"], 3)
    return out


def tower_flop_per_image(E, depth, T, npatch, patch=14):
    return depth * (24 * T * E * E + 4 * T * T * E) + 2 * npatch * E * 3 * patch * patch


def build_tower(key):
    from oracle import vit_towers as ot
    from reed_amd.encoders import VIT_TOWERS, VitEncoder
    cfg = dict(VIT_TOWERS[key], image=448)
    enc = VitEncoder(**cfg)
    P = ot.fill_params(ot.make_config(cfg["embed"], cfg["depth"], cfg["heads"], 14, 448, True, True, "learned", ls=True,
                                      reg=cfg.get("registers", 0)), base_seed=5)
    enc.load_state_dict(P)
    enc.enc_type = "dinov2"
    return enc.cuda().eval()


def towers(reps, iters):
    out = {}
    for key in ("dinov2reg-vit-b", "dinov2reg-vit-l"):
        enc = build_tower(key)
        flop = tower_flop_per_image(enc.embed, enc.depth, enc.tokens, enc.npatch)
        for b in (32, 64):
            x = torch.randn(b, 3, 448, 448, device="cuda")
            f = lambda: enc(x)   # noqa: E731
            for _ in range(2):
                f()
            torch.cuda.synchronize()
            ts = [event_time(f, iters) for _ in range(reps)]
            t = statistics.median(ts)
            out[f"{key}_b{b}"] = {"tokens": enc.tokens, "ms": round(t * 1e3, 2), "images_per_sec": round(b / t, 1),
                                  "gflop_per_image": round(flop / 1e9, 1), "mfma_frac": round(b * flop / t / PEAK_BF16, 4)}
        del enc
        torch.cuda.empty_cache()
    return out


def train_step_512(b, steps, warm):
    """SiT-XL/2 at 512^2 (T = 1024), 768-d alignment target, bf16: the step on synthetic features, then the same step with the
    DINOv2-B tower (registers, full depth) producing the target from raw uint8 512^2 images each step."""
    from reed_amd.encoders import preprocess_raw_image  # noqa: F401
    from reed_amd.loss import SILoss
    from reed_amd.models.sit import SiT_models
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.trainer import TrainStep
    torch.manual_seed(0)
    model = SiT_models["SiT-XL/2"](input_size=64, z_dims=[768], z_types=["i"], encoder_depth=8).cuda().train()
    model.precision = "bf16"
    ema = copy.deepcopy(model).requires_grad_(False).eval()
    opt = FusedAdamWEMA(model, ema, lr=1e-4, max_grad_norm=1.0)
    step = TrainStep(model, SILoss(enc_names=["dinov2"], loss_weights={"dinov2": 1.0}), opt, None, proj_coeff=0.5,
                     diffusion_warm_up_steps=0)
    g = torch.Generator(device="cuda").manual_seed(100)
    mean = torch.randn(b, 4, 64, 64, device="cuda", generator=g) * 5.49
    moments = torch.cat([mean, torch.full_like(mean, 0.5)], dim=1)
    labels = torch.randint(0, 1000, (b,), device="cuda", generator=g)
    zs = [torch.randn(b, 1024, 768, device="cuda", generator=g)]
    raw = torch.randint(0, 256, (b, 3, 512, 512), device="cuda", dtype=torch.uint8, generator=g)
    enc = build_tower("dinov2reg-vit-b")
    out = {}
    for name, zfn in (("synthetic_features", lambda: zs), ("dinov2_b_tower", lambda: [enc.encode_raw(raw)])):
        for _ in range(warm):
            step(None, labels, zfn(), moments=moments)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(None, labels, zfn(), moments=moments)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        out[name] = {"local_batch": b, "ms_per_step": round(dt * 1e3, 2), "images_per_sec": round(b / dt, 2)}
    out["tower_share_of_step"] = round(1 - out["synthetic_features"]["ms_per_step"] / out["dinov2_b_tower"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "attention": attention(a.reps, a.iters)}
    if not a.attn_only:
        out["towers_448"] = towers(3, 5)
        out["step_512_b32"] = train_step_512(32, a.steps, a.warmup)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
