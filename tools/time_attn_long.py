"""The 16-bit attention past 256 tokens (512^2: T = 1024) beside the T = 256 kernels at the same token count, in one process:
  (a) backward, ws form: (B 32, T 1024, H 16, hd 72) on attn_bwd_long_kernel (+ delta row kernel + partial-dQ reduce) against
      (B 128, T 256) on attn_bwd_ring_kernel — device events after warm-up, the two shapes alternating over several repeats;
  (b) forward at the same two shapes (T > 256 runs the non-persistent attn_fwd_kernel);
  (c) a SiT-XL/2 training step through TrainStep (synthetic latents, 1024-d alignment, bf16) at 512^2 / local batch 32 and at
      256^2 / local batch 128, in images/s, with the step's MFMA share from FLOPs per image computed from the model's shapes.
Achieved TFLOP/s count algorithmic products at the unpadded head_dim: 2 per (query, key) pair and head_dim column in the forward,
5 products = 10 in the backward.  usage (GPU box): python tools/time_attn_long.py [--attn-only] [--steps N]"""
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
H, HD = 16, 72
D = H * HD


def sit_xl_flop_per_image_step(T, z_dim=1024, proj=2048, depth=28, mlp=4, patch=2, cin=4):
    """Forward FLOPs of SiT-XL/2 per image from the shapes (x 3 for forward + backward): the blocks' four linears
    (24 T D^2), attention (4 T^2 D), the projector MLP on every token, patch embedding and final layer; adaLN rows are per image."""
    blocks = depth * (2 * T * D * (3 * D + D + 2 * mlp * D) + 4 * T * T * D + 2 * D * 6 * D)
    projector = 2 * T * (D * proj + proj * proj + proj * z_dim)
    embed = 2 * T * cin * patch * patch * D + 2 * T * D * patch * patch * cin * 2 + 2 * D * 2 * D
    return 3.0 * (blocks + projector + embed)


def attn_case(B, T):
    g = torch.Generator(device="cuda").manual_seed(B + T)
    qkv = (torch.randn(B * T, 3 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    do = torch.randn(B * T, D, device="cuda", generator=g).to(torch.bfloat16)
    o = torch.empty(B * T, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, T, device="cuda")
    dqkv = torch.empty(B * T, 3 * D, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ops.attention_bwd_ws_floats(B, T, H), device="cuda")
    fwd = lambda: ops.attention_fwd(qkv, o, lse, B, T, H, HD)          # noqa: E731
    bwd = lambda: ops.attention_bwd(qkv, o, do, lse, dqkv, B, T, H, HD, ws=ws)   # noqa: E731
    fwd()
    return fwd, bwd


def event_time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def attention(reps, iters):
    shapes = {"long": (32, 1024), "ring": (128, 256)}
    fns = {k: attn_case(*v) for k, v in shapes.items()}
    for f, b in fns.values():   # warm-up
        for _ in range(5):
            f()
            b()
    torch.cuda.synchronize()
    times = {(k, w): [] for k in shapes for w in ("fwd", "bwd")}
    for _ in range(reps):
        for k in shapes:
            for w, fn in zip(("fwd", "bwd"), fns[k]):
                times[(k, w)].append(event_time(fn, iters))
    out = {}
    for k, (B, T) in shapes.items():
        pairs = B * H * T * T
        for w, mult in (("fwd", 4.0), ("bwd", 10.0)):
            t = statistics.median(times[(k, w)])
            out[f"{w}_{k}"] = {"B": B, "T": T, "H": H, "hd": HD, "us": round(t * 1e6, 1),
                               "us_all": [round(x * 1e6, 1) for x in times[(k, w)]],
                               "tflops": round(mult * pairs * HD / t / 1e12, 1), "mfma_frac": round(mult * pairs * HD / t / PEAK_BF16, 4)}
    out["bwd_ratio_long_over_ring"] = round(out["bwd_long"]["us"] / out["bwd_ring"]["us"], 3)
    out["fwd_ratio_long_over_ring"] = round(out["fwd_long"]["us"] / out["fwd_ring"]["us"], 3)
    out["bwd_partial_dq_bytes"] = 2 * 32 * 1024 * D * 4 * 4   # 4 slices written by the kernel, read by the reduce
    return out


def train_step(res, b, steps, warm):
    from reed_amd.loss import SILoss
    from reed_amd.models.sit import SiT_models
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.trainer import TrainStep
    lat = res // 8
    T = (lat // 2) ** 2
    torch.manual_seed(0)
    model = SiT_models["SiT-XL/2"](input_size=lat, z_dims=[1024], z_types=["i"], encoder_depth=8).cuda().train()
    model.precision = "bf16"
    ema = copy.deepcopy(model).requires_grad_(False).eval()
    opt = FusedAdamWEMA(model, ema, lr=1e-4, max_grad_norm=1.0)
    step = TrainStep(model, SILoss(enc_names=["dinov2-vit-l"], loss_weights={"dinov2-vit-l": 1.0}), opt, None, proj_coeff=0.5,
                     diffusion_warm_up_steps=0)
    g = torch.Generator(device="cuda").manual_seed(100)
    mean = torch.randn(b, 4, lat, lat, device="cuda", generator=g) * 5.49
    moments = torch.cat([mean, torch.full_like(mean, 0.5)], dim=1)
    labels = torch.randint(0, 1000, (b,), device="cuda", generator=g)
    zs = [torch.randn(b, T, 1024, device="cuda", generator=g)]
    res_ = None
    for _ in range(warm):
        res_ = step(None, labels, zs, moments=moments)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        res_ = step(None, labels, zs, moments=moments)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    loss = float(res_["denoising_loss"]) if isinstance(res_, dict) and "denoising_loss" in res_ else None
    flop = sit_xl_flop_per_image_step(T)
    ips = b / dt
    del model, ema, opt, step
    torch.cuda.empty_cache()
    return {"resolution": res, "T": T, "local_batch": b, "ms_per_step": round(dt * 1e3, 2), "images_per_sec": round(ips, 2),
            "gflop_per_image_step": round(flop / 1e9, 1), "step_mfma_frac": round(ips * flop / PEAK_BF16, 4),
            "last_denoising_loss": loss}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "attention": attention(a.reps, a.iters)}
    if not a.attn_only:
        out["step_512_b32"] = train_step(512, 32, a.steps, a.warmup)
        out["step_256_b128"] = train_step(256, 128, a.steps, a.warmup)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
