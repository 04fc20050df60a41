#!/usr/bin/env python
"""Throughput of a frozen ViT target encoder on the HIP path: images/s through preprocess_raw_image + tower
and the tower alone as a fraction of the MFMA roofline of its operand type.
usage (GPU box): python tools/bench_tower.py [enc-type] [batch] [--precision bf16|fp16|fp32]
enc-type: dinov2-vit-l (default; the C2 configuration's encoder), dinov2reg-vit-l, dinov2-vit-b, dinov2-vit-g, dinov2reg-vit-g (SwiGLU
feed-forward: 3 E Hd MACs per token where the others take 8 E^2), jepa-vit-h, mae-vit-l, mocov3-vit-l, clip-vit-L (the CLIP tower of
tools/bench_encoder.py, here for its --precision)
--precision: the library build the tower runs on (train.py --encoder-precision); the roofline is 2500 TFLOP/s for the 16-bit MFMA and
157 for the fp32 one"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reed_amd.encoders import CLIP_CONFIGS, VIT_TOWERS, ClipVisionEncoder, VitEncoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("key", nargs="?", default="dinov2-vit-l")
ap.add_argument("batch", nargs="?", type=int, default=256)
ap.add_argument("--precision", choices=["bf16", "fp16", "fp32"], default="bf16")
a = ap.parse_args()
key, B, prec = a.key, a.batch, a.precision
dev = torch.device("cuda")
clip = key.startswith("clip")
if clip:
    enc = ClipVisionEncoder(**CLIP_CONFIGS[key.split("-")[2][0].upper()], precision=prec)
else:
    enc = VitEncoder(**VIT_TOWERS[key], precision=prec)
    enc.enc_type = key.split("-")[0]
g = torch.Generator().manual_seed(0)
with torch.no_grad():
    for n, p in enc.named_parameters():
        if p.ndim >= 2 and "token" not in n and "pos_embed" not in n:
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (3.0 / p[0].numel()) ** 0.5)
        elif n.endswith("gamma"):
            p.fill_(0.5)
        elif ("norm" in n or "ln_" in n) and n.endswith("weight"):
            p.fill_(1.0)
        else:
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * 0.05)
enc = enc.to(dev).eval()
E, L, T = enc.embed_dim, (enc.layers if clip else enc.depth), enc.tokens
npatch = T - 1 if clip else enc.npatch
ffn_mac = 3 * E * enc.ffn_hidden if not clip and enc.ffn == "swiglu" else 8 * E * E   # w12 + w3 / fc1 + fc2, per token
mac = L * (T * (4 * E * E + ffn_mac) + 2 * T * T * E) + npatch * 3 * enc.patch ** 2 * E
raw = torch.randint(0, 256, (B, 3, 256, 256), dtype=torch.uint8, device=dev)
for _ in range(2):
    out = enc.encode_raw(raw)
torch.cuda.synchronize()
iters = 5
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    out = enc.encode_raw(raw)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / iters
from reed_amd.encoders import preprocess_raw_image  # noqa: E402
x = preprocess_raw_image(raw, "clip" if clip else enc.enc_type)
torch.cuda.synchronize()
e0.record()
for _ in range(iters):
    out = enc(x)
e1.record()
torch.cuda.synchronize()
ms_tower = e0.elapsed_time(e1) / iters
assert bool(torch.isfinite(out).all()) and out.shape == (B, npatch, E)
peak = 157.0 if prec == "fp32" else 2500.0
print(json.dumps({"metric": f"{key} frozen encoder forward images/sec (1 x MI355X, {prec})", "batch": B, "tokens": T,
                  "value": round(B / ms * 1e3, 1), "ms_per_batch": round(ms, 2), "ms_tower_only": round(ms_tower, 2),
                  "gflop_per_image": round(2 * mac / 1e9, 2),
                  "roofline": {"bound": "mfma", "achieved": round(2 * mac * B / ms_tower / 1e9, 1), "peak": peak,
                               "unit": "TFLOP/s", "frac": round(2 * mac * B / ms_tower / 1e9 / peak, 4)}}))
