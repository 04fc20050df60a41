#!/usr/bin/env python
"""The fused w12 launch of DINOv2 ViT-g's SwiGLU feed-forward (reed_gemm epilogue 17: the [M, 2 Hd] pre-activation is consumed in the
epilogue, [M, Hd] written) against the plain launch of the same shape (epilogue 0: [M, 2 Hd] written), which is the floor of the
unfused alternative — that one adds a row pass reading the pre-activation back and writing the product.
usage (GPU box): python tools/swiglu_vs_plain.py [M] [Hd] [K]      default 16448 4096 1536 = ViT-g at batch 64
Alternating rounds of `iters` launches each, device events; prints one JSON line with the median and the spread per form."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reed_amd import ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 16448
Hd = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
K = int(sys.argv[3]) if len(sys.argv) > 3 else 1536
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
w12 = (torch.randn(2 * Hd, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(dev)
b12 = torch.randn(2 * Hd, generator=g).to(torch.bfloat16).to(dev)
pw, pb = ops.swiglu_pack(w12, b12)
full = torch.empty(M, 2 * Hd, dtype=torch.bfloat16, device=dev)
half = torch.empty(M, Hd, dtype=torch.bfloat16, device=dev)


def fused():
    ops.gemm(ops.NT, ops.EPI_SWIGLU, x, pw, M, 2 * Hd, K, half, K, K, Hd, bias=pb)


def plain():
    ops.gemm(ops.NT, ops.EPI_BF16, x, pw, M, 2 * Hd, K, full, K, K, 2 * Hd, bias=pb)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us per launch


for fn in (fused, plain):
    timed(fn, 20)
rounds, iters = 9, 200
t = {"fused": [], "plain": []}
for _ in range(rounds):
    t["fused"].append(timed(fused, iters))
    t["plain"].append(timed(plain, iters))
# the same products, paired: the fused output equals the pairing of the plain one
x12 = full.view(M, Hd // ops.SWIGLU_GROUP, 2, ops.SWIGLU_GROUP).float()
want = ((x12[:, :, 0] * torch.sigmoid(x12[:, :, 0])).to(torch.bfloat16).float() * x12[:, :, 1]).to(torch.bfloat16).reshape(M, Hd)
same = float((want == half).float().mean())
flop = 2.0 * M * 2 * Hd * K
out = {"shape": {"M": M, "N": 2 * Hd, "K": K}, "rounds": rounds, "launches_per_round": iters}
for k, v in t.items():
    med = statistics.median(v)
    out[k] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
              "tflops": round(flop / med / 1e6, 1)}
out["fused_minus_plain_us"] = round(out["fused"]["median_us"] - out["plain"]["median_us"], 1)
out["unfused_row_pass_bytes"] = M * 2 * Hd * 2 + M * Hd * 2      # reads [M, 2 Hd] back, writes [M, Hd]
out["fused_equals_pairing_of_plain"] = round(same, 6)
print(json.dumps(out))
