"""One SiT-XL/2 training step (loss, backward, fused AdamW + EMA; 1024-d alignment) at `--mixed-precision no` arithmetic with and
without the split fp32 GEMM (SiT.tf32: --allow-tf32), alternated in one process on two models with the same weights.

    python tools/_ab/time_step_f32.py [--batch 32] [--steps 3] [--rounds 3] [--out FILE]

Per mode: the median over rounds of the mean wall time of `steps` steps ending in a device synchronise, and the last loss."""
import argparse
import copy
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reed_amd.loss import SILoss  # noqa: E402
from reed_amd.models.sit import SiT_models  # noqa: E402
from reed_amd.optim import FusedAdamWEMA  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="SiT-XL/2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    base = SiT_models[a.model](z_dims=[1024], z_types=["i"], encoder_depth=8)
    runs = {}
    for tf32 in (False, True):
        m = copy.deepcopy(base).to(dev).train()
        m.precision, m.tf32 = "fp32", tf32
        ema = copy.deepcopy(m).requires_grad_(False).eval()
        ema.precision, ema.tf32 = "fp32", tf32
        runs[tf32] = (m, FusedAdamWEMA(m, ema, lr=1e-4, max_grad_norm=1.0), SILoss(enc_names=["dinov2"], loss_weights={"dinov2": 1.0}))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(a.batch, 4, 32, 32, device=dev, generator=g)
    y = torch.randint(0, 1000, (a.batch,), device=dev, generator=g)
    zs = [torch.randn(a.batch, 256, 1024, device=dev, generator=g)]
    times, loss = {False: [], True: []}, {}

    def steps(tf32, n):
        m, opt, lf = runs[tf32]
        torch.manual_seed(7)                          # the same draws of t and noise in both modes
        for _ in range(n):
            out = lf(m, x, dict(y=y), zs=zs)
            total = out["denoising_loss"].mean() + 0.5 * out["proj_loss"].mean()
            opt.zero_grad()
            total.backward()
            opt.step()
        torch.cuda.synchronize()
        loss[tf32] = float(total.detach())

    for tf32 in runs:
        steps(tf32, 1)                                # warm up: code objects, arenas, workspaces
    for _ in range(a.rounds):
        for tf32 in runs:
            t0 = time.perf_counter()
            steps(tf32, a.steps)
            times[tf32].append((time.perf_counter() - t0) / a.steps)
    ms = {k: statistics.median(v) * 1e3 for k, v in times.items()}
    lines = [f"# tools/_ab/time_step_f32.py --batch {a.batch} --steps {a.steps} --rounds {a.rounds}: {a.model}, fp32 operands, "
             f"{torch.cuda.get_device_name(0)}",
             f"exact fp32 GEMM : {ms[False]:8.1f} ms / step ({a.batch / ms[False] * 1e3:6.1f} images/s), loss {loss[False]:.5f}",
             f"split (tf32)    : {ms[True]:8.1f} ms / step ({a.batch / ms[True] * 1e3:6.1f} images/s), loss {loss[True]:.5f}",
             f"speed-up        : {ms[False] / ms[True]:.2f}x"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
